"""What the nine witness audits have in common at their edges, without a GPU: the Python signatures (names, order, defaults), the refusals the
Python layer makes itself (a trace that is not a matrix, a chip list that is empty or names a chip past 31) with their exact text, and what the
C entry points promise for null arguments (vgpu_X_audit_host with a null `out`: VGPU_ERR_INVALID_ARG and a message; the accessors of a null
report handle: 0, NULL, zeros, nothing freed).  The literals are written down, not derived from the package."""
import ctypes
import inspect

import numpy as np
import pytest

import valida_amd as va

AUDITS = ["bus", "constraint", "mutation", "pair", "rank", "step", "field", "link", "coverage"]
# the options of each audit after (machine, main_matrices, preprocessed) / (self, main, preprocessed): name and default, in order
OPTIONS = {
    "bus": [("max_tuples", 64), ("max_records_per_tuple", 4), ("hash_bits", 64)],
    "constraint": [("max_constraints", 64), ("max_rows_per_constraint", 4)],
    "mutation": [("deltas", None), ("max_entries", 1024), ("max_rows_per_entry", 4)],
    "pair": [("deltas", None), ("max_entries", 1024), ("max_rows_per_entry", 4), ("chips", None)],
    "rank": [("max_entries", 1024), ("max_rows_per_entry", 4), ("chips", None)],
    "step": [("steps", None), ("max_entries", 1024), ("max_rows_per_entry", 4), ("chips", None)],
    "field": [("max_entries", 1024), ("max_rows_per_entry", 4), ("chips", None)],
    "link": [("max_tuples", 64), ("max_records_per_tuple", 4), ("hash_bits", 64)],
    "coverage": [("deltas", None), ("max_cells", 8192)],
}
METHOD_ONLY = {"coverage": [("max_workgroups", 0)]}  # options only the device pass has
TWO_TIMES = ("bus", "constraint")  # vgpu_X_report_timing writes device_ms and host_ms; the others evaluations as well


def signature_of(f):
    return [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()]


def literal(positional, options):
    kind, empty = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.empty
    return [(n, empty, kind) for n in positional] + [(n, d, kind) for n, d in options]


@pytest.fixture(scope="module")
def machine():
    return va.Machine.basic()


@pytest.fixture(scope="module")
def L():
    # a handle of its own: the restypes set here are not the package's
    return ctypes.CDLL(va.lib()._name)


@pytest.mark.parametrize("name", AUDITS)
def test_signatures(name):
    assert signature_of(getattr(va, name + "_audit_host")) == literal(["machine", "main_matrices", "preprocessed"], OPTIONS[name])
    assert signature_of(getattr(va.Prover, name + "_audit")) == literal(["self", "main", "preprocessed"], OPTIONS[name] + METHOD_ONLY.get(name, []))


@pytest.mark.parametrize("name", AUDITS)
def test_a_trace_is_a_matrix(machine, name):
    with pytest.raises(va.VgpuError) as e:
        getattr(va, name + "_audit_host")(machine, [np.zeros(4, dtype=np.uint32)], [])
    assert e.value.code == -1 and str(e.value) == "vgpu error -1: %s_audit: traces are two-dimensional matrices" % name
    with pytest.raises(va.VgpuError) as e:  # a preprocessed one as well
        getattr(va, name + "_audit_host")(machine, [], [(0, np.zeros(4, dtype=np.uint32))])
    assert e.value.code == -1 and str(e.value) == "vgpu error -1: %s_audit: traces are two-dimensional matrices" % name


@pytest.mark.parametrize("name", ["pair", "rank", "step", "field"])
@pytest.mark.parametrize("chips", [[], [32]])
def test_chip_lists(machine, name, chips):
    with pytest.raises(va.VgpuError) as e:
        getattr(va, name + "_audit_host")(machine, [], [], chips=chips)
    assert e.value.code == -1 and str(e.value) == "vgpu error -1: %s_audit: chips is a non-empty list of chip indices below 32" % name


@pytest.mark.parametrize("name", AUDITS)
def test_null_out_is_refused(machine, L, name):
    f = getattr(L, "vgpu_%s_audit_host" % name)
    f.restype = ctypes.c_int32
    L.vgpu_last_error.restype = ctypes.c_char_p
    assert f(machine._h, None, None, None, ctypes.c_uint32(0), None, None, None, None, ctypes.c_uint32(0), None, None) == -1
    assert L.vgpu_last_error()


@pytest.mark.parametrize("name", AUDITS)
def test_null_report_handle(L, name):
    length, words, timing, free = (getattr(L, "vgpu_%s_report_%s" % (name, f)) for f in ("len", "words", "timing", "free"))
    length.restype, words.restype, timing.restype, free.restype = ctypes.c_uint64, ctypes.c_void_p, None, None
    assert length(None) == 0
    assert words(None) is None
    tm = (ctypes.c_double * 3)(7.0, 7.0, 7.0)
    timing(None, tm)
    assert list(tm) == ([0.0, 0.0, 7.0] if name in TWO_TIMES else [0.0, 0.0, 0.0])
    free(None)
