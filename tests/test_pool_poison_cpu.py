"""The pool-poison test hook without a GPU: the parser of the Python binding's VGPU_POOL_POISON switch, and the four C entry
points declared, exported and bound.  What the hook finds is tests/test_pool_poison_gpu.py's business."""
import os
import re

import pytest

import valida_amd as va

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("vgpu_prover_set_pool_poison", "vgpu_prover_pool_poison_stats", "vgpu_prover_pool_peek", "vgpu_verifier_set_poison")


@pytest.mark.parametrize("environ", [{}, {"VGPU_POOL_POISON": ""}, {"VGPU_POOL_POISON": "  "}, {"OTHER": "1"}])
def test_unset_or_empty_switch_means_off(environ):
    assert va._pool_poison_from_env(environ) is None


@pytest.mark.parametrize("text,word", [("0xFFFFFFFF", 0xFFFFFFFF), ("1", 1), ("0x5a5a5a5a", 0x5A5A5A5A), ("0", 0), ("4294967295", 0xFFFFFFFF), ("0X00000001", 1), (" 7 ", 7)])
def test_switch_parses_hex_and_decimal_words(text, word):
    assert va._pool_poison_from_env({"VGPU_POOL_POISON": text}) == word


@pytest.mark.parametrize("text", ["-1", "zz", "4294967296", "0x100000000", "0x", "1e3", "1_0", "+1", "0x-1", "12 34"])
def test_switch_refuses_anything_else_and_names_the_variable(text):
    with pytest.raises(ValueError, match="VGPU_POOL_POISON"):
        va._pool_poison_from_env({"VGPU_POOL_POISON": text})


def test_the_parser_reads_its_argument_not_the_process_environment(monkeypatch):
    monkeypatch.setenv("VGPU_POOL_POISON", "zz")
    assert va._pool_poison_from_env({}) is None
    assert va._pool_poison_from_env({"VGPU_POOL_POISON": "3"}) == 3


def test_hooks_are_declared_exported_and_documented_as_test_hooks():
    hdr = open(os.path.join(ROOT, "include", "vgpu.h")).read()
    lib = va.lib()
    for name in HOOKS:
        assert hasattr(lib, name), name
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*\n[^\n;]*\b%s\s*\(" % name, hdr, re.S)
        assert m and "Test hook" in m.group(1), "%s: the comment in front of its declaration must call it a test hook" % name
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in HOOKS:
        assert "pub fn %s(" % name in rust, name


def test_python_binding_has_the_hooks():
    for cls, names in ((va.Prover, ("set_pool_poison", "pool_poison_stats", "pool_peek")), (va.Verifier, ("set_poison",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls.__name__, n)


def test_the_library_itself_reads_no_environment_switch_for_the_hook():
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    for base, _, files in os.walk(csrc):
        for f in files:
            assert "VGPU_POOL_POISON" not in open(os.path.join(base, f)).read(), f
