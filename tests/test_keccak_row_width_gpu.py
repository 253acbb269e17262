"""Row widths compiled into the Keccak MMCS kernels (merkle.hip: k_keccak_leaves<Cols, N>, k_keccak_compress<N>) on the device: commitments
whose rows have every width of the kernels' tables, and one width outside them, against the oracle's root.

At 128 rows the default launches are the lane-pair kernels (layers of at most 32768 nodes), which take the width at run time, so the same
shapes — and a taller pair whose injection lands on a layer with a launch of its own — are committed once more in ONE child process with
VGPU_KECCAK_PAIRS=0 (the switch is latched per process): there every launch is a thread-per-node kernel, the instance of its width where the
tables have one.  Which instance the dispatch picks for a width is asserted on the same source under emulation (tests/test_keccak_row_width_cpu.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
P = 2013265921
LEAF_WIDTHS, LEAF_WIDTHS_STRIDED, INJECT_WIDTHS = (10, 14), (10,), (10, 20, 25, 40, 51, 55, 61, 67, 95)  # merkle.hip: VK_LEAF_WIDTHS, .._STRIDED, VK_INJECT_WIDTHS
WIDTHS = sorted(set(LEAF_WIDTHS + LEAF_WIDTHS_STRIDED + INJECT_WIDTHS))
UNLISTED = 13


def matrices(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, P, size=s, dtype=np.uint32) for s in shapes]


def batches(w):
    """name -> shapes of one commitment: a single matrix (one strided view), two equally tall ones (a column list of w columns in all) and
    two mixed-height batches whose injected rows are w wide — under a top-of-tree launch, and at a layer of 1024 nodes (a launch of its own)."""
    return {"single": [(128, w)], "list": [(128, w - w // 2), (128, w // 2)] if w > 1 else [(128, 1)], "mixed": [(128, 3), (64, w)], "mixed_tall": [(1024, 3), (512, w)]}


def device_roots(prover, widths, names):
    out = {}
    for w in widths:
        for name in names:
            mats = matrices(batches(w)[name], 1000 * w + len(name))
            out["%s:%d" % (name, w)] = [int(x) for x in prover.commit_batches([prover.upload(m) for m in mats]).root]
    return out


def oracle_root(name, w):
    from oracle import pyoracle as po

    return [int(x) for x in po.commit_root(matrices(batches(w)[name], 1000 * w + len(name)))]


@pytest.mark.parametrize("w", WIDTHS + [UNLISTED])
def test_commit_roots_of_the_table_widths_match_the_oracle(prover, w):
    got = device_roots(prover, [w], ["single", "list", "mixed"])
    for name in ("single", "list", "mixed"):
        assert got["%s:%d" % (name, w)] == oracle_root(name, w), name


@pytest.fixture(scope="module")
def thread_per_node_child():
    env = dict(os.environ, VGPU_KECCAK_PAIRS="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_thread_per_node_kernels_of_every_table_width_match_the_oracle(thread_per_node_child):
    roots = thread_per_node_child
    for w in WIDTHS + [UNLISTED]:
        for name in ("single", "list", "mixed", "mixed_tall"):
            assert roots["%s:%d" % (name, w)] == oracle_root(name, w), (name, w)


if __name__ == "__main__":  # the child of thread_per_node_child: device roots only (the parent holds the oracle), one JSON line
    import valida_amd as va

    p = va.Prover(va.Machine.basic(), va.poseidon_round_constants())
    print(json.dumps(device_roots(p, WIDTHS + [UNLISTED], ["single", "list", "mixed", "mixed_tall"])))
