"""Inputs the invariant audit's CPU and GPU tests share: two captured one-chip machines (an AIR with the one constraint c2 - 3 c0 - 7, and an
AIR without constraints or interactions), their traces, the closed-form Jacobians the reference is given for them, and the "needle" traces
(4096 x 70: a relation that only row 0 or only the last row breaks, and a staircase in which column j first becomes independent in row block
j, so that every workgroup of the streaming elimination finds different pivots and the merge does real work)."""
import ctypes

import numpy as np

import valida_amd as va

P = va.P
NEEDLE_N, NEEDLE_W = 4096, 70


def _machine(name, width, constrained):
    L, u = va.lib(), ctypes.c_uint32
    m, air = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.vgpu_machine_new(ctypes.byref(m)) == 0
    assert L.vgpu_air_new(name, u(width), u(0), ctypes.byref(air)) == 0
    if constrained:
        c0, c2 = L.vgpu_air_variable(air, u(0), u(0), u(0)), L.vgpu_air_variable(air, u(0), u(2), u(0))
        three_c0 = L.vgpu_air_mul(air, u(L.vgpu_air_constant(air, u(3))), u(c0))
        L.vgpu_air_assert_zero(air, u(L.vgpu_air_sub(air, u(L.vgpu_air_sub(air, u(c2), u(three_c0))), u(L.vgpu_air_constant(air, u(7))))))
    assert L.vgpu_machine_push_air(m, air) == 0, L.vgpu_last_error()
    L.vgpu_air_free(air)
    return va.Machine(m)


def affine_machine(width=5):
    """One captured AIR of `width` >= 5 columns with the one constraint c2 - 3 c0 - 7."""
    return _machine(b"affine", width, True)


def free_machine(width):
    """One captured AIR of `width` columns that constrains nothing."""
    return _machine(b"free", width, False)


def affine_trace(n, width=5):
    """c0 = r, c1 = r^2, c2 = 3 c0 + 7, c3 = c0 + c1, c4 = 5; beyond width 5: c_j = (r + 2)^(j - 2) mod p for 5 <= j < width - 1 (independent of
    what is left of them once n > width) and the last column c_(width - 2) + 2 c0 + 1: an invariant in the last lane word."""
    r = np.arange(n, dtype=np.uint64)
    cols = [r, r * r % P, (3 * r + 7) % P, (r + r * r) % P, np.full(n, 5, dtype=np.uint64)]
    for j in range(5, width - 1):
        cols.append(np.array([pow(int(x) + 2, j - 2, P) for x in r], dtype=np.uint64))
    if width > 5:
        cols.append((cols[-1] + 2 * r + 1) % P)
    return np.stack(cols, axis=1).astype(np.uint32)


def affine_jacobians(width=5):
    """The reference's `jacobians` for affine_machine: one constraint, no interaction, J_r = (-3, 0, 1, 0, ..) on every row (the cell read as
    next has derivative zero; for n = 1 the sum over both roles is the same row)."""
    J = np.zeros((1, width), dtype=np.uint64)
    J[0, 0], J[0, 2] = P - 3, 1
    return {0: (1, 0, lambda r: J)}


def free_jacobians(width):
    return {0: (0, 0, lambda r: np.zeros((0, width), dtype=np.uint64))}


def needle(kind):
    """kind 'first' / 'last': 68 random columns, column 68 = 2 c5 + 7 on every row, column 69 = c3 + c10 on every row BUT row 0 / row n - 1:
    the only invariant is column 68.  kind 'stairs': columns 0..67 are zero before row block j (58 rows each) and random from it on, column
    68 = 2 c5 + 7, column 69 = c67 + c0: the invariants are columns 68 and 69."""
    rng = np.random.RandomState(7 if kind == "stairs" else 11)
    n, w = NEEDLE_N, NEEDLE_W
    t = rng.randint(1, P, size=(n, w)).astype(np.uint64)
    if kind == "stairs":
        for j in range(68):
            t[:58 * j, j] = 0
        t[:, 69] = (t[:, 67] + t[:, 0]) % P
    else:
        t[:, 69] = (t[:, 3] + t[:, 10]) % P
        row = 0 if kind == "first" else n - 1
        t[row, 69] = (t[row, 69] + 1) % P
    t[:, 68] = (2 * t[:, 5] + 7) % P
    return t.astype(np.uint32)


NEEDLE_INVARIANTS = {"first": [68], "last": [68], "stairs": [68, 69]}
