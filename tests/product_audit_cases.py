"""Inputs the product audit's CPU and GPU tests share: the captured one-chip machine "quad" (constraints c1^2 - c1 and c1 c2 - c3 only), its
traces, the closed-form Jacobian the reference is given for it, and the "needle" traces (4096 x 40: a product relation that only row 0 or only
the last row breaks, over a staircase in which column j >= 8 is zero before row 100 (j - 8), so that the basis rows lie up to row 3100 and every
slice of the basis-row phase finds different ones)."""
import ctypes

import numpy as np

import valida_amd as va
from invariant_audit_cases import free_jacobians, free_machine  # noqa: F401  (the needles' machine: an AIR that constrains nothing)

P = va.P
NEEDLE_N, NEEDLE_W = 4096, 40


def quad_machine(width=7):
    """One captured AIR of `width` >= 7 columns with the two constraints c1^2 - c1 and c1 c2 - c3."""
    L, u = va.lib(), ctypes.c_uint32
    m, air = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.vgpu_machine_new(ctypes.byref(m)) == 0
    assert L.vgpu_air_new(b"quad", u(width), u(0), ctypes.byref(air)) == 0
    c1, c2, c3 = (L.vgpu_air_variable(air, u(0), u(k), u(0)) for k in (1, 2, 3))
    L.vgpu_air_assert_zero(air, u(L.vgpu_air_sub(air, u(L.vgpu_air_mul(air, u(c1), u(c1))), u(c1))))
    L.vgpu_air_assert_zero(air, u(L.vgpu_air_sub(air, u(L.vgpu_air_mul(air, u(c1), u(c2))), u(c3))))
    assert L.vgpu_machine_push_air(m, air) == 0, L.vgpu_last_error()
    L.vgpu_air_free(air)
    return va.Machine(m)


def quad_trace(n, width=7):
    """c0 = r, c1 = r & 1, c2 = (r >> 1) & 1, c3 = c1 c2, c4 = r^2, c5 = 3 r + 7, c6 = r c1; beyond width 7 filler columns from a fixed-seed
    generator (no product of a filler is a relation)."""
    r = np.arange(n, dtype=np.uint64)
    c1, c2 = r & 1, (r >> 1) & 1
    cols = [r, c1, c2, c1 * c2, r * r % P, (3 * r + 7) % P, r * c1 % P]
    if width > 7:
        cols += list(np.random.RandomState(width).randint(1, P, size=(width - 7, n)).astype(np.uint64))
    return np.stack(cols, axis=1).astype(np.uint32)


def quad_jacobians(t):
    """The reference's `jacobians` for quad_machine on trace t: two constraints, no interaction; at row r the derivatives by the row's own cells
    are (2 c1 - 1) e_1 and c2 e_1 + c1 e_2 - e_3 (nothing is read as next; for n = 1 the sum over both roles is the same)."""
    n, width = t.shape

    def J(r):
        c1, c2 = int(t[r, 1]), int(t[r, 2])
        j = np.zeros((2, width), dtype=np.uint64)
        j[0, 1] = (2 * c1 + P - 1) % P
        j[1, 1], j[1, 2], j[1, 3] = c2, c1, P - 1
        return j

    return {0: (2, 0, J)}


# (i, j) -> the one column of beta (coefficient 1); for 16 <= n
QUAD_RELATIONS = {(0, 0): 4, (0, 1): 6, (1, 1): 1, (1, 2): 3, (1, 3): 3, (1, 6): 6, (2, 2): 2, (2, 3): 3, (3, 3): 3}


def needle(kind):
    """kind 'clean': random columns with c1, c2 random bits, c3 = c1 c2, c5 = c4^2, c7 = c0 c6, and columns 8..39 zero before row 100 (j - 8).
    'first' / 'last': c7 is off by one on row 0 / row n - 1 only."""
    rng = np.random.RandomState(13)
    n, w = NEEDLE_N, NEEDLE_W
    t = rng.randint(1, P, size=(n, w)).astype(np.uint64)
    t[:, 1], t[:, 2] = rng.randint(0, 2, size=n), rng.randint(0, 2, size=n)
    t[:, 3] = t[:, 1] * t[:, 2]
    t[:, 5] = t[:, 4] * t[:, 4] % P
    t[:, 7] = t[:, 0] * t[:, 6] % P
    for j in range(8, w):
        t[:100 * (j - 8), j] = 0
    if kind != "clean":
        row = 0 if kind == "first" else n - 1
        t[row, 7] = (t[row, 7] + 1) % P
    return t.astype(np.uint32)


NEEDLE_BROKEN = [(1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3), (4, 4)]
NEEDLE_RELATIONS = {"first": NEEDLE_BROKEN, "last": NEEDLE_BROKEN, "clean": sorted(NEEDLE_BROKEN + [(0, 6)])}
