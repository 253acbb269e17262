"""Inputs the transition audit's CPU and GPU tests share: the captured one-chip "step" machine (one constraint, when_transition(next.c0 - c0 -
1)) with its analytic trace and the closed-form Jacobian the reference is given for it, a captured machine without constraints, and the
"needle" traces (4096 x 8).  Trace heights are powers of two (every audit's and the prover's rule), so the gated cases run at 256 rows and
more: at least min_gate_windows = 64 windows per gate, and more windows per gate than window columns."""
import ctypes

import numpy as np

import valida_amd as va

P = va.P
NEEDLE_N, NEEDLE_W = 4096, 8
NEEDLE_F = 1 + NEEDLE_W + 5  # the window column of next.c5


def _machine(name, width, step):
    L, u = va.lib(), ctypes.c_uint32
    m, air = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.vgpu_machine_new(ctypes.byref(m)) == 0
    assert L.vgpu_air_new(name, u(width), u(0), ctypes.byref(air)) == 0
    if step:
        loc, nxt = L.vgpu_air_variable(air, u(0), u(0), u(0)), L.vgpu_air_variable(air, u(0), u(0), u(1))
        d = L.vgpu_air_sub(air, u(L.vgpu_air_sub(air, u(nxt), u(loc))), u(L.vgpu_air_constant(air, u(1))))
        L.vgpu_air_assert_zero(air, u(L.vgpu_air_mul(air, u(L.vgpu_air_is_transition(air)), u(d))))
    assert L.vgpu_machine_push_air(m, air) == 0, L.vgpu_last_error()
    L.vgpu_air_free(air)
    return va.Machine(m)


def step_machine(width):
    """One captured AIR of `width` >= 4 columns with the one constraint when_transition(next.c0 - c0 - 1)."""
    return _machine(b"step", width, True)


def free_machine(width):
    """One captured AIR of `width` columns that constrains nothing."""
    return _machine(b"free", width, False)


def step_height(width):
    """The smallest power of two at which every gate of step_trace has at least 64 windows and more windows than window columns."""
    return 256 if width <= 32 else (512 if width <= 64 else 1024)


def step_trace(n, width):
    """c0 = r; c1 = 1 on every third row, else 0; c2 = c0 + 4 where c1 = 1, else r^2; c3: next.c3 = c3 + c0 where next.c1 = 0, else (r + 1)^3;
    the other columns random (seeded): independent of everything once there are more windows than window columns."""
    r = np.arange(n, dtype=np.uint64)
    c1 = (r % 3 == 0).astype(np.uint64)
    c2 = np.where(c1 == 1, (r + 4) % P, r * r % P)
    c3 = np.zeros(n, dtype=np.uint64)
    c3[0] = 5
    for k in range(1, n):
        c3[k] = (c3[k - 1] + r[k - 1]) % P if c1[k] == 0 else pow(k, 3, P)
    t = np.random.RandomState(width).randint(2, P, size=(n, width)).astype(np.uint64)
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = r, c1, c2, c3
    return t.astype(np.uint32)


def step_jacobians(width):
    """The reference's `jacobians` for step_machine at n >= 2: one constraint, no interaction.  The cell c0 of row r is `local` of the evaluation
    at r (derivative -is_transition(r)) and `next` of the evaluation at r - 1 (derivative is_transition(r - 1), r - 1 taken mod n): on every row
    at least one of the two is non-zero, so the row space of J_r is that of e_0."""
    J = np.zeros((1, width), dtype=np.uint64)
    J[0, 0] = 1
    return {0: (1, 0, lambda r: J)}


def free_jacobians(width):
    return {0: (0, 0, lambda r: np.zeros((0, width), dtype=np.uint64))}


def needle(kind):
    """4096 x 8: c0, c2, c3, c7 random; c1 = r mod 2; c4 = 1 on the rows below 63 and c6 = 1 on the rows below 64, else 0 (as `local` columns:
    gates of exactly 63 and of exactly 64 windows); c5: next.c5 = c3 + next.c2 + 7 on every window BUT, by kind, window 0 ('first'), window
    n - 2 ('last') or window 95 ('straddle': its `next` row is the first row of the following elimination slice and enforcement workgroup; no
    combination of the other columns singles that window out).  kind 'none': no window breaks it, and c1 is 2 on row n - 1: boolean as
    `local`, not as `next`."""
    n, w = NEEDLE_N, NEEDLE_W
    t = np.random.RandomState(23).randint(2, P, size=(n, w)).astype(np.uint64)
    r = np.arange(n)
    t[:, 1] = r % 2
    t[:, 4] = r < 63
    t[:, 6] = r < 64
    t[1:, 5] = (t[:-1, 3] + t[1:, 2] + 7) % P
    window = {"first": 0, "last": n - 2, "straddle": 95, "none": None}[kind]
    if window is None:
        t[n - 1, 1] = 2
    else:  # c5 of a row occurs in the relation of one window only, the one it is `next` of
        t[window + 1, 5] = (t[window + 1, 5] + 1) % P
    return t.astype(np.uint32)


NEEDLE_TERMS = [(1 + 3, P - 1), (1 + NEEDLE_W + 2, P - 1), (NEEDLE_F, 1)]  # next.c5 - c3 - next.c2 (- 7 = l0)
