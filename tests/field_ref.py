"""Plain-integer reference of the device's field arithmetic ON STORED WORDS (tests/test_field_edges_*.py): BabyBear, p = 2^31 - 2^27 + 1, elements
stored as x R mod p with R = 2^32, the extension F_p[X] / (X^5 - 2).  Python integers, `%` and pow(., -1, P) only: nothing here comes from
valida_amd/csrc/field.hpp or from the oracle, so an error shared with either cannot hide.  Every function checks that its operands lie in the
domain the device function documents — an operand outside it is an error of the corpus (tests/edge_corpus.py), never something to skip.
"""
import numpy as np

P = 2 ** 31 - 2 ** 27 + 1
R = 2 ** 32
R_INV = pow(R, -1, P)
P_INV = pow(P, -1, R)           # p^-1 mod 2^32
G27 = pow(31, (P - 1) >> 27, P)  # a generator of the 2^27-th roots of unity (31 generates the multiplicative group)


def to_words(x):
    return x * R % P


def from_words(w):
    return w * R_INV % P


# ---- base field -----------------------------------------------------------------------------------------------------------------------------
def reduce_once(s):
    assert 0 <= s < 2 * P, s
    return s % P


def sub_mod(a, b):
    assert 0 <= a < P and 0 <= b < P, (a, b)
    return (a - b) % P


def add(a, b):
    assert 0 <= a < P and 0 <= b < P, (a, b)
    return (a + b) % P


def neg(a):
    assert 0 <= a < P, a
    return -a % P


def monty_reduce(t):
    assert 0 <= t < P * R, t
    return t * R_INV % P


def monty_reduce_wide(t):
    assert 0 <= t < 4 * P * P, t
    return t * R_INV % P


def mul(a, b):
    """Stored word of the product; one operand may be lazy (below 2p): the product only has to stay below p 2^32."""
    assert 0 <= a < 2 * P and 0 <= b < 2 * P and min(a, b) < P, (a, b)
    return monty_reduce(a * b)


def from_canonical(x):
    assert 0 <= x < R, x
    return x % P * R % P


def canonical(w):
    assert 0 <= w < P, w
    return w * R_INV % P


def inv(w):
    """Stored word of 1 / x for x = w / R: R^2 / w.  0 -> 0 (the device's x^(p - 2))."""
    assert 0 <= w < P, w
    return pow(w, -1, P) * R * R % P if w else 0


# ---- F_p[X] / (X^5 - 2) ---------------------------------------------------------------------------------------------------------------------
def _ext_mul_plain(a, b):  # on VALUES (no Montgomery factor)
    c = [0] * 5
    for i in range(5):
        for j in range(5):
            if i + j < 5:
                c[i + j] += a[i] * b[j]
            else:
                c[i + j - 5] += 2 * a[i] * b[j]
    return [v % P for v in c]


def ext_mul(a, b):
    assert all(0 <= v < P for v in a) and all(0 <= v < P for v in b), (a, b)
    return [v * R_INV % P for v in _ext_mul_plain(a, b)]


def ext_square(a):
    return ext_mul(a, a)


def ext_scale(a, s):
    assert all(0 <= v < P for v in a) and 0 <= s < P
    return [v * s * R_INV % P for v in a]


def ext_inv_plain(a):
    """1 / a on values, by Gaussian elimination on the matrix of `multiply by a` (column j = a X^j); 0 -> 0."""
    if not any(a):
        return [0] * 5
    cols = []
    for j in range(5):
        e = [0] * 5
        e[j] = 1
        cols.append(_ext_mul_plain(a, e))
    m = [[cols[j][i] for j in range(5)] + [1 if i == 0 else 0] for i in range(5)]  # M x = e_0
    for c in range(5):
        piv = next(r for r in range(c, 5) if m[r][c])
        m[c], m[piv] = m[piv], m[c]
        s = pow(m[c][c], -1, P)
        m[c] = [v * s % P for v in m[c]]
        for r in range(5):
            if r != c and m[r][c]:
                f = m[r][c]
                m[r] = [(x - f * y) % P for x, y in zip(m[r], m[c])]
    return [m[i][5] for i in range(5)]


def ext_inv(a):
    assert all(0 <= v < P for v in a), a
    return [to_words(v) for v in ext_inv_plain([from_words(v) for v in a])]


# ---- the radix-2 stages of one radix-16 round (kernels/butterfly.hpp, header comment) -------------------------------------------------------
def butterflies16(x, low, lowbits, dit):
    """Stage s = lowbits + 1 + st pairs the points whose indices differ in bit st, with the twiddle w_{2^s}^(low + (k << lowbits)), k = the index's
    bits below st.  DIT (stages upwards, forward roots): (u, v) -> (u + v w, u - v w); DIF (stages downwards, inverse roots — the tables the NTT
    kernels hand each form): (u, v) -> (u + v, (u - v) w).  Every output is a reduced stored word."""
    assert len(x) == 16 and all(0 <= v < P for v in x) and 0 <= lowbits <= 10 and 0 <= low < (1 << lowbits), (x, low, lowbits)
    x = list(x)
    for step in range(4):
        st = step if dit else 3 - step
        w = pow(G27, 1 << (27 - (lowbits + 1 + st)), P)
        if not dit:
            w = pow(w, -1, P)
        for g0 in range(16):
            if g0 >> st & 1:
                continue
            g1 = g0 | 1 << st
            tw = to_words(pow(w, low + ((g0 & ((1 << st) - 1)) << lowbits), P))
            u, v = x[g0], x[g1]
            if dit:
                t = mul(v, tw)
                x[g0], x[g1] = (u + t) % P, (u - t) % P
            else:
                x[g0], x[g1] = (u + v) % P, mul((u - v) % P, tw)
    assert all(0 <= v < P for v in x)
    return x


# ---- the signed products of the Poseidon S-box (kernels/poseidon_perm.hpp) ------------------------------------------------------------------
def monty_signed(t):
    """(t - m p) / 2^32 with m = t p^-1 taken in [-2^31, 2^31): exact, congruent to t / R, and inside (-p, p) for |t| < p 2^31."""
    assert -P * 2 ** 31 < t < P * 2 ** 31, t
    m = t * P_INV % R
    if m >= 2 ** 31:
        m -= R
    assert (t - m * P) % R == 0
    r = (t - m * P) // R
    assert -P < r < P and (r * R - t) % P == 0
    return r


def sbox(x):
    assert 0 <= x < P, x
    return pow(x, 5, P) * pow(R_INV, 4, P) % P


def sbox_plus(x, c):
    assert 0 <= x < P and 0 <= c < P, (x, c)
    return pow(x + c, 5, P) * pow(R_INV, 4, P) % P


# ---- one op of the probe on a whole corpus --------------------------------------------------------------------------------------------------
def _u64(row):
    return row[0] | row[1] << 32


def _s64(row):
    t = _u64(row)
    return t - 2 ** 64 if t >= 2 ** 63 else t


def apply(op, operands, permute=None):
    """The reference's result words for every row of `operands` (an (n, words) array of stored words): (n, result words) uint32.
    permute: canonical 16-word state -> canonical state (the two permutation ops, which are checked against the library's host permutation)."""
    if op == "monty_reduce_wide":  # millions of rows: the same two `%` on 64-bit integers, a column at a time (checked against the scalar form by the CPU test)
        a = np.asarray(operands, dtype=np.uint64)
        t = a[:, 0] | a[:, 1] << np.uint64(32)
        assert (t < np.uint64(4 * P * P)).all()
        return (t % np.uint64(P) * np.uint64(R_INV) % np.uint64(P)).astype(np.uint32).reshape(-1, 1)
    rows = np.asarray(operands, dtype=np.uint64).tolist()
    one = {
        "reduce_once": lambda r: [reduce_once(r[0])], "sub_mod": lambda r: [sub_mod(r[0], r[1])], "add": lambda r: [add(r[0], r[1])],
        "sub": lambda r: [sub_mod(r[0], r[1])], "neg": lambda r: [neg(r[0])], "mul": lambda r: [mul(r[0], r[1])],
        "monty_reduce": lambda r: [monty_reduce(_u64(r))], "monty_reduce_wide": lambda r: [monty_reduce_wide(_u64(r))],
        "from_canonical": lambda r: [from_canonical(r[0])], "canonical": lambda r: [canonical(r[0])], "inv": lambda r: [inv(r[0])],
        "ext_mul": lambda r: ext_mul(r[:5], r[5:]), "ext_square": lambda r: ext_square(r), "ext_scale": lambda r: ext_scale(r[:5], r[5]),
        "ext_inv": lambda r: ext_inv(r),
        "bfly_dit_lb0": lambda r: butterflies16(r[:16], r[16], r[17], True), "bfly_dit": lambda r: butterflies16(r[:16], r[16], r[17], True),
        "bfly_dif_lb0": lambda r: butterflies16(r[:16], r[16], r[17], False), "bfly_dif": lambda r: butterflies16(r[:16], r[16], r[17], False),
        "monty_signed": lambda r: [monty_signed(_s64(r)) % R], "sbox": lambda r: [sbox(r[0])], "sbox_plus": lambda r: [sbox_plus(r[0], r[1])],
    }
    if op in ("permute", "permute_plain"):
        assert all(0 <= v < P for r in rows for v in r)
        return np.array([[to_words(int(v)) for v in permute([from_words(v) for v in r])] for r in rows], dtype=np.uint32)
    if op.endswith("_lb0"):
        assert all(r[16] == 0 and r[17] == 0 for r in rows)
    return np.array([one[op](r) for r in rows], dtype=np.uint32)
