"""The operand corpus of the field-edge tests (tests/test_field_edges_cpu.py, test_field_edges_gpu.py, test_edge_values_gpu.py): STORED WORDS
at the extremes of each primitive's domain, the same seeded corpus for the CPU (hipemu) and the device runs.

  E   stored words every reduced operand may take: 0, 1, 2, p-2, p-1, (p-1)/2, (p+1)/2, R mod p, R^2 mod p, p - (R mod p), 2^27-1, 2^27, 2^30,
      0x77FFFFFF (7-bit digits 127, 127, 127, 63, 7 — the digit planes of the matrix-core column dots; not 127 four times: that needs a top
      digit of at most 6, and 0x6FFFFFFF = 127, 127, 127, 127, 6 joins the COLUMNS of the opening tests, tests/edge_stage_cases.py)
  E2  the lazy range [p, 2p) of the butterfly network's unreduced values: p, p+1, 2^31-1, 2^31, 2p-2, 2p-1

corpus(op) is what is sent to the device for `op` (a key of valida_amd.FIELD_PROBE_OPS), boundary_vectors(op) the NAMED vectors DESIGN.md's
"Arithmetic bounds" table points at; the tests assert that every one of them is a row of corpus(op).  Every row lies in the domain the op's call
sites use (tests/field_ref.py asserts it on every row): nothing is ever skipped.
"""
import functools
import itertools

import numpy as np

P = 2 ** 31 - 2 ** 27 + 1
R = 2 ** 32
R_INV = pow(R, -1, P)
E = [0, 1, 2, P - 2, P - 1, (P - 1) // 2, (P + 1) // 2, R % P, R * R % P, P - R % P, 2 ** 27 - 1, 2 ** 27, 2 ** 30, 0x77FFFFFF]
E2 = [P, P + 1, 2 ** 31 - 1, 2 ** 31, 2 * P - 2, 2 * P - 1]
WIDE_HI = [P - 1, P, 0xE1000000]                       # high words of monty_reduce_wide: around its conditional subtraction, and that of 4 (p-1)^2
WIDE_LO = [0, 1, R - 1, R - P]                         # low words: m = 0 (low word 0), m = 2^32 - 1 (low word -p mod 2^32)
BFLY_LOW = [(1, 1), (3, 5), (4, 0), (4, 15), (8, 0), (8, 77), (8, 255), (10, 1023)]  # (lowbits, low) of the rounds above stage 1: ntt.hip's 4 / 8, the tails
N_RANDOM = 1 << 16

assert all(0 <= w < P for w in E) and all(P <= w < 2 * P for w in E2) and 2 * P - 1 == 0xF0000001
assert [0x77FFFFFF >> 7 * i & 127 for i in range(5)] == [127, 127, 127, 63, 7] and [0x6FFFFFFF >> 7 * i & 127 for i in range(5)] == [127, 127, 127, 127, 6]
assert 4 * (P - 1) ** 2 >> 32 == 0xE1000000 and (2 * P - 1) * (P - 1) >> 32 == 0x70800000 < P


def from_words(words):
    """The canonical values whose stored form is `words`: word R^-1 mod p (what to upload so that the device holds exactly these words)."""
    w = np.asarray(words, dtype=np.uint64)
    assert (w < P).all()
    return (w * np.uint64(R_INV) % np.uint64(P)).astype(np.uint32)


def _rng(op):
    return np.random.default_rng([0xED6E, sum(ord(c) << 8 * (i % 4) for i, c in enumerate(op))])


def _draw(rng, shape, pool, p_pool=1.0, high=P):
    """Each word from `pool` with probability p_pool, else uniform below `high`."""
    pool = np.asarray(pool, dtype=np.uint64)
    pick = pool[rng.integers(0, len(pool), size=shape)]
    uni = rng.integers(0, high, size=shape, dtype=np.uint64)
    return np.where(rng.random(size=shape) < p_pool, pick, uni)


def _rows(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint64).reshape(len(p), -1) for p in parts if len(p)]).astype(np.uint32)


def _split(ts):
    return [(t & (R - 1), t >> 32) for t in ts]


def _binary(op):
    rng = _rng(op)
    return _rows(list(itertools.product(E, E)), rng.integers(0, P, (N_RANDOM, 2)), _draw(rng, (N_RANDOM, 2), E, 0.5))


def _lazy_pairs(rng):  # a < 2p, b < p
    a = np.concatenate([rng.integers(0, 2 * P, N_RANDOM, dtype=np.uint64), _draw(rng, N_RANDOM, E + E2, 0.5, 2 * P)])
    b = np.concatenate([rng.integers(0, P, N_RANDOM, dtype=np.uint64), _draw(rng, N_RANDOM, E, 0.5)])
    return list(itertools.product(E + E2, E)) + list(zip(a.tolist(), b.tolist()))


def _wide_edge_products():
    return sorted({a * b for a in E for b in E})


def _signed_pool():  # the representatives in [-p, p) the S-box hands its products
    return sorted({e for e in E} | {e - P for e in E})


def _ext_operands(rng, n_limbs_extra=0):
    """Ext5 operands: every limb one word of E, one-hot, 2^14 draws from E, 2^12 uniform."""
    same = [[w] * 5 for w in E]
    hot = [[w if i == k else 0 for i in range(5)] for k in range(5) for w in E if w]
    return same, hot, _draw(rng, (1 << 14, 5 + n_limbs_extra), E).tolist(), rng.integers(0, P, (1 << 12, 5 + n_limbs_extra)).tolist()


def _butterfly_points(rng):
    pts = [[w] * 16 for w in E]
    pts += [[0, P - 1] * 8, [P - 1, 0] * 8]
    pts += [[w if g == k else 0 for g in range(16)] for k in range(16) for w in E if w]
    return pts, _draw(rng, (1 << 12, 16), E).tolist() + rng.integers(0, P, (1 << 12, 16)).tolist()


@functools.lru_cache(maxsize=None)
def corpus(op):
    """(n_items, operand words) uint32: what the tests send to the device for `op`."""
    rng = _rng(op)
    if op == "reduce_once":
        return _rows(E + E2, rng.integers(0, 2 * P, N_RANDOM), _draw(rng, N_RANDOM, E + E2, 0.5, 2 * P))
    if op in ("sub_mod", "add", "sub"):
        return _binary(op)
    if op == "mul":  # both reduced, and one operand lazy (the butterflies' case) in either argument order
        lazy = _lazy_pairs(rng)
        return _rows(_binary(op), lazy, [(b, a) for a, b in lazy])
    if op in ("neg", "canonical", "sbox"):
        return _rows(E, rng.integers(0, P, N_RANDOM), _draw(rng, N_RANDOM, E, 0.5))
    if op == "inv":
        return _rows([w for w in E if w], rng.integers(1, P, 1 << 12))
    if op == "from_canonical":  # any u32
        return _rows(E + E2 + [2 * P, 2 * P + 1, R - 2, R - 1], rng.integers(0, R, N_RANDOM), _draw(rng, N_RANDOM, E + E2, 0.5, R))
    if op == "monty_reduce":  # t = a b, a < 2p, b < p, built from operand pairs
        return _rows(_split([a * b for a, b in itertools.product(E, E)]), _split([a * b for a, b in _lazy_pairs(rng)]))
    if op == "monty_reduce_wide":  # every sum of four products of words of E; high x low word edges below 4 p^2; random sums of four products
        pr = np.array(_wide_edge_products(), dtype=np.uint64)  # 4 (p-1)^2 < 2^64: the sums fit
        k, l = np.triu_indices(len(pr))                        # pairs k <= l, sorted by k
        pair, first = pr[k] + pr[l], np.searchsorted(k, np.arange(len(pr)))
        sums = np.concatenate([pr[i] + pr[j] + pair[first[j]:] for i in range(len(pr)) for j in range(i, len(pr))])  # i <= j <= k <= l
        cross = [hi << 32 | lo for hi in WIDE_HI for lo in WIDE_LO if (hi << 32 | lo) < 4 * P * P]
        ab = rng.integers(0, P, (N_RANDOM, 8)).tolist()
        rand = [r[0] * r[1] + r[2] * r[3] + r[4] * r[5] + r[6] * r[7] for r in ab]
        t = np.concatenate([sums, np.array(cross + rand, dtype=np.uint64)])
        return np.stack([t & np.uint64(R - 1), t >> np.uint64(32)], axis=1).astype(np.uint32)
    if op == "ext_mul":
        same, hot, drawn, uni = _ext_operands(rng, 5)
        return _rows([a + b for a in same for b in same], [a + b for a in hot for b in hot], drawn, uni)
    if op in ("ext_square", "ext_inv"):
        same, hot, drawn, uni = _ext_operands(rng)
        return _rows(same, hot, drawn, uni if op == "ext_square" else uni[:1 << 9])  # the inverse's reference is a 5 x 5 elimination per item
    if op == "ext_scale":
        same, hot, drawn, uni = _ext_operands(rng, 1)
        return _rows([a + [s] for a in same for s in E], [a + [s] for a in hot for s in E], drawn, uni)
    if op in ("bfly_dit_lb0", "bfly_dif_lb0"):
        pts, rand = _butterfly_points(rng)
        return _rows([x + [0, 0] for x in pts + rand])
    if op in ("bfly_dit", "bfly_dif"):
        pts, rand = _butterfly_points(rng)
        pick = rng.integers(0, len(BFLY_LOW), len(rand))
        free = [[int(lb), int(rng.integers(0, 1 << lb))] for lb in rng.integers(1, 11, len(rand))]
        return _rows([x + [low, lb] for x in pts for lb, low in BFLY_LOW], [x + [BFLY_LOW[k][1], BFLY_LOW[k][0]] for x, k in zip(rand, pick)],
                     [x + [low, lb] for x, (lb, low) in zip(rand, free)])
    if op == "monty_signed":  # t = x y, x and y in [-p, p): what the S-box multiplies
        pool = _signed_pool()
        xy = (rng.integers(-P, P, (N_RANDOM, 2))).tolist()
        return _rows(_split([(x * y) % 2 ** 64 for x, y in itertools.product(pool, pool)]), _split([(x * y) % 2 ** 64 for x, y in xy]))
    if op == "sbox_plus":
        return _binary(op)
    if op in ("permute", "permute_plain"):
        return _rows([[w] * 16 for w in E], _draw(rng, (64, 16), E), rng.integers(0, P, (64, 16)))
    raise KeyError(op)


def boundary_vectors(op):
    """The named boundary vectors of `op` (rows of corpus(op), asserted by the tests): the operands that reach the bounds of DESIGN.md's
    "Arithmetic bounds" table."""
    pm1 = P - 1
    if op == "reduce_once":
        return [(w,) for w in (0, pm1, P, P + 1, 2 * P - 2, 2 * P - 1)]
    if op in ("sub_mod", "add", "sub", "sbox_plus"):
        return list(itertools.product(E, E))
    if op == "mul":
        return list(itertools.product(E, E)) + [(a, b) for a in E2 for b in E] + [(b, a) for a in E2 for b in E]
    if op in ("neg", "canonical", "sbox"):
        return [(w,) for w in E]
    if op == "inv":
        return [(w,) for w in E if w]
    if op == "from_canonical":
        return [(w,) for w in (0, pm1, P, 2 * P - 1, 2 * P, R - 1)]
    if op == "monty_reduce":  # the largest product of the lazy butterflies, the largest reduced one, m = 0 (low word 0), the canonical() operand p - 1
        return _split([(2 * P - 1) * pm1, pm1 * pm1, 0, 2 ** 60, pm1, (2 * P - 1) * 1])
    if op == "monty_reduce_wide":  # 4 (p-1)^2: the largest high word; the words around the conditional subtraction; m = 0 and m = 2^32 - 1
        return _split([4 * pm1 * pm1, 0, pm1 * pm1] + [hi << 32 | lo for hi in WIDE_HI for lo in WIDE_LO if (hi << 32 | lo) < 4 * P * P])
    if op == "ext_mul":  # every limb p - 1 on both sides: limb 4 sums four products (p-1)^2
        hot = [0, 0, 0, 0, pm1]
        return [tuple([a] * 5 + [b] * 5) for a in E for b in E] + [tuple(hot + hot), tuple(hot[::-1] + hot), tuple(hot + hot[::-1])]
    if op in ("ext_square", "ext_inv"):
        return [tuple([w] * 5) for w in E]
    if op == "ext_scale":
        return [tuple([a] * 5 + [s]) for a in E for s in E]
    if op in ("bfly_dit_lb0", "bfly_dif_lb0"):  # all p - 1 / 0 against p - 1: the lazy sums 2p - 2 and the unreduced differences 2p - 1
        return [tuple([w] * 16 + [0, 0]) for w in E] + [tuple([0, pm1] * 8 + [0, 0]), tuple([pm1, 0] * 8 + [0, 0])] + [
            tuple([pm1 if g == k else 0 for g in range(16)] + [0, 0]) for k in range(16)]
    if op in ("bfly_dit", "bfly_dif"):
        return [tuple(x + [low, lb]) for lb, low in BFLY_LOW for x in [[w] * 16 for w in E] + [[0, pm1] * 8, [pm1, 0] * 8]]
    if op == "monty_signed":  # (-p)^2 (x = 0, c = 0 in poseidon_sbox_plus), the most negative product, (p-1)^2, 0
        return _split([P * P, (-P * pm1) % 2 ** 64, pm1 * pm1, 0, (-1) % 2 ** 64])
    if op in ("permute", "permute_plain"):
        return [tuple([w] * 16) for w in E]
    raise KeyError(op)


def missing_rows(operands, vectors):
    """The `vectors` that are NOT rows of `operands` (compared as whole rows)."""
    a = np.ascontiguousarray(operands, dtype=np.uint32)
    v = np.ascontiguousarray(np.asarray(vectors, dtype=np.uint64).astype(np.uint32).reshape(len(vectors), -1))
    assert v.shape[1] == a.shape[1]
    key = np.dtype((np.void, 4 * a.shape[1]))
    found = np.isin(v.view(key).ravel(), a.view(key).ravel())
    return [tuple(int(x) for x in row) for row, f in zip(v, found) if not f]


def first_mismatch_item(op, operands, got, want):
    """None, or a description of the first item whose result words differ from the reference's, with its operands."""
    bad = np.nonzero((np.asarray(got) != np.asarray(want)).any(axis=1))[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    return "%s: %d of %d items differ; first at item %d: operands %s -> %s, reference %s" % (
        op, bad.size, len(got), i, [hex(int(v)) for v in operands[i]], [hex(int(v)) for v in got[i]], [hex(int(v)) for v in want[i]])


# ---- matrices for the stage tests (canonical values, i.e. what the ABI takes; the device then holds the chosen words) -----------------------
STAGE_WORDS = [0, 1, P - 1, 0x77FFFFFF]


def constant_matrix(word, h, w):
    return np.full((h, w), from_words([word])[0], dtype=np.uint32)


def alternating_matrix(h, w):
    m = np.zeros((h, w), dtype=np.uint32)
    m[1::2] = from_words([P - 1])[0]
    return m


def impulse_matrix(h, w, row):
    m = np.zeros((h, w), dtype=np.uint32)
    m[row] = from_words([P - 1])[0]
    return m


def edge_mix_matrix(seed, h, w):
    rng = np.random.default_rng([0xED6E, seed])
    return from_words(np.asarray(E, dtype=np.uint64)[rng.integers(0, len(E), (h, w))])


def edge_words(seed, n):
    rng = np.random.default_rng([0xED6F, seed])
    return np.asarray(E, dtype=np.uint64)[rng.integers(0, len(E), n)]


def stage_matrices(h, w, seed=0):
    """name -> canonical (h, w) matrix: the corpus matrices of the stage tests."""
    out = {"const_%08x" % word: constant_matrix(word, h, w) for word in STAGE_WORDS + [0x6FFFFFFF]}
    out["alternating"] = alternating_matrix(h, w)
    out["impulse_first"] = impulse_matrix(h, w, 0)
    out["impulse_last"] = impulse_matrix(h, w, h - 1)
    out["edge_mix"] = edge_mix_matrix(seed + 131 * h + w, h, w)
    return out
