"""Corpus and plain-integer reference of the lazy-sum probe (valida_amd/csrc/kernels/lazy_probe.hip; valida_amd.LAZY_PROBE_OPS).  Everything here is
RAW STORED WORDS: a sum of products of stored words, divided by R = 2^32 mod p, is the stored word of the sum of the products of the values.

Per (op, length): 2^16 seeded tuples, then the named boundary vectors (boundary_vectors; the tests assert they are in the corpus):
  * every word p - 1: each fold sees its largest input, the final reduction a high word of 1.9375 p - eps;
  * fold_hi: high words {p - 1, p, p + 1, 2p - 1} x low words {0, 1, 2^32 - 1, 2^32 - p};
  * one-hot operands (one limb of one term p - 1, the rest 0);
  * terms alternating between all 0 and all p - 1, in both phases: a fold is taken and not taken in turn.
"""
import zlib

import numpy as np

import field_ref as fr

P = fr.P
R = fr.R
R_INV = pow(R, -1, P)
N_SEEDED = 1 << 16
LIN_LENGTHS = list(range(1, 18)) + [34]
EXT_LENGTHS = list(range(1, 9))
LOOP_LENGTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 17, 23, 34, 64]  # the rolled form: fewer tuples (N_LOOP), every parity and the 4 / 2 / 2 schedule's first turns
N_LOOP = 1 << 12
CASES = [("fold_hi", 0), ("ext_mul", 0)] + [("lin_dot", n) for n in LIN_LENGTHS] + [("ext_dot", n) for n in EXT_LENGTHS] + [("lin_dot_loop", n) for n in LOOP_LENGTHS]
FOLD_HI_HIGH = [P - 1, P, P + 1, 2 * P - 1]
FOLD_HI_LOW = [0, 1, 2 ** 32 - 1, 2 ** 32 - P]


def case_id(case):
    return "%s-%d" % case if case[1] else case[0]


def words_per_term(op):
    return {"lin_dot": 6, "lin_dot_loop": 6, "ext_dot": 10}[op]


def in_words(op, n):
    return {"fold_hi": 2, "ext_mul": 10}.get(op) or words_per_term(op) * n


def boundary_vectors(op, n):
    pm1 = P - 1
    if op == "fold_hi":
        return [(lo, hi) for hi in FOLD_HI_HIGH for lo in FOLD_HI_LOW]
    if op == "ext_mul":
        v = [(pm1,) * 10, (0,) * 10]
        for i in range(5):
            for j in range(5):
                r = [0] * 10
                r[i], r[5 + j] = pm1, pm1
                v.append(tuple(r))
        v.append((pm1, 0, pm1, 0, pm1, 0, pm1, 0, pm1, 0))
        v.append((0, pm1, 0, pm1, 0, pm1, 0, pm1, 0, pm1))
        return v
    w = words_per_term(op)
    v = [(pm1,) * (w * n), (0,) * (w * n)]
    for phase in (0, 1):  # alternating terms
        v.append(tuple(x for c in range(n) for x in ((pm1,) * w if c % 2 == phase else (0,) * w)))
    for c in sorted({0, n // 2, n - 1}):  # one-hot: one limb of term c against one word of its partner
        for k in range(5):
            for k2 in range(w - 5):
                r = [0] * (w * n)
                r[w * c + k], r[w * c + 5 + k2] = pm1, pm1
                v.append(tuple(r))
    return v


def corpus(op, n):
    """(items, in_words(op, n)) uint32: the seeded tuples, then the boundary vectors."""
    rng = np.random.default_rng(zlib.crc32(("%s/%d" % (op, n)).encode()))
    count = N_LOOP if op == "lin_dot_loop" else N_SEEDED
    iw = in_words(op, n)
    if op == "fold_hi":
        seeded = np.stack([rng.integers(0, 2 ** 32, count, dtype=np.uint64), rng.integers(0, 2 * P, count, dtype=np.uint64)], axis=1)
    else:
        seeded = rng.integers(0, P, (count, iw), dtype=np.uint64)
        # a third of the tuples draw from the extreme words, so that runs of p - 1 and 0 occur in the seeded part as well
        pool = np.array([0, 1, P - 1, P - 2, (P - 1) // 2, R % P], dtype=np.uint64)
        third = count // 3
        seeded[:third] = pool[rng.integers(0, len(pool), (third, iw))]
    return np.concatenate([seeded, np.array(boundary_vectors(op, n), dtype=np.uint64)]).astype(np.uint32)


def missing_rows(operands, vectors):
    have = {r.tobytes() for r in np.ascontiguousarray(operands, dtype=np.uint32)}
    return [v for v in vectors if np.array(v, dtype=np.uint32).tobytes() not in have]


def _ext_mul_words(a, b):
    """(items, 5) x (items, 5) stored words -> stored words of the products; uint64 throughout (a product of two words < 2^62, a residue < 2^31)."""
    p = np.uint64(P)
    out = np.zeros(a.shape, dtype=np.uint64)
    for k in range(5):
        s = np.zeros(a.shape[0], dtype=np.uint64)
        for i in range(5):
            t = a[:, i] * b[:, (k - i) % 5] % p
            s += t if i <= k else 2 * t  # X^5 = 2
        out[:, k] = s % p * np.uint64(R_INV) % p
    return out


def reference(op, n, operands):
    """Stored words the probe must return, from integer arithmetic mod p alone.  Asserts every operand's domain."""
    x = np.asarray(operands, dtype=np.uint64)
    p = np.uint64(P)
    if op == "fold_hi":
        lo, hi = x[:, 0], x[:, 1]
        assert (hi < 2 * P).all()
        return np.stack([lo, np.where(hi >= p, hi - p, hi)], axis=1).astype(np.uint32)
    assert (x < P).all()
    if op == "ext_mul":
        return _ext_mul_words(x[:, :5], x[:, 5:]).astype(np.uint32)
    w = words_per_term(op)
    acc = np.zeros((x.shape[0], 5), dtype=np.uint64)
    for c in range(n):
        t = x[:, w * c:w * (c + 1)]
        if w == 6:
            acc += t[:, :5] * t[:, 5:6] % p * np.uint64(R_INV) % p
        else:
            acc += _ext_mul_words(t[:, :5], t[:, 5:])
    return (acc % p).astype(np.uint32)


def reference_bigint(op, n, row):
    """One item with Python integers and tests/field_ref.py's own product: what `reference` is checked against."""
    row = [int(v) for v in row]
    if op == "fold_hi":
        return [row[0], row[1] - P if row[1] >= P else row[1]]
    if op == "ext_mul":
        return fr.ext_mul(row[:5], row[5:])
    w = words_per_term(op)
    out = [0] * 5
    for c in range(n):
        t = row[w * c:w * (c + 1)]
        term = [a * t[5] * R_INV % P for a in t[:5]] if w == 6 else fr.ext_mul(t[:5], t[5:])
        out = [(o + v) % P for o, v in zip(out, term)]
    return out
