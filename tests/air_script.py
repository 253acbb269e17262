"""Scripted AIRs: one description of an AIR, three consumers (tests/test_air_programs_cpu.py, test_air_programs_gpu.py).

A script is a small expression tree of Python tuples (the constructors below).  From the one tree:
  to_oracle_words  the postfix word list the oracle's scripted chip walks (oracle/chips.hpp: evaluated directly on every builder, no
                   simplification, no sharing: a subtree used twice is written out twice);
  to_ffi           the same AIR captured through vgpu_air_* -- hash-consed, folded, lowered to a register program.  A Python object used twice is
                   handed over ONCE (the same handle), equal trees built separately are handed over separately;
  eval_py          plain integer arithmetic mod p;
  degree_py        the reference's degree rules (symbolic_expression.rs:36-62), no folding;
  satisfiable      the script with one result column per constraint (col_j - expr_j = 0) and the trace filler that makes any DAG hold.
CORPUS holds the named scripts (the register-file boundaries of the device interpreters, padding, every opcode, every fold of the capture,
the assert forms, the load forms, the selectors, the degrees, the constraint counts), generated(seed) the seeded random DAGs.
"""
import ctypes
from collections import namedtuple

import numpy as np

from edge_corpus import E, P

Script = namedtuple("Script", "name width prep_width constraints")


def const(v): return ("const", int(v))
def main(col, nxt=0): return ("main", int(col), int(nxt))
def prep(col, nxt=0): return ("prep", int(col), int(nxt))
def first(): return ("first",)
def last(): return ("last",)
def trans(): return ("trans",)
def add(x, y): return ("add", x, y)
def sub(x, y): return ("sub", x, y)
def mul(x, y): return ("mul", x, y)
def neg(x): return ("neg", x)


SW = dict(const=0, main=1, prep=2, first=3, last=4, trans=5, add=6, sub=7, mul=8, neg=9)
SW_ASSERT = 10


def _postorder(roots):
    """Every node below `roots`, children before parents, each Python object once."""
    seen, out = set(), []
    for root in roots:
        stack = [(root, False)]
        while stack:
            e, done = stack.pop()
            if done:
                out.append(e)
                continue
            if id(e) in seen:
                continue
            seen.add(id(e))
            stack.append((e, True))
            for ch in reversed(e[1:] if e[0] in ("add", "sub", "mul", "neg") else ()):
                stack.append((ch, False))
    return out


def to_oracle_words(script):
    words = []
    for c in script.constraints:
        stack = [(c, False)]
        while stack:  # the tree written out in postfix, shared subtrees once per use
            e, done = stack.pop()
            if e[0] in ("add", "sub", "mul", "neg") and not done:
                stack.append((e, True))
                for ch in reversed(e[1:]):
                    stack.append((ch, False))
            elif e[0] == "const":
                words += [SW["const"], e[1] & 0xFFFFFFFF]
            elif e[0] in ("main", "prep"):
                words += [SW[e[0]], e[1], e[2]]
            else:
                words.append(SW[e[0]])
        words.append(SW_ASSERT)
    return np.array(words, dtype=np.uint32)


def set_oracle(script, slot=0):
    """Hand the script to the oracle's slot; returns the chip id to use with po.eval_constraints / prove_machine / verify_machine."""
    from oracle import pyoracle as po

    return po.set_script(slot, to_oracle_words(script), script.width, script.prep_width)


def capture(L, air, script):
    """The script's constraints through vgpu_air_* on an open AIR handle."""
    u = ctypes.c_uint32
    handle = {}
    for e in _postorder(script.constraints):
        k = e[0]
        if k == "const":
            h = L.vgpu_air_constant(air, u(e[1] & 0xFFFFFFFF))
        elif k in ("main", "prep"):
            h = L.vgpu_air_variable(air, u(1 if k == "prep" else 0), u(e[1]), u(e[2]))
        elif k == "first":
            h = L.vgpu_air_is_first_row(air)
        elif k == "last":
            h = L.vgpu_air_is_last_row(air)
        elif k == "trans":
            h = L.vgpu_air_is_transition(air)
        elif k == "neg":
            h = L.vgpu_air_neg(air, u(handle[id(e[1])]))
        else:
            h = getattr(L, "vgpu_air_" + k)(air, u(handle[id(e[1])]), u(handle[id(e[2])]))
        handle[id(e)] = h
    for c in script.constraints:
        L.vgpu_air_assert_zero(air, u(handle[id(c)]))


def to_ffi(scripts, codes=None):
    """va.Machine with one chip per script, each captured through vgpu_air_*.  A refused push raises, unless `codes` (a list) is given: it
    then receives (code, message) per script."""
    import valida_amd as va

    if isinstance(scripts, Script):
        scripts = [scripts]
    L, u = va.lib(), ctypes.c_uint32
    m = ctypes.c_void_p()
    assert L.vgpu_machine_new(ctypes.byref(m)) == 0
    mach = va.Machine(m)
    for s in scripts:
        air = ctypes.c_void_p()
        assert L.vgpu_air_new(s.name.encode(), u(s.width), u(s.prep_width), ctypes.byref(air)) == 0
        try:
            capture(L, air, s)
            code = L.vgpu_machine_push_air(m, air)
        finally:
            L.vgpu_air_free(air)
        msg = L.vgpu_last_error().decode() if code else ""
        if codes is not None:
            codes.append((code, msg))
        elif code:
            raise va.VgpuError(code, msg)
    return mach


def eval_py(script, local, nxt, prep_local=(), prep_next=(), first=0, last=0, trans=1):
    """The asserted values, in order, in plain integers mod p (the rows may also be uint64 numpy arrays per column: the same formulas)."""
    val = {}
    for e in _postorder(script.constraints):
        k = e[0]
        if k == "const":
            v = e[1] % P
        elif k == "main":
            v = (nxt if e[2] else local)[e[1]] % P
        elif k == "prep":
            v = (prep_next if e[2] else prep_local)[e[1]] % P
        elif k == "first":
            v = first % P
        elif k == "last":
            v = last % P
        elif k == "trans":
            v = trans % P
        elif k == "add":
            v = (val[id(e[1])] + val[id(e[2])]) % P
        elif k == "sub":
            v = (val[id(e[1])] + P - val[id(e[2])]) % P
        elif k == "mul":
            v = val[id(e[1])] * val[id(e[2])] % P
        else:
            v = (P - val[id(e[1])]) % P
        val[id(e)] = v
    return [val[id(c)] for c in script.constraints]


def degree_py(script):
    """(max constraint degree, log_quotient_degree) by the reference's rules: variables, first, last 1; constant, transition 0; add, sub, neg
    the max; mul the sum; log_quotient_degree = log2_ceil(max(degree, 3) - 1)."""
    deg = {}
    for e in _postorder(script.constraints):
        k = e[0]
        if k in ("main", "prep", "first", "last"):
            d = 1
        elif k in ("const", "trans"):
            d = 0
        elif k == "mul":
            d = deg[id(e[1])] + deg[id(e[2])]
        elif k == "neg":
            d = deg[id(e[1])]
        else:
            d = max(deg[id(e[1])], deg[id(e[2])])
        deg[id(e)] = d
    dmax = max([deg[id(c)] for c in script.constraints], default=0)
    return dmax, (max(dmax, 3) - 2).bit_length()


def boolean_selectors(h):
    """is_first, is_last, is_transition per row as the witness check sees them (DebugConstraintBuilder): 0 / 1."""
    r = np.arange(h)
    return (r == 0).astype(np.uint64), (r == h - 1).astype(np.uint64), (r != h - 1).astype(np.uint64)


def domain_selectors(h):
    """The same selectors as the PROOF sees them, the polynomials Z_H(x) / (x - 1), Z_H(x) / (x - g^-1), x - g^-1 on the trace domain x = g^r:
    h at row 0, h g at row h - 1 (the derivative of Z_H there; 0 elsewhere), g^r - g^-1."""
    from oracle import pyoracle as po

    g = int(po.lib().oracle_two_adic_generator(ctypes.c_uint32(h.bit_length() - 1)))
    x = np.array([pow(g, r, P) for r in range(h)], dtype=np.uint64)
    r = np.arange(h)
    return ((r == 0) * np.uint64(h % P)).astype(np.uint64), ((r == h - 1) * np.uint64(h * g % P)).astype(np.uint64), (x + np.uint64(P - pow(g, -1, P))) % np.uint64(P)


def satisfiable(script):
    """(script', fill): script' has one more main column per constraint, constraint j being col_j - expr_j = 0; fill(main, prep, domain)
    completes a (height, width) matrix of free values to the (height, width') trace on which every constraint holds on every row -- with the
    0 / 1 selectors of the witness check (domain=False: what prove(check=True) accepts), or with the selector polynomials' values on the trace
    domain (domain=True: what a proof that verifies needs).  The two traces differ only where a selector is used as a value, not as a gate."""
    w = script.width
    sat = Script(script.name + "+sat", w + len(script.constraints), script.prep_width, [sub(main(w + j), c) for j, c in enumerate(script.constraints)])

    def fill(free, pre=None, domain=False):
        free = np.asarray(free, dtype=np.uint64)
        h = free.shape[0]
        assert free.shape[1] == w
        nx = np.roll(free, -1, axis=0)
        pl = np.zeros((h, 0), np.uint64) if pre is None else np.asarray(pre, dtype=np.uint64)
        pn = np.roll(pl, -1, axis=0)
        vals = eval_py(script, free.T, nx.T, pl.T, pn.T, *(domain_selectors(h) if domain else boolean_selectors(h)))
        cols = [np.broadcast_to(np.asarray(v, dtype=np.uint64), (h,)) for v in vals]
        return np.concatenate([free] + [c[:, None] for c in cols], axis=1).astype(np.uint32)

    return sat, fill


def first_failing_row(script, trace, pre=None):
    """The first row of `trace` on which some constraint is non-zero (row r against row r + 1 mod h, 0/1 selectors), or None."""
    t = np.asarray(trace, dtype=np.uint64)
    h = t.shape[0]
    pl = np.zeros((h, 0), np.uint64) if pre is None else np.asarray(pre, dtype=np.uint64)
    vals = eval_py(script, t.T, np.roll(t, -1, axis=0).T, pl.T, np.roll(pl, -1, axis=0).T, *boolean_selectors(h))
    bad = np.zeros(h, bool)
    for v in vals:
        bad |= np.broadcast_to(np.asarray(v, dtype=np.uint64) != 0, (h,))
    return int(np.nonzero(bad)[0][0]) if bad.any() else None


# ---- traces ---------------------------------------------------------------------------------------------------------------------------------
def trace(seed, h, w):
    """Seeded uniform words, with rows of 0, 1 and p - 1 where the height leaves room for them."""
    rng = np.random.default_rng([0xA125, seed, h, w])
    t = rng.integers(0, P, (h, w), dtype=np.uint64)
    for r, v in ((1, 0), (2, 1), (h - 1, P - 1)):
        if 0 < r < h and h >= 4:
            t[r] = v
    return t.astype(np.uint32)


def eval_rows(seed, w, pw):
    """(local, next, prep_local, prep_next, first, last, trans) tuples: every 0/1 selector combination, edge rows, off-domain selector values."""
    rng = np.random.default_rng([0xA126, seed, w, pw])
    rows = []
    edge = [0, 1, P - 1]
    for i in range(8):  # all selector combinations, on uniform rows
        rows.append((rng.integers(0, P, w), rng.integers(0, P, w), rng.integers(0, P, pw), rng.integers(0, P, pw), i & 1, i >> 1 & 1, i >> 2 & 1))
    for a in edge:      # constant rows of 0, 1, p - 1 against each other
        for b in edge:
            rows.append((np.full(w, a), np.full(w, b), np.full(pw, b), np.full(pw, a), a, b, (a + b) % P))
    for _ in range(4):  # words of the edge corpus, selectors anywhere in the field (the quotient domain's are)
        pick = lambda n: np.asarray(E, dtype=np.uint64)[rng.integers(0, len(E), n)]
        rows.append((pick(w), pick(w), pick(pw), pick(pw), int(rng.integers(0, P)), int(rng.integers(0, P)), int(rng.integers(0, P))))
    return [tuple(np.asarray(x, dtype=np.uint32) if isinstance(x, np.ndarray) else int(x) for x in r) for r in rows]


# ---- the named corpus -----------------------------------------------------------------------------------------------------------------------
def power(x, d):
    p = x
    for _ in range(d - 1):
        p = mul(p, x)
    return p


def held_products(k, lqd=1):
    """k products x0 * c_i asserted in order and again in reverse order: all k stay live until the second pass, and the program needs k + 1
    registers (the k products and, until the last product, x0 -- whose register the last constant takes over).  lqd 2 / 3: one x1^5 / x1^9
    constraint in front (a handful of registers, long dead when the products pile up)."""
    x0 = main(0)
    cs = []
    if lqd > 1:
        cs.append(sub(main(2), power(main(1), 5 if lqd == 2 else 9)))
    ps = [mul(x0, const(i + 2)) for i in range(k)]
    return Script("regs_%d_lqd%d" % (k + 1, lqd), 3, 0, cs + ps + ps[::-1])


# the largest register files the LDS interpreters hold (valida_amd/csrc/kernels/launch.hpp): 148 KiB (k_quotient<0>: log_quotient_degree 1) and
# 160 KiB (k_quotient_general<0>: above) of one wave's four-byte slots
MAX_REGS_PAIR, MAX_REGS_GENERAL = 148 * 1024 // 256, 160 * 1024 // 256
REGISTER_CASES = [(1, 1), (31, 1), (63, 1)] + [(r, q) for r in (32, 33, 64, 65, 200) for q in (1, 2, 3)] + [(MAX_REGS_PAIR, 1), (MAX_REGS_GENERAL, 2)]


def _corpus():
    x, y, z = main(0), main(1), main(2)
    c = {}

    def put(name, width, prep_width, constraints):
        assert name not in c
        c[name] = Script(name, width, prep_width, list(constraints))

    # registers: the boundaries of the one-bank / two-bank VGPR files and of the LDS file, at every log_quotient_degree that reaches them
    put("regs_1_lqd1", 3, 0, [x])
    for r, q in REGISTER_CASES[1:]:
        s = held_products(r - 1, q)
        c[s.name] = s
    # length and padding: unpadded lengths 4, 5, 6, 7 (a bare variable is LOAD + ASSERT, its negation one more); no constraints at all
    put("pad_len4", 3, 0, [x, y])
    put("pad_len5", 3, 0, [x, neg(y)])
    put("pad_len6", 3, 0, [x, y, z])
    put("pad_len7", 3, 0, [x, y, neg(z)])
    put("no_constraints", 3, 0, [])
    # opcodes and operands
    put("every_opcode", 2, 1, [sub(mul(add(x, const(5)), prep(0)), neg(mul(first(), add(last(), trans())))), mul(main(1, 1), prep(0, 1))])
    put("sub_both_orders", 2, 0, [sub(x, y), sub(y, x)])
    put("operand_id_orders", 2, 0, [add(x, y), mul(x, y), add(main(1), main(0)), mul(main(1), main(0)), add(add(y, x), x), mul(mul(y, x), x)])
    put("neg_of_neg", 1, 0, [neg(neg(x)), neg(neg(neg(x)))])
    t = x
    for i in range(40):  # every destination may take the register of the source that dies in it
        t = [add, sub, mul][i % 3](t, const(i + 2)) if i % 4 else neg(t)
    put("alias_chain", 1, 0, [t])
    keep = mul(add(x, y), z)
    put("late_last_use", 3, 0, [keep] + [mul(main(i % 3), const(i + 7)) for i in range(9)] + [sub(keep, x)])
    # folds of the capture (air/symbolic.hpp), each one asserted on its own and inside a product
    zero, one = const(0), const(1)
    folds = [add(x, zero), add(zero, x), sub(x, zero), sub(zero, x), sub(x, x), mul(x, zero), mul(zero, x), mul(x, one), mul(one, x)]
    put("folds", 2, 0, folds + [mul(add(f, y), y) for f in [add(x, const(0)), sub(const(0), x), sub(x, main(0)), mul(x, const(0)), mul(const(1), x)]])
    m1 = const(P - 1)
    put("const_const", 1, 0, [add(m1, const(P - 1)), sub(const(0), m1), sub(m1, const(P - 1)), mul(m1, const(P - 1)), neg(m1), sub(const(1), m1), mul(add(m1, m1), x),
                              mul(mul(m1, m1), x), add(neg(const(0)), x)])
    put("const_unreduced", 1, 0, [const(P), const(P + 1), const(2 ** 32 - 1), mul(const(P), x), mul(const(P + 1), x), mul(const(2 ** 32 - 1), x), add(const(P), x)])
    # asserts
    shared = mul(x, y)
    put("assert_forms", 2, 0, [x, main(1, 1), first(), last(), trans(), const(0), const(7), shared, shared, add(x, y), shared, mul(main(0), main(1)), add(main(0), main(1))])
    # loads
    put("load_main_w1", 1, 0, [sub(main(0, 1), main(0, 0))])
    put("load_edges", 5, 0, [main(0), main(4), main(0, 1), main(4, 1), mul(main(0), main(4, 1))])
    put("load_prep_w1", 2, 1, [sub(x, prep(0)), mul(prep(0, 1), y)])
    put("load_prep_w7", 2, 7, [sub(prep(0), prep(6)), mul(prep(6, 1), prep(0, 1)), add(mul(prep(3), x), prep(6))])
    put("load_main_w300", 300, 0, [sub(main(299), main(0)), mul(main(256), main(255, 1)), add(main(299, 1), main(257))])
    # selectors
    put("selectors", 2, 0, [mul(first(), x), mul(last(), x), mul(trans(), sub(main(0, 1), x)), first(), last(), trans()])
    put("first_times_last", 2, 0, [mul(mul(first(), last()), x)])
    # degrees 3, 4, 5, 8, 9 (log_quotient_degree 1, 2, 2, 3, 3); 10 is refused; folded expressions keep the reference's degree
    for d in (3, 4, 5, 8, 9, 10):
        put("degree_%d" % d, 2, 0, [sub(y, power(x, d))])
    put("fold_zero_times_x4", 2, 0, [mul(const(0), power(x, 4)), sub(y, x)])
    x5 = power(x, 5)
    put("fold_x5_minus_x5", 2, 0, [sub(x5, x5), sub(y, x)])
    # constraint counts: the lazy group of four, the alpha-power table
    for n in (1, 4, 5, 300):
        put("constraints_%d" % n, 4, 0, [sub(mul(main(i % 4), const(i + 2)), main((i + 1) % 4, i & 1)) for i in range(n)])
    return c


CORPUS = _corpus()
NAMED = (["regs_%d_lqd%d" % rq for rq in REGISTER_CASES] + ["pad_len4", "pad_len5", "pad_len6", "pad_len7", "no_constraints", "every_opcode", "sub_both_orders",
         "operand_id_orders", "neg_of_neg", "alias_chain", "late_last_use", "folds", "const_const", "const_unreduced", "assert_forms", "load_main_w1", "load_edges",
         "load_prep_w1", "load_prep_w7", "load_main_w300", "selectors", "first_times_last", "degree_3", "degree_4", "degree_5", "degree_8", "degree_9", "degree_10",
         "fold_zero_times_x4", "fold_x5_minus_x5", "constraints_1", "constraints_4", "constraints_5", "constraints_300"])
REFUSED = ["degree_10"]  # VGPU_ERR_UNSUPPORTED at vgpu_machine_push_air
N_GENERATED = 40


def generated(seed):
    """A seeded random DAG: width <= 8, preprocessed width <= 3, degree <= 9, constants from the edge corpus; subtrees are shared."""
    rng = np.random.default_rng([0xA127, seed])
    w, pw = int(rng.integers(1, 9)), int(rng.integers(0, 4))
    cap = [3, 5, 9, 9][seed % 4]
    pool = [(main(int(rng.integers(0, w)), int(rng.integers(0, 2))), 1) for _ in range(3)] + [(const(E[int(rng.integers(0, len(E)))]), 0)]
    if pw:
        pool.append((prep(int(rng.integers(0, pw)), int(rng.integers(0, 2))), 1))
    pool += [(first(), 1), (last(), 1), (trans(), 0)][:int(rng.integers(0, 4))]
    for _ in range(int(rng.integers(4, 40))):
        op = int(rng.integers(0, 10))
        (a, da), (b, db) = pool[int(rng.integers(0, len(pool)))], pool[int(rng.integers(0, len(pool)))]
        if op < 4 and da + db <= cap:
            pool.append((mul(a, b), da + db))
        elif op < 6:
            pool.append((add(a, b), max(da, db)))
        elif op < 8:
            pool.append((sub(a, b), max(da, db)))
        elif op == 8:
            pool.append((neg(a), da))
        else:
            k = int(rng.integers(0, 3))
            pool.append(([const(E[int(rng.integers(0, len(E)))]), main(int(rng.integers(0, w)), int(rng.integers(0, 2))), const(int(rng.integers(0, 2)))][k], 1 if k == 1 else 0))
    n = int(rng.integers(1, 9))
    picks = [pool[int(i)][0] for i in rng.integers(len(pool) // 2, len(pool), n)]
    return Script("generated_%d" % seed, w, pw, picks)


Sat = namedtuple("Sat", "script fill free_width break_col")


def satisfiable_case(name):
    """Sat(script, fill, free_width, break_col) of the case `name`: a script with the case's program shape, the filler fill(free, prep, domain)
    that completes a (height, free_width) matrix of free values to a trace on which every constraint holds, and a column in which any changed
    cell breaks a constraint on that row.  In general this is satisfiable() (break_col: the last result column).  The held-products programs
    stay as they are -- a result column per constraint would cost a register and over a thousand columns: x0 * c_i = 0 holds where column 0
    is 0, and the power constraint in front where column 2 is column 1 to the 5th or 9th."""
    if name.startswith("regs_"):
        s = all_cases()[name]
        d = {1: 0, 2: 5, 3: 9}[int(name[-1])]

        def fill(free, pre=None, domain=False):
            t = np.array(free, dtype=np.uint64)
            t[:, 0] = 0
            if d:
                t[:, 2] = [pow(int(v), d, P) for v in t[:, 1]]
            return t.astype(np.uint32)
        return Sat(s._replace(name=name + "+sat"), fill, s.width, 0)
    s, fill = satisfiable(all_cases()[name])
    return Sat(s, fill, s.width - len(s.constraints), s.width - 1)


def all_cases():
    """name -> Script: the named corpus and the generated DAGs."""
    out = dict(CORPUS)
    for seed in range(N_GENERATED):
        s = generated(seed)
        out[s.name] = s
    return out
