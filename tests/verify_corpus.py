"""Proof corpora for the batched verifier's tests (test_verify_batch_*): single-word mutations at the positions of
test_machine_verify_cpu.py's tampering test, and hostile shapes (length fields, paths one digest off, heights past the two-adicity, wrong
counts) built by walking the VPF1 layout (DESIGN.md "Proof wire format")."""
import numpy as np

P = 2013265921


def head_end(words, n_chips=14):
    """First word after the per-chip openings."""
    at = 26
    for _ in range(n_chips):
        at += 1
        for _ in range(5):
            at += 1 + 5 * int(words[at])
        at += 5
    return at


def mutate(words, at):
    bad = words.copy()
    bad[at] = (int(bad[at]) + 1) % P if bad[at] < P else 0
    return bad


def mutations(words, n_tail, seed, stride=7, n_chips=14):
    """Every `stride`-th head word and n_tail random tail words, one mutated word each (the unchanged ones left out)."""
    rng = np.random.default_rng(seed)
    he = head_end(words, n_chips)
    positions = list(range(2, he, stride)) + [int(x) for x in rng.integers(he, words.size, n_tail)]
    return [mutate(words, at) for at in positions if not (words[at] == (int(words[at]) + 1) % P)]


def layout(words, n_chips=14):
    """Word positions of the FRI tail: dict with the commit-phase path length fields [query][layer], the opened rows' length fields
    [query][round][matrix] and the input-round path length fields [query][round]."""
    w = [int(x) for x in words]
    at = head_end(words, n_chips)
    out = {"step_path": [], "row": [], "in_path": []}
    at += 1 + 8 * w[at]  # commit-phase roots
    nq = w[at]
    at += 1
    for _ in range(nq):
        ns = w[at]
        at += 1
        paths = []
        for _ in range(ns):
            at += 5
            paths.append(at)
            at += 1 + 8 * w[at]
        out["step_path"].append(paths)
    at += 6  # final polynomial, witness
    nq = w[at]
    at += 1
    for _ in range(nq):
        nr = w[at]
        at += 1
        rows, paths = [], []
        for _ in range(nr):
            nm = w[at]
            at += 1
            r = []
            for _ in range(nm):
                r.append(at)
                at += 1 + w[at]
            rows.append(r)
            paths.append(at)
            at += 1 + 8 * w[at]
        out["row"].append(rows)
        out["in_path"].append(paths)
    assert at == len(w)
    return out


def _splice(words, at, remove=0, insert=()):
    return np.concatenate([words[:at], np.asarray(insert, dtype=np.uint32), words[at + remove:]]).astype(np.uint32)


def hostile(words, n_chips=14):
    """Malformed proofs: (label, words).  Every one must be rejected while the plan is built, or at the shape check the host verifier meets."""
    L = layout(words, n_chips)
    out = []
    for at in (1, 26 + 1, head_end(words, n_chips), L["step_path"][0][0], L["row"][1][0][0], L["in_path"][0][2]):
        bad = words.copy()
        bad[at] = 0xFFFFFFFF
        out.append(("length field 2^32-1 at word %d" % at, bad))
    # sibling paths one digest short / long (the length field kept consistent): the walk would end off the root
    for q, key in ((0, "in_path"), (1, "in_path"), (0, "step_path"), (2, "step_path")):
        at = L[key][q][1] if key == "in_path" else L[key][q][len(L[key][q]) // 2]
        n = int(words[at])
        short = _splice(words, at, 1 + 8 * n, np.concatenate([[n - 1], words[at + 1: at + 1 + 8 * (n - 1)]]))
        long_ = _splice(words, at, 1, np.concatenate([[n + 1], words[at + 1: at + 9]]))
        out += [("%s q%d one digest short" % (key, q), short), ("%s q%d one digest long" % (key, q), long_)]
    # an opened row one column short at query 1 (query 0's checks come first), and the same with query 0's row tampered too
    at = L["row"][1][0][3]
    n = int(words[at])
    narrow = _splice(words, at, 1 + n, np.concatenate([[n - 1], words[at + 1: at + n]]))
    out.append(("row one column short at query 1", narrow))
    out.append(("query 0 row tampered, query 1 row short", mutate(narrow, L["row"][0][0][3] + 1)))
    # heights past the two-adicity / the first FRI layer: chip 0's log_degree
    for ld in (26, 27, 40, 0xFFFFFFFF):
        bad = words.copy()
        bad[26] = ld
        out.append(("log_degree %d" % ld, bad))
    # an opened-values vector one element short (chip 0's trace_local)
    n = int(words[27])
    out.append(("trace_local one value short", _splice(words, 27, 1 + 5 * n, np.concatenate([[n - 1], words[28: 28 + 5 * (n - 1)]]))))
    # counts: rounds of a query, queries
    bad = words.copy()
    bad[L["row"][0][0][0] - 2] += 1
    out.append(("rounds of query 0 + 1", bad))
    out.append(("truncated", words[:-1].copy()))
    out.append(("extended", np.concatenate([words, [0]]).astype(np.uint32)))
    out.append(("empty", np.zeros(0, dtype=np.uint32)))
    out.append(("one word", words[:1].copy()))
    return out
