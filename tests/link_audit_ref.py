"""An independent restatement of the link audit's contract (include/vgpu.h, "Link audit").  The float masks are the field audit reference's
(field_audit_ref.chip_rows: exact interpolation of the oracle's own chips, one numpy RREF per field), the tuples the bus audit reference's way
(bus_audit_ref.vcol, per-bus zero padding, np.unique(axis=0)); the join is one AND per tuple.  Nothing of the audit's own code is used.  Test
infrastructure; the product never imports it."""
import numpy as np

import bus_audit_ref as br
import field_audit_ref as fr
import rank_audit_ref as rr

MAGIC = 0x31414C56


def audit(machine, mains, preps):
    """The contract's report as LinkReport's attributes, every open tuple with ALL its records (cut() applies limits)."""
    prep_of = dict(preps)
    per_bus, widths, chips = {}, {}, []
    for chip in range(machine.num_chips):
        t = np.asarray(mains[chip])
        inter = machine.interactions(chip)
        rows = None
        recs = []
        for m, it in enumerate(inter):
            bus = (int(it["global"]), int(it["bus"]))
            nf = len(it["fields"])
            widths[bus] = max(widths.get(bus, 0), nf)
            rec = dict(interaction=m, is_send=bool(it["send"]), is_global=bool(it["global"]), bus_index=it["bus"], fields=nf, live_rows=0,
                       constant=[not rr._weights(fl, t.shape[1]).any() for fl in it["fields"]], floating=[0] * nf, open=[0] * nf)
            recs.append(rec)
            cnt = br.vcol(it["count"], t, prep_of.get(chip))
            live = np.nonzero(cnt)[0]
            if not live.size:
                continue
            if rows is None:
                rows = [{mm: sum(1 << j for j in fl) for mm, fl in row.items()} for row in fr.chip_rows(machine, chip, t, prep_of.get(chip))]
            f = np.stack([br.vcol(x, t, prep_of.get(chip))[live] for x in it["fields"]], axis=1) if nf else np.zeros((live.size, 0), np.uint64)
            mk = np.array([rows[int(r)][m] for r in live], dtype=np.uint64)
            ids = np.stack([np.full(live.size, chip), live, np.full(live.size, m)], axis=1)
            per_bus.setdefault(bus, []).append((f, mk, np.full(live.size, 1 if it["send"] else 0), ids))
            rec["live_rows"] = int(live.size)
            for j in range(nf):
                rec["floating"][j] = int(np.count_nonzero((mk >> np.uint64(j)) & np.uint64(1)))
        chips.append(dict(chip=chip, records=recs))
    buses, out, largest = [], [], 0
    for bus in sorted(widths):
        W = widths[bus]
        assert W <= 32
        parts = per_bus.get(bus, [])
        stat = dict(bus=bus, width=W, live=0, tuples=0, open_tuples=0, open_in=[0] * W, open_records=[0] * W)
        if parts:
            f = np.concatenate([np.pad(p[0], ((0, 0), (0, W - p[0].shape[1]))) for p in parts])
            mk, snd, ids = (np.concatenate([p[k] for p in parts]) for k in (1, 2, 3))
            u, inv, sizes = np.unique(f, axis=0, return_inverse=True, return_counts=True)
            inv = inv.reshape(-1)
            largest = max(largest, int(sizes.max()))
            tm = np.full(len(u), 0xffffffff, dtype=np.uint64)
            np.bitwise_and.at(tm, inv, mk)
            stat.update(live=int(len(mk)), tuples=int(len(u)), open_tuples=int(np.count_nonzero(tm)))
            for j in range(W):
                is_open = ((tm >> np.uint64(j)) & np.uint64(1)).astype(bool)
                stat["open_in"][j] = int(np.count_nonzero(is_open))
                stat["open_records"][j] = int(sizes[is_open].sum())
            for i in range(len(mk)):  # the record-level split
                c, _, m = (int(x) for x in ids[i])
                rec = chips[c]["records"][m]
                for j in range(rec["fields"]):
                    if (int(mk[i]) >> j) & 1 and (int(tm[inv[i]]) >> j) & 1:
                        rec["open"][j] += 1
            order = np.lexsort((ids[:, 2], ids[:, 1], ids[:, 0], inv))
            starts = np.concatenate([[0], np.nonzero(np.diff(inv[order]))[0] + 1, [order.size]])
            for a, b in zip(starts[:-1], starts[1:]):
                g, rows_ = int(inv[order[a]]), order[a:b]
                if not tm[g]:
                    continue
                mask = int(tm[g])
                out.append(dict(bus=bus, mask=mask, open=[j for j in range(W) if (mask >> j) & 1], n_send=int(snd[rows_].sum()), n_recv=int(rows_.size - snd[rows_].sum()),
                                fields=[int(x) for x in u[g]], records=[(int(ids[i, 0]), int(ids[i, 1]), int(ids[i, 2]), int(snd[i]), int(mk[i])) for i in rows_]))
        buses.append(stat)
    out.sort(key=lambda r: r["records"][0][:3])
    return dict(truncated=False, open_tuples=len(out), buses=buses, chips=chips, tuples=out, largest_group=largest)


def cut(want, max_tuples=64, max_records_per_tuple=4):
    """audit()'s dict cut to the limits of a report (the counts do not depend on them)."""
    tuples = [dict(t, records=t["records"][:max_records_per_tuple]) for t in want["tuples"][:max_tuples]]
    return dict(want, truncated=want["open_tuples"] > len(tuples), tuples=tuples)


def assert_report_equals(rep, want):
    """A LinkReport (valida_amd) against cut()'s dict."""
    assert (rep.truncated, rep.open_tuples, rep.reported) == (want["truncated"], want["open_tuples"], len(want["tuples"]))
    assert rep.buses == want["buses"], (rep.buses, want["buses"])
    for got, exp in zip(rep.chips, want["chips"]):
        assert got == exp, (got, exp)
    assert len(rep.chips) == len(want["chips"])
    for got, exp in zip(rep.tuples, want["tuples"]):
        assert got == exp, (got, exp)


def words(want):
    """The report's flat word image (include/vgpu.h) of cut()'s dict."""
    def u64(v):
        return [v & 0xffffffff, v >> 32]

    w = [MAGIC, 0, int(want["truncated"])] + u64(want["open_tuples"]) + [len(want["tuples"]), len(want["buses"]), len(want["chips"])]
    for b in want["buses"]:
        w += [b["bus"][0], b["bus"][1], b["width"]] + u64(b["live"]) + u64(b["tuples"]) + u64(b["open_tuples"])
        for j in range(b["width"]):
            w += u64(b["open_in"][j]) + u64(b["open_records"][j])
    for c in want["chips"]:
        w += [len(c["records"])]
        for r in c["records"]:
            w += [int(r["is_send"]), int(r["is_global"]), r["bus_index"], r["fields"]] + u64(r["live_rows"])
            for j in range(r["fields"]):
                w += [int(r["constant"][j])] + u64(r["floating"][j]) + u64(r["open"][j])
    for t in want["tuples"]:
        w += [t["bus"][0], t["bus"][1], len(t["fields"]), t["mask"]] + u64(t["n_send"]) + u64(t["n_recv"]) + [len(t["records"])] + list(t["fields"])
        for r in t["records"]:
            w += list(r)
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
