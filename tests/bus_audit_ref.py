"""An independent numpy restatement of the bus-audit contract (include/vgpu.h).  It uses nothing of the audit's own code:
only Machine.interactions(chip) (the neutral interaction word image) and host traces.  Evaluate the virtual columns mod p, drop count == 0, pad per
bus to the widest interaction, np.unique(axis=0), sum the counts mod p, order by first record.  Test infrastructure; the product never imports it."""
import numpy as np

P = 2013265921


def vcol(v, main, prep):  # v = (constant, [(is_preprocessed, column, weight), ...])
    acc = np.full(main.shape[0], v[0] % P, dtype=np.uint64)
    for is_prep, col, weight in v[1]:
        acc = (acc + (prep if is_prep else main)[:, col].astype(np.uint64) * np.uint64(weight)) % np.uint64(P)
    return acc


def audit(machine, mains, preps):
    """-> dict(tuples = every unbalanced tuple in report order with ALL its records, buses = per-bus statistics, total_unbalanced, live, pairs,
    largest_group)."""
    prep_of, per_bus, out, widths = dict(preps), {}, [], {}
    pairs = 0
    for chip in range(machine.num_chips):
        for m, it in enumerate(machine.interactions(chip)):
            bus = (int(it["global"]), int(it["bus"]))
            widths[bus] = max(widths.get(bus, 0), len(it["fields"]))
            pairs += mains[chip].shape[0]
            cnt = vcol(it["count"], mains[chip], prep_of.get(chip))
            live = np.nonzero(cnt)[0]
            if live.size:
                f = np.stack([vcol(x, mains[chip], prep_of.get(chip))[live] for x in it["fields"]], axis=1) if it["fields"] else np.zeros((live.size, 0), np.uint64)
                ids = np.stack([np.full(live.size, chip), live, np.full(live.size, m)], axis=1)
                per_bus.setdefault(bus, []).append((f, cnt[live], np.full(live.size, 1 if it["send"] else 0), ids))
    buses, largest = [], 0
    for bus in sorted(widths):
        W = widths[bus]
        parts = per_bus.get(bus, [])
        stat = dict(bus=bus, width=W, live=0, sends=0, receives=0, unbalanced=0)
        if parts:
            f = np.concatenate([np.pad(p[0], ((0, 0), (0, W - p[0].shape[1]))) for p in parts])
            c, snd, ids = (np.concatenate([p[k] for p in parts]) for k in (1, 2, 3))
            u, inv, sizes = np.unique(f, axis=0, return_inverse=True, return_counts=True)
            inv = inv.reshape(-1)
            largest = max(largest, int(sizes.max()))
            s_sum, r_sum = np.zeros(len(u), dtype=np.uint64), np.zeros(len(u), dtype=np.uint64)
            np.add.at(s_sum, inv[snd == 1], c[snd == 1])
            np.add.at(r_sum, inv[snd == 0], c[snd == 0])
            s_sum %= np.uint64(P)
            r_sum %= np.uint64(P)
            net = (s_sum + np.uint64(P) - r_sum) % np.uint64(P)
            stat.update(live=int(len(c)), sends=int(snd.sum()), receives=int(len(c) - snd.sum()), unbalanced=int(np.count_nonzero(net)))
            bad = np.nonzero(net)[0]
            if bad.size:
                sel = np.nonzero(np.isin(inv, bad))[0]  # one pass over the records of the unbalanced tuples
                order = sel[np.lexsort((ids[sel, 2], ids[sel, 1], ids[sel, 0], inv[sel]))]
                starts = np.concatenate([[0], np.nonzero(np.diff(inv[order]))[0] + 1, [order.size]])
                for a, b in zip(starts[:-1], starts[1:]):
                    g, rows = int(inv[order[a]]), order[a:b]
                    n = int(net[g])
                    out.append(dict(bus=bus, fields=[int(x) for x in u[g]], net=n, net_signed=n if n <= P // 2 else n - P, send_sum=int(s_sum[g]), recv_sum=int(r_sum[g]),
                                    n_send=int(snd[rows].sum()), n_recv=int(rows.size - snd[rows].sum()),
                                    records=[(int(ids[i, 0]), int(ids[i, 1]), int(ids[i, 2]), int(snd[i]), int(c[i])) for i in rows]))
        buses.append(stat)
    out.sort(key=lambda r: r["records"][0][:3])
    return dict(tuples=out, buses=buses, total_unbalanced=len(out), live=sum(b["live"] for b in buses), pairs=pairs, largest_group=largest)


def expect(ref, max_tuples=64, max_records_per_tuple=4):
    """What a report must say for these options: (tuples, buses, total_unbalanced, truncated)."""
    tuples = [dict(t, records=t["records"][:max_records_per_tuple]) for t in ref["tuples"][:max_tuples]]
    return tuples, ref["buses"], ref["total_unbalanced"], ref["total_unbalanced"] > len(tuples)


def assert_report_equals(report, ref, max_tuples=64, max_records_per_tuple=4):
    """Field for field: tuples, buses, total_unbalanced, truncated (and what follows from them: balanced, reported)."""
    tuples, buses, total, truncated = expect(ref, max_tuples, max_records_per_tuple)
    assert report.total_unbalanced == total, (report.total_unbalanced, total)
    assert report.truncated == truncated and report.balanced == (total == 0) and report.reported == len(tuples)
    assert report.buses == buses, (report.buses, buses)
    assert len(report.tuples) == len(tuples)
    for got, want in zip(report.tuples, tuples):
        assert got == want, (got, want)
