"""A numpy restatement of the domain audit's contract (include/vgpu.h, "Domain audit"), written from its text: virtual columns over whole
columns, liveness, the column domains by np.unique, the lookup buses from the machine's interaction lists (vgpu_machine_interaction_words), the
appearances and guards as boolean row vectors, the bus positions over the concatenated live records of the whole machine, and the report's word
image.  Nothing here calls the audit under test."""
import numpy as np

import valida_amd as va

P = va.P
CLASSES = ("constant", "boolean", "byte", "half", "wide")


def vcol(v, main, prep):
    const, terms = v
    acc = np.full(main.shape[0], const % P, dtype=np.uint64)
    for is_prep, col, weight in terms:
        src = prep if is_prep else main
        acc = (acc + np.uint64(weight % P) * (src[:, col].astype(np.uint64) % np.uint64(P))) % np.uint64(P)
    return acc


def bare(v):
    const, terms = v
    if const == 0 and len(terms) == 1 and not terms[0][0] and terms[0][2] == 1:
        return terms[0][1]
    return None


def domain(values):
    """min, max, distinct_narrow, class, dense, bits, nonzero, wide of a non-empty vector of canonical values"""
    mn, mx = int(values.min()), int(values.max())
    wide = int((values >= 65536).sum())
    distinct = int(np.unique(values[values < 65536]).size)
    cls = 0 if mn == mx else 1 if mx <= 1 else 2 if mx < 256 else 3 if mx < 65536 else 4
    return dict(min=mn, max=mx, distinct=distinct, cls=cls, dense=int(wide == 0 and distinct == mx - mn + 1), bits=mx.bit_length(), nonzero=int((values != 0).sum()), wide=wide)


def lookup_buses(machine, lookup=None):
    """[(is_global, bus_index, lookup, width)] ascending; lookup: None (the structural rule) or a set of (is_global, bus_index)"""
    its = [machine.interactions(c) for c in range(machine.num_chips)]
    table = [machine.chip_info(c)["constraints"] == 0 and not any(i["send"] for i in its[c]) and any(not i["send"] for i in its[c]) for c in range(machine.num_chips)]
    buses = {}
    for c, lst in enumerate(its):
        for i in lst:
            b = buses.setdefault((int(i["global"]), i["bus"]), dict(width=0, receive=False, all_table=True))
            b["width"] = max(b["width"], len(i["fields"]))
            if not i["send"]:
                b["receive"] = True
                b["all_table"] = b["all_table"] and table[c]
    out = []
    for key in sorted(buses):
        b = buses[key]
        flag = (b["receive"] and b["all_table"]) if lookup is None else ((bool(key[0]), key[1]) in lookup)
        out.append((key[0], key[1], int(flag), b["width"]))
    return out, table


def audit(machine, main, preprocessed, max_entries=1024, max_rows_per_entry=4, chips=None, max_bits=16, lookup=None):
    NC = machine.num_chips
    prep_of = {c: np.asarray(m, dtype=np.uint64) for c, m in preprocessed}
    buses, table = lookup_buses(machine, lookup)
    bus_no = {(b[0], b[1]): k for k, b in enumerate(buses)}
    # the values of the live records per (bus, position, is_send)
    offered = {}
    chip_blocks, entries, total = [], [], 0
    for c in range(NC):
        info, its = machine.chip_info(c), machine.interactions(c)
        m = np.asarray(main[c], dtype=np.uint64) % np.uint64(P)
        n, w = m.shape
        audited = chips is None or c in chips
        live = [vcol(i["count"], m, prep_of.get(c)) != 0 for i in its]
        for i, lv in zip(its, live):
            for j, f in enumerate(i["fields"]):
                offered.setdefault((bus_no[(int(i["global"]), i["bus"])], j, int(i["send"])), []).append(vcol(f, m, prep_of.get(c))[lv])
        block = dict(width=w, constraints=info["constraints"], interactions=len(its), audited=int(audited), height=n, is_table=int(table[c]), narrow=0, entries=0, appearances=0, cols=[])
        chip_blocks.append(block)
        if not audited:
            continue
        for col in range(w):
            d = domain(m[:, col])
            narrow = int(d["cls"] in (2, 3) and d["max"] < (1 << max_bits))
            guarded, sent, received, mixed = (np.zeros(n, dtype=bool) for _ in range(4))
            apps = []
            for k, (i, lv) in enumerate(zip(its, live)):
                is_lookup = bool(i["send"] and buses[bus_no[(int(i["global"]), i["bus"])]][2])
                for j, f in enumerate(i["fields"]):
                    if bare(f) == col:
                        apps.append(dict(interaction=k, position=j, is_send=int(i["send"]), is_global=int(i["global"]), bus_index=i["bus"], lookup=int(is_lookup), live=int(lv.sum())))
                        if not i["send"]:
                            received |= lv
                        elif is_lookup:
                            guarded |= lv
                        else:
                            sent |= lv
                    elif i["send"] and any(not t[0] and t[1] == col for t in f[1]):
                        mixed |= lv
            ungnz = ~guarded & (m[:, col] != 0)
            d.update(narrow=narrow, n_app=len(apps), guarded=int(guarded.sum()), sent=int(sent.sum()), received=int(received.sum()), unguarded=n - int(guarded.sum()),
                     ungnz=int(ungnz.sum()), mixed=int(mixed.sum()))
            block["cols"].append(d)
            block["appearances"] += len(apps)
            block["narrow"] += narrow
            if narrow and d["ungnz"]:
                block["entries"] += 1
                total += 1
                if len(entries) < max_entries:
                    rows = np.flatnonzero(ungnz)[:max_rows_per_entry]
                    entries.append(dict(chip=c, column=col, cls=d["cls"], max=d["max"], ungnz=d["ungnz"], apps=apps, rows=[(int(r), int(m[r, col])) for r in rows]))
    positions = []
    for k, b in enumerate(buses):
        for j in range(b[3]):
            for is_send in (1, 0):
                vals = np.concatenate(offered.get((k, j, is_send), [np.zeros(0, dtype=np.uint64)]))
                rec = dict(bus=k, position=j, is_send=is_send, lookup=b[2], min=0, max=0, distinct=0, wide=0, records=int(vals.size))
                if vals.size:
                    d = domain(vals)
                    rec.update(min=d["min"], max=d["max"], distinct=d["distinct"], wide=d["wide"])
                positions.append(rec)
    return dict(max_bits=max_bits, lookup_auto=int(lookup is None), total_entries=total, chips=chip_blocks, buses=buses, positions=positions, entries=entries)


def words(rep):
    w = []

    def u64(v):
        w.extend([v & 0xFFFFFFFF, v >> 32])

    w += [0x314D4456, 0, rep["max_bits"], int(rep["total_entries"] > len(rep["entries"]))]
    u64(rep["total_entries"])
    w += [len(rep["entries"]), len(rep["chips"]), rep["lookup_auto"], len(rep["buses"]), len(rep["positions"]), 0]
    for c in rep["chips"]:
        w += [c["width"], c["constraints"], c["interactions"], c["audited"]]
        u64(c["height"])
        w += [c["is_table"], c["narrow"], c["entries"], c["appearances"]]
        if not c["audited"]:
            w += [0] * (24 * c["width"])
        for k in c["cols"]:
            w += [k["min"], k["max"], k["distinct"], k["cls"], k["dense"], k["bits"], k["narrow"], k["n_app"]]
            for key in ("nonzero", "wide", "guarded", "sent", "received", "unguarded", "ungnz", "mixed"):
                u64(k[key])
    for b in rep["buses"]:
        w += list(b)
    for p in rep["positions"]:
        w += [p["bus"], p["position"], p["is_send"], p["lookup"], p["min"], p["max"], p["distinct"], 0]
        u64(p["wide"])
        u64(p["records"])
    for e in rep["entries"]:
        w += [e["chip"], e["column"], e["cls"], e["max"], len(e["apps"]), len(e["rows"])]
        u64(e["ungnz"])
        for a in e["apps"]:
            w += [a["interaction"], a["position"], a["is_send"], a["is_global"], a["bus_index"], a["lookup"]]
            u64(a["live"])
        for r, v in e["rows"]:
            w += [r, v]
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
