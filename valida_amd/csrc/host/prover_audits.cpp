// The device passes of the nine witness audits: Prover::*_audit (see prover.hpp and each host/*_audit.hpp).  The plumbing they share is
// audit_pass.hpp; what follows per audit is its own scratch layout, its launches in order and the decoding of what it lists.
#include "audit_pass.hpp"

namespace vhost {

// ---- bus audit (host/bus_audit.hpp; kernels/bus_audit.hip) ------------------------------------------------------------------------------
BusReport Prover::bus_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed, const BusAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const BusAuditOpts o = bus_audit_checked_opts(opts_in);
    const auto tr = audit_traces<BusShape>("bus_audit", main, preprocessed);
    std::vector<int> prep_slot;
    BusPlan plan = bus_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, prep_slot);
    const uint64_t n = plan.n_slots;
    if (n >= 0xffffffffull) throw std::invalid_argument("bus_audit: more than 2^32 - 2 (row, interaction) pairs; record ids are 32-bit");

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const size_t NC = machine_.airs.size(), NB = plan.buses.size();
    const hipStream_t st = pass.stream;

    BusReport rep;
    rep.buses = plan.buses;
    audit_or_no_memory(st, [&] {
        // working-layout copies, as prove makes them (traces generated on the device are already column-major Montgomery)
        std::vector<const uint32_t*> mptr(NC, nullptr), pptr(NC, nullptr);
        std::vector<uint64_t> mstride(NC, 0), pstride(NC, 0);
        pass.begin();
        for (size_t i = 0; i < NC; i++) {
            if (!plan.chips[i].M) continue;  // a chip without interactions is not read
            const vk::DMatView v = pass.working(main[i]);
            mptr[i] = v.data; mstride[i] = v.stride;
            if (prep_slot[i] >= 0) { const vk::DMatView pv = pass.working(preprocessed[(size_t)prep_slot[i]].second); pptr[i] = pv.data; pstride[i] = pv.stride; }
        }
        c.check_launch("bus_audit ingest");
        DBuf desc(&c, bus_audit_descriptor(machine_, plan, mptr, mstride, pptr, pstride));

        uint32_t total_inter = 0;
        std::vector<uint32_t> inter_base(NC, 0);
        for (size_t i = 0; i < NC; i++) { inter_base[i] = total_inter; total_inter += plan.chips[i].M; }
        const size_t n_counters = 8 + NB + total_inter;
        const uint64_t na = n ? n : 1;
        DBuf keys2(&c, (size_t)(4 * na)), ids2(&c, (size_t)(2 * na)), cnt(&c, (size_t)na), gid(&c, (size_t)na), head_pos(&c, (size_t)na), sums(&c, (size_t)(4 * na)),
            nrec(&c, (size_t)(2 * na)), sort_tmp(&c, vk::bus_audit_sort_scratch_words(na)), scan_tmp(&c, vk::bus_audit_scan_scratch_words(na)), counters(&c, n_counters);
        unsigned long long* keys = (unsigned long long*)keys2.data;
        unsigned long long* sums_p = (unsigned long long*)sums.data;
        VG_HIP_CHECK(hipMemsetAsync(counters.data, 0, n_counters * 4, st));
        VG_HIP_CHECK(hipMemsetAsync(sums.data, 0, (size_t)(4 * na) * 4, st));
        VG_HIP_CHECK(hipMemsetAsync(nrec.data, 0, (size_t)(2 * na) * 4, st));

        for (size_t i = 0; i < NC; i++)
            vk::launch_ba_records(st, desc.data, (uint32_t)i, plan.chips[i].height, machine_.airs[i].width, plan.chips[i].M, o.hash_bits, keys, ids2.data, cnt.data,
                                  counters.data + 8 + NB + inter_base[i]);
        int shifts[8], n_shifts = 0;
        for (uint32_t b = 0; b < (o.hash_bits + 7) / 8; b++) shifts[n_shifts++] = 8 * (int)b;
        if (o.hash_bits <= 56) shifts[n_shifts++] = 56;  // the pass that sinks the dead slots (key ~0) behind the live ones
        int half = vk::launch_ba_sort(st, keys, ids2.data, n, sort_tmp.data, shifts, n_shifts, 0);
        vk::launch_ba_groups(st, desc.data, keys + (uint64_t)half * n, ids2.data + (uint64_t)half * n, n, false, gid.data, head_pos.data, scan_tmp.data, counters.data);
        vk::launch_ba_reduce(st, desc.data, ids2.data + (uint64_t)half * n, cnt.data, gid.data, head_pos.data, n, true, sums_p, nrec.data, counters.data);
        vk::launch_ba_select(st, desc.data, ids2.data + (uint64_t)half * n, head_pos.data, sums_p, n, false, 0, nullptr, nullptr, counters.data);
        c.check_launch("bus_audit");
        std::vector<uint32_t> cw(n_counters);
        c.download_small(cw.data(), counters.data, n_counters * 4);

        if (cw[2]) {
            // a key collision (with 64 key bits: practically never; the hash_bits test hook forces it): group by the full padded tuples instead.
            // Words [bus slot, field 0, ..]: two per radix sort, least significant pair first; the sorts are stable, ids start ascending.
            VG_HIP_CHECK(hipMemsetAsync(counters.data + 1, 0, (7 + NB) * 4, st));
            VG_HIP_CHECK(hipMemsetAsync(sums.data, 0, (size_t)(4 * na) * 4, st));
            VG_HIP_CHECK(hipMemsetAsync(nrec.data, 0, (size_t)(2 * na) * 4, st));
            const int all[8] = {0, 8, 16, 24, 32, 40, 48, 56};
            half = 0;
            vk::launch_ba_iota(st, ids2.data, n);
            for (int chunk = (int)(plan.wmax + 1 + 1) / 2 - 1; chunk >= 0; chunk--) {
                vk::launch_ba_rekey(st, desc.data, (uint32_t)chunk, ids2.data + (uint64_t)half * n, cnt.data, keys + (uint64_t)half * n, n);
                half = vk::launch_ba_sort(st, keys, ids2.data, n, sort_tmp.data, all, 8, half);
            }
            vk::launch_ba_groups(st, desc.data, keys + (uint64_t)half * n, ids2.data + (uint64_t)half * n, n, true, gid.data, head_pos.data, scan_tmp.data, counters.data);
            vk::launch_ba_reduce(st, desc.data, ids2.data + (uint64_t)half * n, cnt.data, gid.data, head_pos.data, n, false, sums_p, nrec.data, counters.data);
            vk::launch_ba_select(st, desc.data, ids2.data + (uint64_t)half * n, head_pos.data, sums_p, n, false, 0, nullptr, nullptr, counters.data);
            c.check_launch("bus_audit exact");
            c.download_small(cw.data(), counters.data, n_counters * 4);
        }
        const uint32_t n_unb = cw[3];
        rep.total_unbalanced = n_unb;
        for (size_t b = 0; b < NB; b++) rep.buses[b].unbalanced = cw[8 + b];
        for (size_t i = 0; i < NC; i++)
            for (uint32_t m = 0; m < plan.chips[i].M; m++) {
                BusStat& b = rep.buses[plan.chips[i].bus_slot[m]];
                const uint64_t live = cw[8 + NB + inter_base[i] + m];
                b.live += live;
                (machine_.airs[i].interactions[m].is_send() ? b.sends : b.receives) += live;
            }
        if (n_unb) {
            const uint32_t n_rep = (uint32_t)std::min<uint64_t>(n_unb, o.max_tuples), R = o.max_records_per_tuple, stride = 8 + plan.wmax + 2 * R;
            DBuf ukeys(&c, (size_t)4 * n_unb), uvals(&c, (size_t)2 * n_unb), out(&c, (size_t)n_rep * stride);
            vk::launch_ba_select(st, desc.data, ids2.data + (uint64_t)half * n, head_pos.data, sums_p, cw[1], true, n_unb, (unsigned long long*)ukeys.data, uvals.data, counters.data);
            const int id_bytes[4] = {0, 8, 16, 24};  // keys are 32-bit record ids
            const int uh = vk::launch_ba_sort(st, (unsigned long long*)ukeys.data, uvals.data, n_unb, sort_tmp.data, id_bytes, 4, 0);
            vk::launch_ba_report(st, desc.data, ids2.data + (uint64_t)half * n, cnt.data, head_pos.data, sums_p, nrec.data, uvals.data + (uint64_t)uh * n_unb, n_rep, R, out.data);
            c.check_launch("bus_audit report");
            std::vector<uint32_t> w((size_t)n_rep * stride);
            c.download_small(w.data(), out.data, w.size() * 4);
            for (uint32_t t = 0; t < n_rep; t++) {
                const uint32_t* e = w.data() + (size_t)t * stride;
                const BusStat& bus = plan.buses.at(e[0]);
                BusTuple bt;
                bt.is_global = bus.is_global; bt.bus_index = bus.bus_index;
                bt.fields.assign(e + 8, e + 8 + bus.width);
                bt.send_sum = (uint32_t)((((uint64_t)e[3] << 32) | e[2]) % vg::P);
                bt.recv_sum = (uint32_t)((((uint64_t)e[5] << 32) | e[4]) % vg::P);
                bt.net = (bt.send_sum + vg::P - bt.recv_sum) % vg::P;
                bt.n_send = e[6]; bt.n_recv = e[7];
                for (uint32_t k = 0; k < e[1] && k < R; k++) {
                    BusRecord r = plan.decode(e[8 + plan.wmax + 2 * k]);
                    r.is_send = machine_.airs[r.chip].interactions[r.interaction].is_send() ? 1u : 0u;
                    r.count = e[8 + plan.wmax + 2 * k + 1];
                    bt.records.push_back(r);
                }
                rep.tuples.push_back(std::move(bt));
            }
        }
        pass.end(rep);
    }, [&] {
        return std::string("bus_audit: the device pool cannot give the pass its scratch: " + std::to_string(BUS_AUDIT_BYTES_PER_SLOT) + " bytes for each of the " +
                           std::to_string(n) + " (row, interaction) pairs, 24 more per unbalanced tuple, plus the working-layout copies of uploaded traces");
    });
    bus_audit_finish(rep, o);
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- constraint audit (host/constraint_audit.hpp; kernels/constraint_audit.hip) ------------------------------------------------------------
ConstraintReport Prover::constraint_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed,
                                          const ConstraintAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const ConstraintAuditOpts o = constraint_audit_checked_opts(opts_in);
    const auto tr = audit_traces<ConstraintShape>("constraint_audit", main, preprocessed);
    std::vector<int> prep_slot;
    constraint_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, prep_slot);
    const size_t NC = machine_.airs.size();
    for (auto& air : machine_.airs) audit_refuse_constraints("constraint_audit", air);

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const hipStream_t st = pass.stream;

    ConstraintReport rep;
    rep.chips.resize(NC);
    uint64_t scratch_words = 0;
    audit_or_no_memory(st, [&] {
        // per chip: the launch shape and its slice of the scratch (u32 words): totals [2 (K + 1)], table [K NB], prefix [K NB]
        std::vector<vk::CaArgs> args(NC);
        AuditScratch sc(NC);
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine_.airs[i];
            vk::CaArgs& a = args[i];
            a = vk::CaArgs{};
            rep.chips[i].n_constraints = air.program.num_asserts; rep.chips[i].height = main[i]->height;
            if (!air.program.num_asserts) continue;  // a chip without constraints (program, mem, div, range) is not read
            audit_chip_sizes(a, air, main[i]->height, fri_.interpret_air);
            pass.bind(a, main[i], audit_prep(preprocessed, prep_slot, i), prog_dev_[i]);
            a.T = vk::ca_block_threads(a);
            a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
            sc.add(i, 2 * (uint64_t)(a.K + 1), (uint64_t)a.K * a.NB);
        }
        scratch_words = sc.place_prefixes();
        c.check_launch("constraint_audit ingest");
        DBuf scratch(&c, (size_t)(scratch_words ? scratch_words : 1));
        // the device pass: everything from here to the last download is between the two events (the working-layout copies of uploaded traces,
        // which a proof makes as well, are before them)
        pass.begin();
        if (sc.zeroed) VG_HIP_CHECK(hipMemsetAsync(scratch.data, 0, (size_t)sc.zeroed * 4, st));
        for (size_t i = 0; i < NC; i++)
            if (args[i].K) vk::launch_ca_count(st, args[i], reinterpret_cast<unsigned long long*>(scratch.data + sc.tot_at[i]), scratch.data + sc.tab_at[i]);
        c.check_launch("constraint_audit count");
        // the totals of all chips lie in front of their tables: gather them with one small copy per chip
        std::vector<std::vector<uint64_t>> counts(NC);
        {
            std::vector<uint32_t> tw;
            for (size_t i = 0; i < NC; i++) {
                const uint32_t K = args[i].K;
                counts[i].assign(K, 0);
                if (!K) continue;
                tw.resize(2 * (size_t)(K + 1));
                c.download_small(tw.data(), scratch.data + sc.tot_at[i], tw.size() * 4);
                for (uint32_t k = 0; k < K; k++) counts[i][k] = audit_u64(tw, k);
                rep.chips[i].failing_rows = audit_u64(tw, K);
            }
        }
        constraint_audit_finish(rep, counts, o);
        const uint32_t R = o.max_rows_per_constraint;
        audit_chip_runs(rep.constraints, [&](uint32_t chip, size_t e0, size_t e1) {
            // the listed constraints of one chip: scan, list, values, one download
            vk::CaListed listed{};
            for (size_t e = e0; e < e1; e++) { const uint32_t k = rep.constraints[e].constraint; listed.w[k >> 5] |= 1u << (k & 31u); }
            const vk::CaArgs& a = args[chip];
            DBuf out(&c, (size_t)2 * a.K * R);
            uint32_t* rows = out.data;
            uint32_t* values = out.data + (size_t)a.K * R;
            vk::launch_ca_scan(st, a, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], listed);
            vk::launch_ca_list(st, a, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], listed, R, rows);
            vk::launch_ca_values(st, a, reinterpret_cast<const unsigned long long*>(scratch.data + sc.tot_at[chip]), listed, R, rows, values);
            c.check_launch("constraint_audit list");
            std::vector<uint32_t> w((size_t)2 * a.K * R);
            c.download_small(w.data(), out.data, w.size() * 4);
            for (size_t e = e0; e < e1; e++) {
                ConstraintEntry& en = rep.constraints[e];
                const uint64_t listed_rows = std::min<uint64_t>(en.failing_rows, R);
                for (uint64_t j = 0; j < listed_rows; j++) en.rows.push_back({w[(size_t)en.constraint * R + j], w[(size_t)a.K * R + (size_t)en.constraint * R + j]});
            }
        });
        pass.end(rep);
    }, [&] {
        return std::string("constraint_audit: the device pool cannot give the pass its scratch: 8 bytes per (constraint, workgroup of 256 rows) of every chip (" +
                           std::to_string(scratch_words * 4) + " bytes for this witness), 8 more per listed row, plus the working-layout copies of uploaded traces");
    });
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- mutation audit (host/mutation_audit.hpp; kernels/mutation_audit.hip) ------------------------------------------------------------------
MutationReport Prover::mutation_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed,
                                      const MutationAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const MutationAuditOpts o = mutation_audit_checked_opts(opts_in);
    const auto tr = audit_traces<ConstraintShape>("mutation_audit", main, preprocessed);
    std::vector<int> prep_slot;
    mutation_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, prep_slot);
    const size_t NC = machine_.airs.size();
    for (auto& air : machine_.airs) audit_refuse_constraints("mutation_audit", air);
    const uint32_t D = o.n_deltas, R = o.max_rows_per_entry;

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const hipStream_t st = pass.stream;

    MutationReport rep;
    rep.chips.resize(NC);
    uint64_t scratch_words = 0, rows_words = 0;
    audit_or_no_memory(st, [&] {
        // per chip: the launch shape, its column flags and its slice of the scratch (u32 words): totals [6 E], table [E NB], prefix [E NB]
        std::vector<vk::MaArgs> args(NC);
        AuditScratch sc(NC);
        std::vector<uint64_t> flag_at(NC, 0);
        std::vector<uint32_t> flag_words;
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine_.airs[i];
            vk::MaArgs& a = args[i];
            a = vk::MaArgs{};
            rep.chips[i].width = air.width; rep.chips[i].n_constraints = air.program.num_asserts; rep.chips[i].height = main[i]->height;
            const double evaluations = ma_evaluations(air, main[i]->height, D);
            rep.evaluations += evaluations;
            if (!air.width) continue;
            audit_chip_sizes(a, air, main[i]->height, fri_.interpret_air);
            pass.bind(a, main[i], audit_prep(preprocessed, prep_slot, i), prog_dev_[i]);
            a.iw = iw_dev_[i].data;
            a.evaluations = evaluations;
            a.D = D;
            for (uint32_t k = 0; k < D; k++) a.delta[k] = Fp::from_canonical(o.deltas[k]).v;
            a.T = vk::ma_block_threads(a);
            a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
            a.CY = vk::ma_column_slices(a, a.NB);
            const double baselines = a.K ? (a.n == 1 ? 1.0 : 2.0) * (double)a.n * (a.CY - 1) : 0;  // every column slice evaluates the baselines of its rows
            a.evaluations += baselines; rep.evaluations += baselines;
            const std::vector<uint32_t> fl = ma_column_flags(air);
            bool masks_ok = false;
            const std::vector<uint32_t> bm = ma_bus_masks(air, masks_ok);
            a.bus_walk = masks_ok ? 0u : 1u;
            flag_at[i] = flag_words.size();
            flag_words.insert(flag_words.end(), fl.begin(), fl.end());
            flag_words.insert(flag_words.end(), bm.begin(), bm.end());
            const uint64_t E = (uint64_t)a.width * D;
            sc.add(i, 6 * E, E * a.NB);
            rows_words = std::max<uint64_t>(rows_words, E * R);
        }
        scratch_words = sc.place_prefixes();
        if (flag_words.empty()) flag_words.push_back(0);
        DBuf flags(&c, flag_words);
        for (size_t i = 0; i < NC; i++) args[i].flags = flags.data + flag_at[i];
        c.check_launch("mutation_audit ingest");
        DBuf scratch(&c, (size_t)(scratch_words ? scratch_words : 1));
        DBuf out(&c, (size_t)(rows_words ? rows_words : 1));
        // the device pass: everything from here to the last download is between the two events (the working-layout copies of uploaded traces,
        // which a proof makes as well, are before them)
        pass.begin();
        if (sc.zeroed) VG_HIP_CHECK(hipMemsetAsync(scratch.data, 0, (size_t)sc.zeroed * 4, st));
        for (size_t i = 0; i < NC; i++)
            if (args[i].width) vk::launch_ma_count(st, args[i], reinterpret_cast<unsigned long long*>(scratch.data + sc.tot_at[i]), scratch.data + sc.tab_at[i]);
        c.check_launch("mutation_audit count");
        std::vector<std::vector<uint64_t>> counts(NC);
        {
            std::vector<uint32_t> tw;
            for (size_t i = 0; i < NC; i++) {
                const size_t E = (size_t)args[i].width * D;
                counts[i].assign(3 * E, 0);
                if (!E) continue;
                tw.resize(6 * E);
                c.download_small(tw.data(), scratch.data + sc.tot_at[i], tw.size() * 4);
                for (size_t k = 0; k < 3 * E; k++) counts[i][k] = audit_u64(tw, k);
            }
        }
        mutation_audit_finish(rep, counts, o);
        audit_chip_runs(rep.entries, [&](uint32_t chip, size_t e0, size_t e1) {
            // the listed entries of one chip: scan, list, one download
            const vk::MaArgs& a = args[chip];
            const uint32_t e_cut = rep.entries[e1 - 1].column * D + rep.entries[e1 - 1].delta + 1;  // entries ascend: the listed ones of a chip are a prefix
            vk::launch_ma_scan(st, a, reinterpret_cast<const unsigned long long*>(scratch.data + sc.tot_at[chip]), scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], e_cut);
            vk::launch_ma_list(st, a, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], e_cut, R, out.data);
            c.check_launch("mutation_audit list");
            std::vector<uint32_t> w((size_t)e_cut * R);
            c.download_small(w.data(), out.data, w.size() * 4);
            for (size_t e = e0; e < e1; e++) {
                MutationEntry& en = rep.entries[e];
                const uint64_t listed = std::min<uint64_t>(en.free_, R);
                const size_t at = ((size_t)en.column * D + en.delta) * R;
                en.rows.assign(w.begin() + at, w.begin() + at + listed);
            }
        });
        pass.end(rep);
    }, [&] {
        return std::string("mutation_audit: the device pool cannot give the pass its scratch: 8 bytes per (column, delta, workgroup of rows) and 24 per (column, delta) of every chip (" +
                           std::to_string(scratch_words * 4) + " bytes for this witness), " + std::to_string(rows_words * 4) + " bytes of listed rows (4 x columns x deltas x max_rows_per_entry of the widest chip), plus the working-layout copies of uploaded traces");
    });
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- pair audit (host/pair_audit.hpp; kernels/pair_audit.hip) ------------------------------------------------------------------------------
PairReport Prover::pair_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed, const PairAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const PairAuditOpts o = pair_audit_checked_opts(opts_in, machine_.airs.size());
    const auto tr = audit_traces<ConstraintShape>("pair_audit", main, preprocessed);
    std::vector<int> prep_slot;
    pair_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, prep_slot);
    const size_t NC = machine_.airs.size();
    for (size_t i = 0; i < NC; i++) {
        if (!pair_audit_selected(o, i)) continue;
        audit_refuse_constraints("pair_audit", machine_.airs[i]);
        if (machine_.airs[i].width > 4096)
            throw std::invalid_argument("pair_audit: chip " + machine_.airs[i].name + " has more than 4096 columns; the device audit handles up to 4096 (the host audit up to 65535)");
    }
    const uint32_t D = o.n_deltas, DD = D * D, R = o.max_rows_per_entry;

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const hipStream_t st = pass.stream;

    PairReport rep;
    rep.chips.resize(NC);
    uint64_t scratch_words = 0, rows_words = 0, desc_words_n = 0;
    audit_or_no_memory(st, [&] {
        // per chip: the launch shape, its descriptor words (column flags and bus masks, the coupled pairs, the pairs' bus masks) and its slice
        // of the scratch (u32 words): totals, table [E NB], prefix [E NB]
        std::vector<vk::PaArgs> args(NC);
        std::vector<std::vector<uint32_t>> pairs(NC);
        AuditScratch sc(NC);
        std::vector<uint64_t> flag_at(NC, 0), pair_at(NC, 0), mask_at(NC, 0);
        std::vector<uint32_t> desc_words;
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine_.airs[i];
            vk::PaArgs& v = args[i];
            v = vk::PaArgs{};
            vk::MaArgs& a = v.m;
            PairChipStat& cs = rep.chips[i];
            cs.width = air.width; cs.n_constraints = air.program.num_asserts; cs.n_interactions = (uint32_t)air.interactions.size(); cs.height = main[i]->height;
            cs.audited = pair_audit_selected(o, i) ? 1u : 0u;
            if (!cs.audited || !air.width) continue;
            audit_chip_sizes(a, air, main[i]->height, fri_.interpret_air);
            pass.bind(a, main[i], audit_prep(preprocessed, prep_slot, i), prog_dev_[i]);
            a.iw = iw_dev_[i].data;
            a.D = D;
            for (uint32_t k = 0; k < D; k++) a.delta[k] = Fp::from_canonical(o.deltas[k]).v;
            pairs[i] = pa_coupled_pairs(air, a.n);
            v.P = (uint32_t)pairs[i].size();
            vk::pa_shape(v);
            a.evaluations = pa_device_evaluations(air, a.n, D, pairs[i], v.PPS, a.CY);
            rep.evaluations += a.evaluations;
            const std::vector<uint32_t> fl = ma_column_flags(air);
            bool masks_ok = false;
            const std::vector<uint32_t> bm = ma_bus_masks(air, masks_ok);
            const std::vector<uint32_t> pmk = pa_bus_masks(air, pairs[i], o.deltas, D, masks_ok);
            a.bus_walk = masks_ok ? 0u : 1u;
            flag_at[i] = desc_words.size();
            desc_words.insert(desc_words.end(), fl.begin(), fl.end());
            desc_words.insert(desc_words.end(), bm.begin(), bm.end());
            pair_at[i] = desc_words.size();
            desc_words.insert(desc_words.end(), pairs[i].begin(), pairs[i].end());
            desc_words.push_back(0);
            mask_at[i] = desc_words.size();
            desc_words.insert(desc_words.end(), pmk.begin(), pmk.end());
            sc.add(i, vk::pa_totals_words(v), (uint64_t)v.P * DD * a.NB);
        }
        scratch_words = sc.place_prefixes();
        if (desc_words.empty()) desc_words.push_back(0);
        desc_words_n = desc_words.size();
        DBuf desc(&c, desc_words);
        for (size_t i = 0; i < NC; i++) { args[i].m.flags = desc.data + flag_at[i]; args[i].pairs = desc.data + pair_at[i]; args[i].pmasks = desc.data + mask_at[i]; }
        c.check_launch("pair_audit ingest");
        DBuf scratch(&c, (size_t)(scratch_words ? scratch_words : 1));
        // the device pass: everything from here to the last download is between the two events
        pass.begin();
        if (sc.zeroed) VG_HIP_CHECK(hipMemsetAsync(scratch.data, 0, (size_t)sc.zeroed * 4, st));
        for (size_t i = 0; i < NC; i++)
            if (args[i].m.width) vk::launch_pa_count(st, args[i], reinterpret_cast<unsigned long long*>(scratch.data + sc.tot_at[i]), scratch.data + sc.tab_at[i]);
        c.check_launch("pair_audit count");
        std::vector<std::vector<uint64_t>> counts(NC), ufree(NC);
        {
            std::vector<uint32_t> tw;
            for (size_t i = 0; i < NC; i++) {
                const size_t E = (size_t)args[i].P * DD;
                counts[i].assign(2 * E, 0);
                ufree[i].assign(DD, 0);
                if (!args[i].m.width) continue;
                tw.resize(vk::pa_totals_words(args[i]));
                c.download_small(tw.data(), scratch.data + sc.tot_at[i], tw.size() * 4);
                for (size_t k = 0; k < 2 * E; k++) counts[i][k] = audit_u64(tw, k);
                for (uint32_t q = 0; q < DD; q++) ufree[i][q] = audit_u64(tw, 2 * E + q) - audit_u64(tw, 2 * E + 16 + q);  // all pairs - coupled pairs: both singles free
            }
        }
        pair_audit_finish(rep, pairs, counts, ufree, o);
        // entry index of a listed entry within its chip: its pair's position in the coupled list
        auto entry_index = [&](const PairEntry& en) {
            const auto& pl = pairs[en.chip];
            size_t lo = 0, hi = pl.size();
            while (lo < hi) {  // ascending (c1, c2)
                const size_t mid = (lo + hi) / 2;
                const uint32_t m1 = pl[mid] & 0xffffu, m2 = pl[mid] >> 16;
                if (m1 < en.c1 || (m1 == en.c1 && m2 < en.c2)) lo = mid + 1; else hi = mid;
            }
            return (uint64_t)lo * DD + en.q;
        };
        audit_chip_runs(rep.entries, [&](uint32_t, size_t, size_t e1) {
            rows_words = std::max<uint64_t>(rows_words, (entry_index(rep.entries[e1 - 1]) + 1) * R);
        });
        DBuf out(&c, (size_t)(rows_words ? rows_words : 1));
        audit_chip_runs(rep.entries, [&](uint32_t chip, size_t e0, size_t e1) {
            // the listed entries of one chip: scan, list, one download
            const vk::PaArgs& v = args[chip];
            const uint32_t e_cut = (uint32_t)(entry_index(rep.entries[e1 - 1]) + 1);  // entries ascend: the listed ones of a chip are below it
            vk::launch_pa_scan(st, v, reinterpret_cast<const unsigned long long*>(scratch.data + sc.tot_at[chip]), scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], e_cut);
            vk::launch_pa_list(st, v, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], e_cut, R, out.data);
            c.check_launch("pair_audit list");
            std::vector<uint32_t> w((size_t)e_cut * R);
            c.download_small(w.data(), out.data, w.size() * 4);
            for (size_t e = e0; e < e1; e++) {
                PairEntry& en = rep.entries[e];
                const uint64_t listed = std::min<uint64_t>(en.compensated, R);
                const size_t at = (size_t)entry_index(en) * R;
                en.rows.assign(w.begin() + at, w.begin() + at + listed);
            }
        });
        pass.end(rep);
    }, [&] {
        return std::string("pair_audit: the device pool cannot give the pass its scratch: 16 bytes per (coupled pair, delta pair) and 8 per (coupled pair, delta pair, workgroup of rows) of every chip (" +
                           std::to_string(scratch_words * 4) + " bytes for this witness), " + std::to_string(desc_words_n * 4) + " bytes of pair lists and bus masks, " + std::to_string(rows_words * 4) +
                           " bytes of listed rows, plus the working-layout copies of uploaded traces; chip_mask audits fewer chips at a time");
    });
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- rank audit (host/rank_audit.hpp; kernels/rank_audit.hip) ------------------------------------------------------------------------------
RankReport Prover::rank_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed, const RankAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const RankAuditOpts o = rank_audit_checked_opts(opts_in, machine_.airs.size());
    const auto tr = audit_traces<ConstraintShape>("rank_audit", main, preprocessed);
    std::vector<int> prep_slot;
    rank_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, prep_slot);
    const size_t NC = machine_.airs.size();
    const uint32_t R = o.max_rows_per_entry;
    // per chip its launch shape: a chip that does not fit the LDS is refused before anything is queued
    std::vector<vk::RaArgs> args(NC);
    RankReport rep;
    rep.chips.resize(NC);
    for (size_t i = 0; i < NC; i++) {
        const AirDesc& air = machine_.airs[i];
        vk::RaArgs& a = args[i];
        a = vk::RaArgs{};
        RankChipStat& cs = rep.chips[i];
        cs.width = air.width; cs.n_constraints = air.program.num_asserts; cs.n_interactions = (uint32_t)air.interactions.size(); cs.height = main[i]->height;
        cs.audited = rank_audit_selected(o, i) ? 1u : 0u;
        cs.loose.assign(air.width, 0); cs.zeros.assign(air.width, 0);
        if (!cs.audited || !air.width) continue;
        audit_chip_sizes(a, air, main[i]->height, fri_.interpret_air);
        audit_chip_shape(air, [&] { vk::ra_shape(a); });
        a.evaluations = a.K ? (double)a.n * a.width * (a.n == 1 ? 1 : 2) : 0;
        rep.evaluations += a.evaluations;
    }

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const hipStream_t st = pass.stream;

    uint64_t scratch_words = 0, rows_words = 0, desc_words_n = 0;
    audit_or_no_memory(st, [&] {
        // per chip: its weight rows and its slice of the scratch (u32 words): totals, table [w NB], prefix [w NB]
        AuditScratch sc(NC);
        std::vector<uint64_t> wr_at(NC, 0);
        std::vector<uint32_t> desc_words;
        for (size_t i = 0; i < NC; i++) {
            vk::RaArgs& a = args[i];
            if (!a.width) continue;
            pass.bind(a, main[i], audit_prep(preprocessed, prep_slot, i), prog_dev_[i]);
            a.iw = iw_dev_[i].data;
            const std::vector<uint32_t> wr = ra_weight_rows(machine_.airs[i]);
            wr_at[i] = desc_words.size();
            desc_words.insert(desc_words.end(), wr.begin(), wr.end());
            sc.add(i, vk::ra_totals_words(a), (uint64_t)a.width * a.NB);
        }
        scratch_words = sc.place_prefixes();
        if (desc_words.empty()) desc_words.push_back(0);
        desc_words_n = desc_words.size();
        DBuf desc(&c, desc_words);
        for (size_t i = 0; i < NC; i++) args[i].wr = desc.data + wr_at[i];
        c.check_launch("rank_audit ingest");
        DBuf scratch(&c, (size_t)(scratch_words ? scratch_words : 1));
        // the device pass: everything from here to the last download is between the two events
        pass.begin();
        if (sc.zeroed) VG_HIP_CHECK(hipMemsetAsync(scratch.data, 0, (size_t)sc.zeroed * 4, st));
        for (size_t i = 0; i < NC; i++)
            if (args[i].width) vk::launch_ra_count(st, args[i], reinterpret_cast<unsigned long long*>(scratch.data + sc.tot_at[i]), scratch.data + sc.tab_at[i]);
        c.check_launch("rank_audit count");
        {
            std::vector<uint32_t> tw;
            for (size_t i = 0; i < NC; i++) {
                if (!args[i].width) continue;
                RankChipStat& cs = rep.chips[i];
                tw.resize(vk::ra_totals_words(args[i]));
                c.download_small(tw.data(), scratch.data + sc.tot_at[i], tw.size() * 4);
                auto u64 = [&](size_t k) { return audit_u64(tw, k); };
                cs.nullity = u64(0); cs.zero = u64(1); cs.coupled_rows = u64(2); cs.max_nullity = (uint32_t)u64(3);
                for (uint32_t k = 0; k < cs.width; k++) { cs.loose[k] = u64(4 + 2 * (size_t)k); cs.zeros[k] = u64(5 + 2 * (size_t)k); }
            }
        }
        rank_audit_finish(rep, o);
        audit_chip_runs(rep.entries, [&](uint32_t, size_t, size_t e1) {
            rows_words = std::max<uint64_t>(rows_words, ((uint64_t)rep.entries[e1 - 1].column + 1) * R * RA_ROW_WORDS);
        });
        DBuf out(&c, (size_t)(rows_words ? rows_words : 1));
        audit_chip_runs(rep.entries, [&](uint32_t chip, size_t e0, size_t e1) {
            // the listed columns of one chip: scan, list, one download
            const vk::RaArgs& a = args[chip];
            const uint32_t c_cut = rep.entries[e1 - 1].column + 1;  // entries ascend: the listed columns of a chip are below it
            const size_t words = (size_t)c_cut * R * RA_ROW_WORDS;
            VG_HIP_CHECK(hipMemsetAsync(out.data, 0, words * 4, st));  // unused term slots are zero
            vk::launch_ra_scan(st, a, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], c_cut);
            vk::launch_ra_list(st, a, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], c_cut, R, out.data);
            c.check_launch("rank_audit list");
            std::vector<uint32_t> w(words);
            c.download_small(w.data(), out.data, w.size() * 4);
            for (size_t e = e0; e < e1; e++) {
                RankEntry& en = rep.entries[e];
                const uint64_t listed = std::min<uint64_t>(en.coupled, R);
                en.rows.resize((size_t)listed);
                for (size_t k = 0; k < listed; k++) {
                    const uint32_t* src = w.data() + ((size_t)en.column * R + k) * RA_ROW_WORDS;
                    en.rows[k].row = src[0]; en.rows[k].n_support = src[1];
                    for (uint32_t x = 0; x < 2 * RA_TERMS; x++) en.rows[k].terms[x] = src[2 + x];
                }
            }
        });
        pass.end(rep);
    }, [&] {
        return std::string("rank_audit: the device pool cannot give the pass its scratch: 32 + 16 bytes per column of totals and 8 per (column, workgroup of rows) of every chip (" +
                           std::to_string(scratch_words * 4) + " bytes for this witness), " + std::to_string(desc_words_n * 4) + " bytes of interaction weight rows, " + std::to_string(rows_words * 4) +
                           " bytes of listed rows (72 per (listed column, row slot)), plus the working-layout copies of uploaded traces; chip_mask audits fewer chips at a time");
    });
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- step audit (host/step_audit.hpp; kernels/step_audit.hip) ------------------------------------------------------------------------------
StepReport Prover::step_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed, const StepAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const StepAuditOpts o = step_audit_checked_opts(opts_in, machine_.airs.size());
    const auto tr = audit_traces<ConstraintShape>("step_audit", main, preprocessed);
    std::vector<int> prep_slot;
    step_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, prep_slot);
    const size_t NC = machine_.airs.size();
    const uint32_t R = o.max_rows_per_entry;
    // per chip its launch shape: a chip that does not fit the LDS is refused before anything is queued
    std::vector<vk::SaArgs> sargs(NC);
    StepReport rep;
    rep.chips.resize(NC);
    for (size_t i = 0; i < NC; i++) {
        const AirDesc& air = machine_.airs[i];
        sargs[i] = vk::SaArgs{};
        vk::RaArgs& a = sargs[i].r;
        sargs[i].n_steps = o.n_steps;
        for (uint32_t s = 0; s < SA_MAX_STEPS; s++) sargs[i].steps[s] = vg::Fp::from_canonical(o.steps[s]).v;
        StepChipStat& cs = rep.chips[i];
        step_audit_chip_block(cs, air, main[i]->height, step_audit_selected(o, i), o.n_steps);
        if (!cs.audited || !air.width) continue;
        audit_chip_sizes(a, air, main[i]->height, fri_.interpret_air);
        audit_chip_shape(air, [&] { vk::sa_shape(sargs[i]); });
        // dual evaluations, and at most one plain evaluation per (column, step) and q
        a.evaluations = a.K ? (double)a.n * a.width * (a.n == 1 ? 1 : 2) * (1 + o.n_steps) : 0;
        rep.evaluations += a.evaluations;
    }

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const hipStream_t st = pass.stream;

    uint64_t scratch_words = 0, rows_words = 0, desc_words_n = 0;
    audit_or_no_memory(st, [&] {
        // per chip: its weight rows and its slice of the scratch (u32 words): totals, table [w NB], prefix [w NB]
        AuditScratch sc(NC);
        std::vector<uint64_t> wr_at(NC, 0);
        std::vector<uint32_t> desc_words;
        for (size_t i = 0; i < NC; i++) {
            vk::RaArgs& a = sargs[i].r;
            if (!a.width) continue;
            pass.bind(a, main[i], audit_prep(preprocessed, prep_slot, i), prog_dev_[i]);
            a.iw = iw_dev_[i].data;
            const std::vector<uint32_t> wr = ra_weight_rows(machine_.airs[i]);
            wr_at[i] = desc_words.size();
            desc_words.insert(desc_words.end(), wr.begin(), wr.end());
            sc.add(i, vk::sa_totals_words(sargs[i]), (uint64_t)a.width * a.NB);
        }
        scratch_words = sc.place_prefixes();
        if (desc_words.empty()) desc_words.push_back(0);
        desc_words_n = desc_words.size();
        DBuf desc(&c, desc_words);
        for (size_t i = 0; i < NC; i++) sargs[i].r.wr = desc.data + wr_at[i];
        c.check_launch("step_audit ingest");
        DBuf scratch(&c, (size_t)(scratch_words ? scratch_words : 1));
        // the device pass: everything from here to the last download is between the two events
        pass.begin();
        if (sc.zeroed) VG_HIP_CHECK(hipMemsetAsync(scratch.data, 0, (size_t)sc.zeroed * 4, st));
        for (size_t i = 0; i < NC; i++)
            if (sargs[i].r.width) vk::launch_sa_count(st, sargs[i], reinterpret_cast<unsigned long long*>(scratch.data + sc.tot_at[i]), scratch.data + sc.tab_at[i]);
        c.check_launch("step_audit count");
        {
            std::vector<uint32_t> tw;
            for (size_t i = 0; i < NC; i++) {
                if (!sargs[i].r.width) continue;
                StepChipStat& cs = rep.chips[i];
                tw.resize(vk::sa_totals_words(sargs[i]));
                c.download_small(tw.data(), scratch.data + sc.tot_at[i], tw.size() * 4);
                auto u64 = [&](size_t k) { return audit_u64(tw, k); };
                cs.confirmed_rows = u64(0); cs.refuted_rows = u64(1);
                for (uint32_t s = 0; s < SA_MAX_STEPS; s++) cs.passes[s] = u64(2 + s);
                for (uint32_t k = 0; k < cs.width; k++) {
                    cs.loose[k] = u64(6 + 4 * (size_t)k); cs.zeros[k] = u64(7 + 4 * (size_t)k); cs.exact[k] = u64(8 + 4 * (size_t)k); cs.coupled_exact[k] = u64(9 + 4 * (size_t)k);
                }
            }
        }
        step_audit_finish(rep, o);
        audit_chip_runs(rep.entries, [&](uint32_t, size_t, size_t e1) {
            rows_words = std::max<uint64_t>(rows_words, ((uint64_t)rep.entries[e1 - 1].column + 1) * R * SA_ROW_WORDS);
        });
        DBuf out(&c, (size_t)(rows_words ? rows_words : 1));
        audit_chip_runs(rep.entries, [&](uint32_t chip, size_t e0, size_t e1) {
            // the listed columns of one chip: scan, list, one download
            const vk::SaArgs& sa = sargs[chip];
            const uint32_t c_cut = rep.entries[e1 - 1].column + 1;  // entries ascend: the listed columns of a chip are below it
            const size_t words = (size_t)c_cut * R * SA_ROW_WORDS;
            VG_HIP_CHECK(hipMemsetAsync(out.data, 0, words * 4, st));  // unused term slots are zero
            vk::launch_ra_scan(st, sa.r, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], c_cut);
            vk::launch_sa_list(st, sa, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], c_cut, R, out.data);
            c.check_launch("step_audit list");
            std::vector<uint32_t> w(words);
            c.download_small(w.data(), out.data, w.size() * 4);
            for (size_t e = e0; e < e1; e++) {
                StepEntry& en = rep.entries[e];
                const uint64_t listed = std::min<uint64_t>(en.coupled_exact + en.curved, R);
                en.rows.resize((size_t)listed);
                for (size_t k = 0; k < listed; k++) {
                    const uint32_t* src = w.data() + ((size_t)en.column * R + k) * SA_ROW_WORDS;
                    en.rows[k].row = src[0]; en.rows[k].pass_mask = src[1]; en.rows[k].zero = src[2]; en.rows[k].n_support = src[3];
                    for (uint32_t x = 0; x < 2 * RA_TERMS; x++) en.rows[k].terms[x] = src[4 + x];
                }
            }
        });
        pass.end(rep);
    }, [&] {
        return std::string("step_audit: the device pool cannot give the pass its scratch: 48 + 32 bytes per column of totals and 8 per (column, workgroup of rows) of every chip (" +
                           std::to_string(scratch_words * 4) + " bytes for this witness), " + std::to_string(desc_words_n * 4) + " bytes of interaction weight rows, " + std::to_string(rows_words * 4) +
                           " bytes of listed rows (80 per (listed column, row slot)), plus the working-layout copies of uploaded traces; chip_mask audits fewer chips at a time");
    });
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- invariant audit (host/invariant_audit.hpp; kernels/invariant_audit.hip) -----------------------------------------------------------------
InvariantReport Prover::invariant_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed, const InvariantAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const InvariantAuditOpts o = invariant_audit_checked_opts(opts_in, machine_.airs.size());
    const auto tr = audit_traces<ConstraintShape>("invariant_audit", main, preprocessed);
    std::vector<int> prep_slot;
    invariant_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, prep_slot);
    const size_t NC = machine_.airs.size();
    const uint32_t R = o.max_rows_per_entry;
    // per chip its launch shapes: a chip that does not fit the LDS is refused before anything is queued (phase 2 with d = w, the most there can be)
    std::vector<vk::IaArgs> args(NC);
    InvariantReport rep;
    rep.chips.resize(NC);
    for (size_t i = 0; i < NC; i++) {
        const AirDesc& air = machine_.airs[i];
        args[i] = vk::IaArgs{};
        InvariantChipStat& cs = rep.chips[i];
        invariant_audit_chip_block(cs, air, main[i]->height, invariant_audit_selected(o, i));
        if (!cs.audited || !air.width) continue;
        audit_chip_sizes(args[i].r, air, main[i]->height, fri_.interpret_air);
        audit_chip_shape(air, [&] { vk::ia_basis_shape(args[i]); args[i].d = air.width; vk::ia_shape(args[i]); });
    }

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const hipStream_t st = pass.stream;

    uint64_t basis_words = 0, scratch_words = 0, rows_words = 0, desc_words_n = 0;
    audit_or_no_memory(st, [&] {
        // per chip: its weight rows and its slice of the basis scratch (u32 words): the workgroups' bases, the merged one
        std::vector<uint64_t> wr_at(NC, 0), part_at(NC, 0), inv_at(NC, 0);
        std::vector<size_t> e_at(NC + 1, 0);  // chip i's entries are [e_at[i], e_at[i + 1]) until the list is cut
        std::vector<uint32_t> desc_words;
        for (size_t i = 0; i < NC; i++) {
            vk::RaArgs& a = args[i].r;
            if (!a.width) continue;
            pass.bind(a, main[i], audit_prep(preprocessed, prep_slot, i), prog_dev_[i]);
            a.iw = iw_dev_[i].data;
            const std::vector<uint32_t> wr = ra_weight_rows(machine_.airs[i]);
            wr_at[i] = desc_words.size();
            desc_words.insert(desc_words.end(), wr.begin(), wr.end());
            part_at[i] = basis_words; basis_words += vk::ia_part_words(args[i]);
            inv_at[i] = basis_words; basis_words += vk::ia_inv_words(args[i]);
        }
        if (desc_words.empty()) desc_words.push_back(0);
        desc_words_n = desc_words.size();
        DBuf desc(&c, desc_words);
        for (size_t i = 0; i < NC; i++) args[i].r.wr = desc.data + wr_at[i];
        c.check_launch("invariant_audit ingest");
        DBuf basis(&c, (size_t)(basis_words ? basis_words : 1));
        // the device pass: everything from here to the last download is between the two events
        pass.begin();
        // phase 1: every chip's invariant basis
        for (size_t i = 0; i < NC; i++) {
            if (!args[i].r.width) continue;
            vk::launch_ia_basis(st, args[i], basis.data + part_at[i]);
            vk::launch_ia_merge(st, args[i], basis.data + part_at[i], basis.data + inv_at[i]);
        }
        c.check_launch("invariant_audit basis");
        {
            std::vector<uint32_t> iv;
            for (size_t i = 0; i < NC; i++) {
                e_at[i] = rep.entries.size();
                vk::IaArgs& ia = args[i];
                ia.d = 0;
                if (!ia.r.width) continue;
                const uint32_t AW = ia.r.width + 1;
                iv.resize(2 + AW);
                c.download_small(iv.data(), basis.data + inv_at[i], iv.size() * 4);
                const uint32_t d = iv[1];
                if (iv[0] + d != AW || d > ia.r.width) throw std::logic_error("invariant_audit: the merged basis is inconsistent");
                std::vector<uint8_t> pivot(AW);
                for (uint32_t k = 0; k < AW; k++) pivot[k] = iv[2 + k] != 0;
                std::vector<vg::Fp> vec((size_t)d * AW);
                if (d) {
                    iv.resize((size_t)d * AW);
                    c.download_small(iv.data(), basis.data + inv_at[i] + 2 + AW, iv.size() * 4);
                    for (size_t k = 0; k < vec.size(); k++) vec[k] = vg::Fp::raw(iv[k]);
                }
                invariant_audit_entries(rep.chips[i], (uint32_t)i, pivot, vec, o.max_terms, rep.entries);
                ia.d = d;
                ia.vec = basis.data + inv_at[i] + 2 + AW;
                if (!d) continue;
                vk::ia_shape(ia);  // with the chip's d: it fitted with d = w
                ia.r.evaluations = ia.r.K ? (double)ia.r.n * ia.r.width * (ia.r.n == 1 ? 1 : 2) : 0;
                rep.evaluations += ia.r.evaluations;
            }
            e_at[NC] = rep.entries.size();
        }
        // phase 2: per invariant the rows that do not enforce it
        AuditScratch sc(NC);
        for (size_t i = 0; i < NC; i++)
            if (args[i].d) sc.add(i, vk::ia_totals_words(args[i]), (uint64_t)args[i].d * args[i].r.NB);
        scratch_words = sc.place_prefixes();
        DBuf scratch(&c, (size_t)(scratch_words ? scratch_words : 1));
        if (sc.zeroed) VG_HIP_CHECK(hipMemsetAsync(scratch.data, 0, (size_t)sc.zeroed * 4, st));
        for (size_t i = 0; i < NC; i++)
            if (args[i].d) vk::launch_ia_count(st, args[i], reinterpret_cast<unsigned long long*>(scratch.data + sc.tot_at[i]), scratch.data + sc.tab_at[i]);
        c.check_launch("invariant_audit count");
        {
            std::vector<uint32_t> tw;
            for (size_t i = 0; i < NC; i++) {
                if (!args[i].d) continue;
                tw.resize(vk::ia_totals_words(args[i]));
                c.download_small(tw.data(), scratch.data + sc.tot_at[i], tw.size() * 4);
                for (uint32_t k = 0; k < args[i].d; k++) {
                    InvariantEntry& en = rep.entries[e_at[i] + k];
                    en.free_rows = audit_u64(tw, k);
                    en.enforced = rep.chips[i].height - en.free_rows;
                }
            }
        }
        invariant_audit_finish(rep, o);
        // the listed invariants of a chip are its first ones: entry e of the list is invariant e - e_at[chip]
        audit_chip_runs(rep.entries, [&](uint32_t chip, size_t e0, size_t e1) {
            rows_words = std::max<uint64_t>(rows_words, (uint64_t)(e1 - e0) * R);
            (void)chip;
        });
        DBuf out(&c, (size_t)(rows_words ? rows_words : 1));
        audit_chip_runs(rep.entries, [&](uint32_t chip, size_t e0, size_t e1) {
            bool any = false;
            for (size_t e = e0; e < e1; e++) any |= rep.entries[e].free_rows != 0;
            if (!any) return;
            // the listed invariants of one chip: scan, list, one download
            const vk::IaArgs& ia = args[chip];
            const uint32_t i_cut = (uint32_t)(e1 - e0);
            const size_t words = (size_t)i_cut * R;
            VG_HIP_CHECK(hipMemsetAsync(out.data, 0, words * 4, st));
            vk::launch_ra_scan(st, ia.r, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], i_cut);
            vk::launch_ia_list(st, ia, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], i_cut, R, out.data);
            c.check_launch("invariant_audit list");
            std::vector<uint32_t> w(words);
            c.download_small(w.data(), out.data, w.size() * 4);
            for (size_t e = e0; e < e1; e++) {
                InvariantEntry& en = rep.entries[e];
                const uint64_t listed = std::min<uint64_t>(en.free_rows, R);
                en.rows.assign(w.begin() + (e - e0) * R, w.begin() + (e - e0) * R + (size_t)listed);
            }
        });
        pass.end(rep);
    }, [&] {
        return std::string("invariant_audit: the device pool cannot give the pass its scratch: per chip (w + 1) (w + 2) words per workgroup of phase 1 (at most 2048, 64 MB) and a sixteenth of that for the merge tree, (w + 1)^2 + 2 of merged basis (" +
                           std::to_string(basis_words * 4) + " bytes for this witness), 8 bytes per invariant of totals and 8 per (invariant, workgroup of rows) (" + std::to_string(scratch_words * 4) +
                           " bytes), " + std::to_string(desc_words_n * 4) + " bytes of interaction weight rows, " + std::to_string(rows_words * 4) +
                           " bytes of listed rows, plus the working-layout copies of uploaded traces; chip_mask audits fewer chips at a time");
    });
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- product audit (host/product_audit.hpp; kernels/product_audit.hip) -----------------------------------------------------------------------
ProductReport Prover::product_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed, const ProductAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const ProductAuditOpts o = product_audit_checked_opts(opts_in, machine_.airs.size());
    const auto tr = audit_traces<ConstraintShape>("product_audit", main, preprocessed);
    std::vector<int> prep_slot;
    product_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, prep_slot);
    const size_t NC = machine_.airs.size();
    const uint32_t R = o.max_rows_per_entry;
    // per chip its launch shapes: a chip the invariant audit would refuse is refused here, before anything is queued
    std::vector<vk::IaArgs> iargs(NC);
    std::vector<vk::PqArgs> args(NC);
    ProductReport rep;
    rep.chips.resize(NC);
    for (size_t i = 0; i < NC; i++) {
        const AirDesc& air = machine_.airs[i];
        iargs[i] = vk::IaArgs{};
        args[i] = vk::PqArgs{};
        ProductChipStat& cs = rep.chips[i];
        product_audit_chip_block(cs, air, main[i]->height, product_audit_selected(o, i));
        if (!cs.audited || !air.width) continue;
        audit_chip_sizes(iargs[i].r, air, main[i]->height, fri_.interpret_air);
        try {
            audit_chip_shape(air, [&] { vk::ia_basis_shape(iargs[i]); iargs[i].d = air.width; vk::ia_shape(iargs[i]); });
        } catch (const std::invalid_argument& e) {
            throw std::invalid_argument(pq_renamed(e));
        }
    }

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const hipStream_t st = pass.stream;

    uint64_t basis_words = 0, space_words = 0, scratch_words = 0, rows_words = 0, desc_words_n = 0;
    audit_or_no_memory(st, [&] {
        std::vector<uint64_t> wr_at(NC, 0), part_at(NC, 0), inv_at(NC, 0);
        std::vector<size_t> e_at(NC + 1, 0);  // chip i's entries are [e_at[i], e_at[i + 1]) until the list is cut
        std::vector<ProductVec> vecs;          // one per entry
        std::vector<std::vector<uint32_t>> pivots(NC);  // per chip the augmented pivot columns, ascending
        std::vector<uint32_t> desc_words;
        for (size_t i = 0; i < NC; i++) {
            vk::RaArgs& a = iargs[i].r;
            if (!a.width) continue;
            pass.bind(a, main[i], audit_prep(preprocessed, prep_slot, i), prog_dev_[i]);
            a.iw = iw_dev_[i].data;
            const std::vector<uint32_t> wr = ra_weight_rows(machine_.airs[i]);
            wr_at[i] = desc_words.size();
            desc_words.insert(desc_words.end(), wr.begin(), wr.end());
            part_at[i] = basis_words; basis_words += vk::ia_part_words(iargs[i]);
            inv_at[i] = basis_words; basis_words += vk::ia_inv_words(iargs[i]);
        }
        if (desc_words.empty()) desc_words.push_back(0);
        desc_words_n = desc_words.size();
        DBuf desc(&c, desc_words);
        for (size_t i = 0; i < NC; i++) iargs[i].r.wr = desc.data + wr_at[i];
        c.check_launch("product_audit ingest");
        // the device pass: everything from here to the last download is between the two events
        pass.begin();
        {
            // (1) every chip's pivot columns: the invariant audit's phase 1 and merge; their scratch goes back to the pool before the rest is taken
            DBuf basis(&c, (size_t)(basis_words ? basis_words : 1));
            for (size_t i = 0; i < NC; i++) {
                if (!iargs[i].r.width) continue;
                vk::launch_ia_basis(st, iargs[i], basis.data + part_at[i]);
                vk::launch_ia_merge(st, iargs[i], basis.data + part_at[i], basis.data + inv_at[i]);
            }
            c.check_launch("product_audit pivots");
            std::vector<uint32_t> iv;
            for (size_t i = 0; i < NC; i++) {
                if (!iargs[i].r.width) continue;
                const uint32_t AW = iargs[i].r.width + 1;
                iv.resize(2 + AW);
                c.download_small(iv.data(), basis.data + inv_at[i], iv.size() * 4);
                std::vector<uint32_t> pcols;
                for (uint32_t k = 0; k < AW; k++) if (iv[2 + k]) pcols.push_back(k);
                if (iv[0] != pcols.size() || pcols.empty() || pcols[0] != 0) throw std::logic_error("product_audit: the merged basis is inconsistent");
                product_audit_space(rep.chips[i], pcols);
                args[i].r = iargs[i].r;
                args[i].rho = (uint32_t)pcols.size();
                pivots[i] = std::move(pcols);
            }
        }
        // (2) - (4) per chip: the basis rows, the inverse, beta of every pair, the two sweeps; its relations come back as (pair, beta)
        std::vector<DBuf> keep;  // what the enforcement phase reads: the chips' lists
        for (size_t i = 0; i < NC; i++) {
            e_at[i] = rep.entries.size();
            vk::PqArgs& pa = args[i];
            if (pa.rho < 2) continue;
            const uint32_t rho = pa.rho, m = (uint32_t)vk::pq_pairs(rho);
            const std::vector<uint32_t>& pcols = pivots[i];
            DBuf pc(&c, pcols);
            pa.pcols = pc.data;
            vk::pq_rows_shape(pa);
            const uint64_t rows_w = vk::pq_rows_words(pa), aug_w = vk::pq_solve_in_lds(rho) ? 0 : 2ull * rho * rho;
            // rows [rho + 1], status [1], count [1], G, inv, the slices' slots, aug, beta [m][rho], flags [m], two pair lists [m]
            const uint64_t at_rows = 0, at_status = at_rows + rho + 1, at_count = at_status + 1, at_G = at_count + 1, at_inv = at_G + (uint64_t)rho * rho, at_part = at_inv + (uint64_t)rho * rho,
                           at_aug = at_part + rows_w, at_beta = at_aug + aug_w, at_flags = at_beta + (uint64_t)m * rho, at_l1 = at_flags + m, at_l2 = at_l1 + m, words = at_l2 + m;
            space_words = std::max(space_words, words);
            DBuf sp(&c, (size_t)words);
            uint32_t* d = sp.data;
            VG_HIP_CHECK(hipMemsetAsync(d + at_rows, 0, (size_t)(rho + 3) * 4, st));  // rows, status, count: row 0 is a row of the trace
            vk::launch_pq_rows(st, pa, d + at_part);
            vk::launch_pq_rowmerge(st, pa, d + at_part, d + at_rows);
            vk::launch_pq_solve(st, pa, d + at_rows, aug_w ? d + at_aug : nullptr, d + at_G, d + at_inv, d + at_status);
            vk::launch_pq_beta(st, pa, d + at_G, d + at_inv, d + at_beta, d + at_flags);
            const uint64_t prefix_rows = std::min<uint64_t>(pa.r.n, vk::PQ_PREFIX_ROWS);
            vk::launch_pq_sweep(st, pa, "k_pq_sweep.prefix", prefix_rows, d + at_beta, nullptr, m, d + at_flags);
            vk::launch_pq_compact(st, d + at_flags, nullptr, m, d + at_l1, d + at_count);
            c.check_launch("product_audit prefix sweep");
            uint32_t head[3];  // rows[0], status, count
            c.download_small(head, d + at_rows, 4);
            c.download_small(head + 1, d + at_status, 8);
            if (head[0] != rho || head[1] != 0) throw std::logic_error("product_audit: the basis rows of chip " + machine_.airs[i].name + " are not independent");
            uint32_t n_rel = head[2];
            if (n_rel > m) throw std::logic_error("product_audit: more survivors than pairs");
            const uint32_t* rel_dev = d + at_l1;
            if (n_rel && prefix_rows < pa.r.n) {
                vk::launch_pq_sweep(st, pa, "k_pq_sweep.survivors", pa.r.n, d + at_beta, d + at_l1, n_rel, d + at_flags);
                vk::launch_pq_compact(st, d + at_flags, d + at_l1, n_rel, d + at_l2, d + at_count);
                c.check_launch("product_audit survivor sweep");
                const uint32_t before = n_rel;
                c.download_small(&n_rel, d + at_count, 4);
                if (n_rel > before) throw std::logic_error("product_audit: more relations than survivors");
                rel_dev = d + at_l2;
            }
            if (!n_rel) continue;
            std::vector<uint32_t> rel(n_rel), betas((size_t)n_rel * rho);
            DBuf gb(&c, betas.size());
            vk::launch_pq_gather(st, pa, d + at_beta, rel_dev, n_rel, gb.data);
            c.check_launch("product_audit gather");
            c.download_small(rel.data(), rel_dev, rel.size() * 4);
            c.download_small(betas.data(), gb.data, betas.size() * 4);
            product_audit_chip_entries(rep.chips[i], (uint32_t)i, pcols, rel, betas, o.max_terms, rep.entries, vecs);
            // (5) the chip's relations as the enforcement kernel takes them, and its launch shape with them
            const ProductLists l = product_audit_lists(vecs.data() + e_at[i], n_rel, vk::PQ_GROUP_ENTRIES, vk::PQ_GROUP_WORDS);
            pa.E = n_rel; pa.G = (uint32_t)l.gstart.size() - 1; pa.GE = l.GE; pa.GW = l.GW;
            keep.emplace_back(&c, l.eoff); pa.eoff = keep.back().data;
            keep.emplace_back(&c, l.ewords); pa.ewords = keep.back().data;
            keep.emplace_back(&c, l.gstart); pa.gstart = keep.back().data;
            audit_chip_shape(machine_.airs[i], [&] { vk::pq_shape(pa); });
            pa.r.evaluations = pa.r.K ? (double)pa.r.n * pa.r.width * (pa.r.n == 1 ? 1 : 2) : 0;
            rep.evaluations += pa.r.evaluations;
        }
        e_at[NC] = rep.entries.size();
        // per relation the rows that do not enforce it
        AuditScratch sc(NC);
        for (size_t i = 0; i < NC; i++)
            if (args[i].E) sc.add(i, vk::pq_totals_words(args[i]), (uint64_t)args[i].E * args[i].r.NB);
        scratch_words = sc.place_prefixes();
        DBuf scratch(&c, (size_t)(scratch_words ? scratch_words : 1));
        if (sc.zeroed) VG_HIP_CHECK(hipMemsetAsync(scratch.data, 0, (size_t)sc.zeroed * 4, st));
        for (size_t i = 0; i < NC; i++)
            if (args[i].E) vk::launch_pq_count(st, args[i], reinterpret_cast<unsigned long long*>(scratch.data + sc.tot_at[i]), scratch.data + sc.tab_at[i]);
        c.check_launch("product_audit count");
        {
            std::vector<uint32_t> tw;
            for (size_t i = 0; i < NC; i++) {
                if (!args[i].E) continue;
                tw.resize(vk::pq_totals_words(args[i]));
                c.download_small(tw.data(), scratch.data + sc.tot_at[i], tw.size() * 4);
                for (uint32_t k = 0; k < args[i].E; k++) {
                    ProductEntry& en = rep.entries[e_at[i] + k];
                    en.free_rows = audit_u64(tw, 2 * k);
                    en.flat_rows = audit_u64(tw, 2 * k + 1);
                    en.enforced = rep.chips[i].height - en.free_rows;
                }
            }
        }
        product_audit_finish(rep, o);
        // the listed relations of a chip are its first ones: entry e of the list is relation e - e_at[chip]
        audit_chip_runs(rep.entries, [&](uint32_t chip, size_t e0, size_t e1) {
            rows_words = std::max<uint64_t>(rows_words, (uint64_t)(e1 - e0) * R);
            (void)chip;
        });
        DBuf out(&c, (size_t)(rows_words ? rows_words : 1));
        audit_chip_runs(rep.entries, [&](uint32_t chip, size_t e0, size_t e1) {
            bool any = false;
            for (size_t e = e0; e < e1; e++) any |= rep.entries[e].free_rows != 0;
            if (!any) return;
            // the listed relations of one chip: scan, list, one download
            const vk::PqArgs& pa = args[chip];
            const uint32_t i_cut = (uint32_t)(e1 - e0);
            const size_t words = (size_t)i_cut * R;
            VG_HIP_CHECK(hipMemsetAsync(out.data, 0, words * 4, st));
            vk::launch_ra_scan(st, pa.r, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], i_cut);
            vk::launch_pq_list(st, pa, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], i_cut, R, out.data);
            c.check_launch("product_audit list");
            std::vector<uint32_t> w(words);
            c.download_small(w.data(), out.data, w.size() * 4);
            for (size_t e = e0; e < e1; e++) {
                ProductEntry& en = rep.entries[e];
                const uint64_t listed = std::min<uint64_t>(en.free_rows, R);
                en.rows.assign(w.begin() + (e - e0) * R, w.begin() + (e - e0) * R + (size_t)listed);
            }
        });
        pass.end(rep);
    }, [&] {
        return std::string("product_audit: the device pool cannot give the pass its scratch: for the pivots the invariant audit's (w + 1) (w + 2) words per workgroup of its phase 1 (at most 2048, 64 MB), a sixteenth of that for the merge tree and (w + 1)^2 + 2 of merged basis (" +
                           std::to_string(basis_words * 4) + " bytes for this witness, given back before the rest is taken); per chip, one chip at a time, rho + 1 words per slice of rows (at most 2048) and a sixteenth of that, 2 rho^2 for the basis rows and their inverse (4 rho^2 when rho > 142), m rho of beta and 3 m of flags and pair lists for m = rho (rho - 1) / 2 pairs (" +
                           std::to_string(space_words * 4) + " bytes for the widest chip so far); 16 bytes per relation of totals and 8 per (relation, workgroup of rows) (" + std::to_string(scratch_words * 4) +
                           " bytes), the relations' sparse lists, " + std::to_string(desc_words_n * 4) + " bytes of interaction weight rows, " + std::to_string(rows_words * 4) +
                           " bytes of listed rows, plus the working-layout copies of uploaded traces; chip_mask audits fewer chips at a time");
    });
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- domain audit (host/domain_audit.hpp; kernels/domain_audit.hip) ------------------------------------------------------------------------
DomainReport Prover::domain_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed, const DomainAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const DomainAuditOpts o = domain_audit_checked_opts(opts_in, machine_.airs.size());
    const auto tr = audit_traces<ConstraintShape>("domain_audit", main, preprocessed);
    const DomainPlan plan = domain_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, o);
    const size_t NC = machine_.airs.size();
    const uint32_t R = o.max_rows_per_entry;
    DomainReport rep;
    domain_audit_blocks(rep, machine_, plan, tr.ms, o);
    std::vector<uint32_t> slot0;
    const uint32_t n_slots = domain_audit_slots(machine_, plan, o, slot0);
    // per chip its launch shape and tables: a chip whose guard table does not fit the LDS is refused before anything is queued
    std::vector<vk::DaArgs> args(NC);
    std::vector<uint32_t> desc_words;
    std::vector<uint64_t> vt_at(NC, 0), gt_at(NC, 0);
    for (size_t i = 0; i < NC; i++) {
        const AirDesc& air = machine_.airs[i];
        vk::DaArgs& a = args[i];
        a = vk::DaArgs{};
        a.n = main[i]->height; a.width = air.width; a.prep_width = air.prep_width;
        vk::da_shape(a);
        const bool audited = rep.chips[i].audited && air.width;
        const std::vector<uint32_t> vt = domain_audit_vt(air, plan.chips[i], audited, slot0[i]);
        a.NV = (uint32_t)(vt.size() / 4);
        vt_at[i] = desc_words.size();
        desc_words.insert(desc_words.end(), vt.begin(), vt.end());
        rep.evaluations += (double)a.n * a.NV;
        rep.evaluations += (double)a.n * air.interactions.size();  // the counts
        if (!audited) { a.width = 0; continue; }
        const std::vector<uint32_t> gt = domain_audit_gt(air, plan.chips[i]);
        a.GW = (uint32_t)gt.size(); a.A = (uint32_t)plan.chips[i].apps.size(); a.slot0 = slot0[i];
        gt_at[i] = desc_words.size();
        desc_words.insert(desc_words.end(), gt.begin(), gt.end());
        if (vk::da_guard_lds_words(a) + 4 * 66 > vk::DA_GUARD_LDS_WORDS)
            throw std::invalid_argument("domain_audit: the guard table of chip " + air.name + " (" + std::to_string(a.GW) + " words for " + std::to_string(plan.chips[i].items.size()) +
                                        " items, " + std::to_string(5 * (size_t)air.width + a.A) + " counters) does not fit 64 KB of LDS [the host audit has no limit]");
    }

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const hipStream_t st = pass.stream;

    uint64_t scratch_words = 0, rows_words = 0;
    audit_or_no_memory(st, [&] {
        for (size_t i = 0; i < NC; i++) {
            vk::DaArgs& a = args[i];
            if (!a.NV && !a.width) continue;  // neither a column nor a field: the chip is not read
            const vk::DMatView v = pass.working(main[i]);
            a.main = v.data; a.mstride = v.stride;
            if (const DeviceTrace* p = audit_prep(preprocessed, plan.prep_slot, i)) { const vk::DMatView pv = pass.working(p); a.prep = pv.data; a.pstride = pv.stride; }
            a.iw = iw_dev_[i].data;
        }
        if (desc_words.empty()) desc_words.push_back(0);
        DBuf desc(&c, desc_words);
        for (size_t i = 0; i < NC; i++) { args[i].vt = desc.data + vt_at[i]; args[i].gt = desc.data + gt_at[i]; }
        c.check_launch("domain_audit ingest");
        // the scratch (u32 words), all of it zeroed by one memset: tot [slots][5] u64, cls [slots][8], bitmaps [slots][2048], per audited chip
        // gtot [5 w + A] u64 and table [w][NB]; behind them the prefix tables, which the scan writes whole
        const uint64_t tot_at = 0, cls_at = tot_at + 2ull * vk::DA_TOT * n_slots, bm_at = cls_at + (uint64_t)vk::DA_CLS * n_slots;
        AuditScratch sc(NC);
        sc.zeroed = bm_at + (uint64_t)vk::DA_BITMAP_WORDS * n_slots;
        for (size_t i = 0; i < NC; i++)
            if (args[i].width) sc.add(i, 2 * (5ull * args[i].width + args[i].A), (uint64_t)args[i].width * args[i].NB);
        scratch_words = sc.place_prefixes();
        DBuf scratch(&c, (size_t)(scratch_words ? scratch_words : 1));
        unsigned long long* tot = reinterpret_cast<unsigned long long*>(scratch.data + tot_at);
        uint32_t* cls = scratch.data + cls_at;
        pass.begin();
        if (sc.zeroed) VG_HIP_CHECK(hipMemsetAsync(scratch.data, 0, (size_t)sc.zeroed * 4, st));
        for (size_t i = 0; i < NC; i++)
            if (args[i].NV) vk::launch_da_scan(st, args[i], tot, scratch.data + bm_at);
        vk::launch_da_classify(st, tot, scratch.data + bm_at, cls, n_slots, o.max_bits);
        for (size_t i = 0; i < NC; i++)
            if (args[i].width) vk::launch_da_guard(st, args[i], vk::MA_COUNT, cls, reinterpret_cast<unsigned long long*>(scratch.data + sc.tot_at[i]), scratch.data + sc.tab_at[i], nullptr, 0, 0, nullptr);
        c.check_launch("domain_audit count");
        // tot and cls lie in front: one download; then the guard totals of each audited chip
        std::vector<uint32_t> tw((size_t)bm_at ? (size_t)bm_at : 1);
        if (bm_at) c.download_small(tw.data(), scratch.data, (size_t)bm_at * 4);
        auto total = [&](uint32_t s, uint32_t k) { return audit_u64(tw, (size_t)s * vk::DA_TOT + k); };
        for (uint32_t p = 0; p < plan.n_positions; p++) {
            if (!total(p, 4)) continue;
            const uint32_t* k = tw.data() + cls_at + (size_t)p * vk::DA_CLS;
            DomainPosition& dp = rep.positions[p];
            dp.min = k[5]; dp.max = k[6]; dp.distinct = k[0]; dp.wide = total(p, 3); dp.records = total(p, 4);
        }
        std::vector<uint32_t> gw;
        for (size_t i = 0; i < NC; i++) {
            if (!args[i].width) continue;
            DomainChipStat& cs = rep.chips[i];
            const uint32_t W = args[i].width;
            gw.resize(2 * (5 * (size_t)W + args[i].A));
            c.download_small(gw.data(), scratch.data + sc.tot_at[i], gw.size() * 4);
            for (uint32_t col = 0; col < W; col++) {
                const uint32_t s = slot0[i] + col;
                const uint32_t* k = tw.data() + cls_at + (size_t)s * vk::DA_CLS;
                DomainColumn& dc = cs.cols[col];
                dc.distinct = k[0]; dc.cls = k[1]; dc.dense = k[2]; dc.bits = k[3]; dc.narrow = k[4]; dc.min = k[5]; dc.max = k[6];
                dc.nonzero = total(s, 2); dc.wide = total(s, 3);
                dc.guarded = audit_u64(gw, 5 * (size_t)col); dc.sent = audit_u64(gw, 5 * (size_t)col + 1); dc.received = audit_u64(gw, 5 * (size_t)col + 2);
                dc.mixed = audit_u64(gw, 5 * (size_t)col + 3);
                dc.unguarded = args[i].n - dc.guarded;
                // a column without items that is not narrow is not walked by the guard pass: none of its rows is guarded
                const bool walked = dc.narrow || plan.chips[i].item_at[col] != plan.chips[i].item_at[col + 1];
                dc.unguarded_nonzero = walked ? audit_u64(gw, 5 * (size_t)col + 4) : dc.nonzero;
            }
            for (uint32_t k = 0; k < args[i].A; k++) cs.app_live[k] = audit_u64(gw, 5 * (size_t)W + k);
        }
        domain_audit_entries(rep, plan, o);
        if (R) {
            audit_chip_runs(rep.entries, [&](uint32_t, size_t, size_t e1) { rows_words = std::max<uint64_t>(rows_words, ((uint64_t)rep.entries[e1 - 1].column + 1) * R * 2); });
            DBuf out(&c, (size_t)(rows_words ? rows_words : 1));
            audit_chip_runs(rep.entries, [&](uint32_t chip, size_t e0, size_t e1) {
                // the listed columns of one chip: scan, list, one download
                const vk::DaArgs& a = args[chip];
                const uint32_t c_cut = rep.entries[e1 - 1].column + 1;  // entries ascend: the listed columns of a chip are below it
                const size_t words = (size_t)c_cut * R * 2;
                vk::launch_ra_scan(st, vk::da_scan_args(a), scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], c_cut);
                vk::launch_da_guard(st, a, vk::MA_LIST, cls, nullptr, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], c_cut, R, out.data);
                c.check_launch("domain_audit list");
                std::vector<uint32_t> w(words);
                c.download_small(w.data(), out.data, w.size() * 4);
                for (size_t e = e0; e < e1; e++) {
                    DomainEntry& en = rep.entries[e];
                    const uint64_t listed = std::min<uint64_t>(en.unguarded_nonzero, R);
                    en.rows.assign(w.begin() + (size_t)en.column * R * 2, w.begin() + (size_t)en.column * R * 2 + (size_t)listed * 2);
                }
            });
        }
        pass.end(rep);
    }, [&] {
        return std::string("domain_audit: the device pool cannot give the pass its scratch: per slot (" + std::to_string(n_slots) + ": the main columns of the audited chips and " +
                           std::to_string(plan.n_positions) + " bus positions) 8192 bytes of bitmap, 40 of totals and 32 of classes, per audited chip 40 bytes per column, 8 per appearance and 8 per "
                           "(column, workgroup of 256 rows) (" + std::to_string(scratch_words * 4) + " bytes for this witness), " + std::to_string(rows_words * 4) +
                           " bytes of listed rows (8 per (listed column, row slot)), plus the working-layout copies of uploaded traces; chip_mask audits fewer chips at a time");
    });
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- transition audit (host/transition_audit.hpp; kernels/transition_audit.hip) --------------------------------------------------------------
TransitionReport Prover::transition_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed, const TransitionAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const TransitionAuditOpts o = transition_audit_checked_opts(opts_in, machine_.airs.size());
    const auto tr = audit_traces<ConstraintShape>("transition_audit", main, preprocessed);
    std::vector<int> prep_slot;
    transition_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, prep_slot);
    const size_t NC = machine_.airs.size();
    const uint32_t R = o.max_rows_per_entry;
    // per chip its launch shapes: a chip that does not fit is refused before anything is queued (phase 1 by its window, phase 2 with one entry staged)
    std::vector<vk::TaArgs> args(NC);
    TransitionReport rep;
    rep.chips.resize(NC);
    for (size_t i = 0; i < NC; i++) {
        const AirDesc& air = machine_.airs[i];
        args[i] = vk::TaArgs{};
        TransitionChipStat& cs = rep.chips[i];
        transition_audit_chip_block(cs, air, main[i]->height, transition_audit_selected(o, i));
        if (!transition_audit_has_windows(cs)) continue;
        audit_chip_sizes(args[i].r, air, main[i]->height, fri_.interpret_air);
        audit_chip_shape(air, [&] { vk::ta_basis_shape(args[i], o.max_gates); args[i].E = 0; vk::ta_shape(args[i]); });
    }

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const hipStream_t st = pass.stream;

    uint64_t flag_words = 0, basis_words = 0, entry_words = 0, bits_words = 0, desc_words_n = 0;
    audit_or_no_memory(st, [&] {
        std::vector<uint64_t> wr_at(NC, 0), fl_at(NC, 0);
        std::vector<uint32_t> desc_words;
        for (size_t i = 0; i < NC; i++) {
            vk::RaArgs& a = args[i].r;
            if (!a.width) continue;
            pass.bind(a, main[i], audit_prep(preprocessed, prep_slot, i), prog_dev_[i]);
            a.iw = iw_dev_[i].data;
            const std::vector<uint32_t> wr = ra_weight_rows(machine_.airs[i]);
            wr_at[i] = desc_words.size();
            desc_words.insert(desc_words.end(), wr.begin(), wr.end());
            // per window column a u64 of ones, then a u32 of flags (AW + 1 of them: the next chip's u64 stay 8-byte aligned)
            fl_at[i] = flag_words; flag_words += 3ull * (2ull * a.width + 2);
        }
        if (desc_words.empty()) desc_words.push_back(0);
        desc_words_n = desc_words.size();
        DBuf desc(&c, desc_words);
        for (size_t i = 0; i < NC; i++) args[i].r.wr = desc.data + wr_at[i];
        c.check_launch("transition_audit ingest");
        DBuf flags(&c, (size_t)(flag_words ? flag_words : 1));
        // the device pass: everything from here to the last download is between the two events
        pass.begin();
        // the boolean window columns of every chip
        if (flag_words) VG_HIP_CHECK(hipMemsetAsync(flags.data, 0, (size_t)flag_words * 4, st));
        for (size_t i = 0; i < NC; i++) {
            if (!args[i].r.width) continue;
            const uint64_t AW1 = 2ull * args[i].r.width + 2;
            vk::launch_ta_flags(st, args[i], flags.data + fl_at[i] + 2 * AW1, reinterpret_cast<unsigned long long*>(flags.data + fl_at[i]));
        }
        c.check_launch("transition_audit flags");
        std::vector<size_t> g_at(NC + 1, 0);  // chip i's gates are [g_at[i], g_at[i + 1])
        {
            std::vector<uint32_t> fw((size_t)flag_words);
            if (flag_words) c.download_small(fw.data(), flags.data, fw.size() * 4);
            for (size_t i = 0; i < NC; i++) {
                g_at[i] = rep.gates.size();
                if (!args[i].r.width) continue;
                const uint32_t AW = 2 * args[i].r.width + 1;
                std::vector<uint32_t> fl(AW);
                std::vector<uint64_t> ones(AW);
                for (uint32_t j = 0; j < AW; j++) { ones[j] = audit_u64(fw, (size_t)(fl_at[i] / 2) + j); fl[j] = fw[(size_t)fl_at[i] + 2 * (AW + 1) + j]; }
                transition_audit_gates(rep.chips[i], (uint32_t)i, fl, ones, o, rep.gates);
            }
            g_at[NC] = rep.gates.size();
        }
        // phase 1: per chip the reduced basis of every audited gate, one chip's scratch at a time
        for (size_t i = 0; i < NC; i++) {
            vk::TaArgs& ta = args[i];
            if (!ta.r.width) continue;
            const uint32_t W = ta.r.width, AW = 2 * W + 1;
            std::vector<uint32_t> gw;  // the audited gates, in order
            std::vector<size_t> which;
            for (size_t g = g_at[i]; g < g_at[i + 1]; g++) {
                if (!rep.gates[g].audited) continue;
                gw.push_back(rep.gates[g].column); gw.push_back(rep.gates[g].value ? vg::Fp::one().v : 0u);
                which.push_back(g);
            }
            ta.G = (uint32_t)which.size();
            vk::ta_basis_shape(ta, ta.G);
            DBuf gates(&c, gw);
            ta.gates = gates.data;
            const uint64_t part_words = vk::ta_part_words(ta), inv_words = vk::ta_inv_words(ta);
            basis_words = std::max(basis_words, part_words + ta.G * inv_words);
            DBuf part(&c, (size_t)part_words), inv(&c, (size_t)(ta.G * inv_words));
            vk::launch_ta_basis(st, ta, part.data);
            vk::launch_ta_merge(st, ta, part.data, inv.data);
            c.check_launch("transition_audit basis");
            std::vector<uint32_t> iv((size_t)(ta.G * inv_words));
            c.download_small(iv.data(), inv.data, iv.size() * 4);
            TransitionBasis b0;
            for (size_t k = 0; k < which.size(); k++) {
                const uint32_t* v = iv.data() + k * inv_words;
                const uint32_t d = v[1];
                if (v[0] + d != AW || d >= AW) throw std::logic_error("transition_audit: the merged basis is inconsistent");
                TransitionBasis b;
                b.pivot.resize(AW);
                for (uint32_t x = 0; x < AW; x++) b.pivot[x] = v[2 + x] != 0;
                b.vec.resize((size_t)d * AW);
                for (size_t x = 0; x < b.vec.size(); x++) b.vec[x] = vg::Fp::raw(v[2 + AW + x]);
                if (k == 0) b0 = b;
                transition_audit_entries(rep.chips[i], rep.gates[which[k]], b0, b, o.max_terms, rep.entries);
            }
            ta.gates = nullptr;
        }
        transition_audit_cut(rep, o);
        // phase 2: the verdicts of the listed entries, one chip's scratch at a time
        audit_chip_runs(rep.entries, [&](uint32_t chip, size_t e0, size_t e1) {
            vk::TaArgs& ta = args[chip];
            vk::RaArgs& a = ta.r;
            const uint32_t W = a.width, E = (uint32_t)(e1 - e0);
            std::vector<uint32_t> ev((size_t)E * 2 * W), eg((size_t)E * 4, 0);
            std::vector<uint64_t> windows(E, 0);
            for (uint32_t k = 0; k < E; k++) {
                const TransitionEntry& en = rep.entries[e0 + k];
                uint32_t nz = 0;
                for (uint32_t x = 0; x < 2 * W; x++) { ev[(size_t)k * 2 * W + x] = en.l[1 + x].v; if (en.l[1 + x].v) nz |= x < W ? 1u : 2u; }
                eg[4 * (size_t)k] = en.gate_column; eg[4 * (size_t)k + 1] = en.gate_value ? vg::Fp::one().v : 0u; eg[4 * (size_t)k + 2] = nz;
                for (size_t g = g_at[chip]; g < g_at[chip + 1]; g++)
                    if (rep.gates[g].column == en.gate_column && rep.gates[g].value == en.gate_value) windows[k] = rep.gates[g].windows;
            }
            ta.E = E;
            vk::ta_shape(ta);  // with the chip's entries: it fitted with one
            a.evaluations = a.K ? (double)a.n * a.width * 2 : 0;
            rep.evaluations += a.evaluations;
            const uint64_t tab = (uint64_t)E * ta.NB2;
            entry_words = std::max<uint64_t>(entry_words, ev.size() + eg.size() + 2ull * E + 2 * tab + (uint64_t)E * R);
            bits_words = std::max(bits_words, vk::ta_bits_words(ta));
            DBuf evec(&c, ev), egate(&c, eg);
            ta.evec = evec.data; ta.egate = egate.data;
            DBuf bits(&c, (size_t)vk::ta_bits_words(ta));
            DBuf scratch(&c, (size_t)(2ull * E + 2 * tab)), out(&c, (size_t)E * R);
            uint32_t *table = scratch.data + 2ull * E, *prefix = table + tab;
            VG_HIP_CHECK(hipMemsetAsync(scratch.data, 0, (size_t)(2ull * E + tab) * 4, st));
            vk::launch_ta_enforce(st, ta, bits.data);
            vk::launch_ta_count(st, ta, bits.data, reinterpret_cast<unsigned long long*>(scratch.data), table);
            c.check_launch("transition_audit count");
            std::vector<uint32_t> tw(2 * (size_t)E);
            c.download_small(tw.data(), scratch.data, tw.size() * 4);
            bool any = false;
            for (uint32_t k = 0; k < E; k++) {
                TransitionEntry& en = rep.entries[e0 + k];
                en.free_windows = audit_u64(tw, k);
                if (en.free_windows > windows[k]) throw std::logic_error("transition_audit: more free windows than the gate has");
                en.held_windows = windows[k] - en.free_windows;
                any |= en.free_windows != 0;
            }
            if (any) {
                VG_HIP_CHECK(hipMemsetAsync(out.data, 0, (size_t)E * R * 4, st));
                vk::launch_ta_scan(st, ta, table, prefix);
                vk::launch_ta_list(st, ta, bits.data, table, prefix, R, out.data);
                c.check_launch("transition_audit list");
                std::vector<uint32_t> w((size_t)E * R);
                c.download_small(w.data(), out.data, w.size() * 4);
                for (uint32_t k = 0; k < E; k++) {
                    TransitionEntry& en = rep.entries[e0 + k];
                    const uint64_t listed = std::min<uint64_t>(en.free_windows, R);
                    en.rows.assign(w.begin() + (size_t)k * R, w.begin() + (size_t)k * R + (size_t)listed);
                }
            }
            ta.evec = ta.egate = nullptr;
        });
        pass.end(rep);
    }, [&] {
        return std::string("transition_audit: the device pool cannot give the pass its scratch: 12 bytes per window column of flags (" + std::to_string(flag_words * 4) +
                           " bytes), per chip and audited gate (2 w + 1) (2 w + 2) words per slice of phase 1 (at most 2048 slices and 128 MB per chip) and a sixteenth of that for the merge tree, (2 w + 1)^2 + 2 of merged basis (" +
                           std::to_string(basis_words * 4) + " bytes for the largest chip of this witness), per chip with listed entries 8 w + 24 + 4 R bytes per entry and 8 per (entry, 256 windows or more) (" +
                           std::to_string(entry_words * 4) + " bytes) and one bit per (entry, half, row) in words of 32 entries (" + std::to_string(bits_words * 4) + " bytes), " +
                           std::to_string(desc_words_n * 4) + " bytes of interaction weight rows, plus the working-layout copies of uploaded traces; chip_mask audits fewer chips and max_entries lists fewer entries at a time");
    });
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- field audit (host/field_audit.hpp; kernels/field_audit.hip) ---------------------------------------------------------------------------
FieldReport Prover::field_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed, const RankAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const RankAuditOpts o = field_audit_checked_opts(opts_in, machine_.airs.size());
    const auto tr = audit_traces<ConstraintShape>("field_audit", main, preprocessed);
    std::vector<int> prep_slot;
    field_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, prep_slot);
    const size_t NC = machine_.airs.size();
    const uint32_t R = o.max_rows_per_entry;
    // per chip its launch shape: a chip that does not fit the LDS is refused before anything is queued
    std::vector<vk::FaArgs> args(NC);
    std::vector<std::vector<uint32_t>> wrs(NC), slot0(NC);  // weight rows; the first slot of every interaction
    FieldReport rep;
    rep.chips.resize(NC);
    for (size_t i = 0; i < NC; i++) {
        const AirDesc& air = machine_.airs[i];
        vk::FaArgs& a = args[i];
        a = vk::FaArgs{};
        wrs[i] = ra_weight_rows(air);
        FieldChipStat& cs = rep.chips[i];
        field_audit_chip_block(cs, air, main[i]->height, rank_audit_selected(o, i), wrs[i]);
        if (!cs.audited || !air.width) continue;
        audit_chip_sizes(a, air, main[i]->height, fri_.interpret_air);
        a.M = (uint32_t)air.interactions.size();
        for (auto& it : cs.interactions) { slot0[i].push_back(a.NS); a.NS += it.n_fields; a.F = std::max(a.F, it.n_fields); }
        audit_chip_shape(air, [&] { vk::fa_shape(a); });
        a.evaluations = a.K && a.M ? (double)a.n * a.width * (a.n == 1 ? 1 : 2) : 0;
        rep.evaluations += a.evaluations;
    }

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const hipStream_t st = pass.stream;

    uint64_t scratch_words = 0, rows_words = 0, desc_words_n = 0;
    audit_or_no_memory(st, [&] {
        // per chip: its weight rows and its slice of the scratch (u32 words): totals, table [NS NB], prefix [NS NB]
        AuditScratch sc(NC);
        std::vector<uint64_t> wr_at(NC, 0);
        std::vector<uint32_t> desc_words;
        for (size_t i = 0; i < NC; i++) {
            vk::FaArgs& a = args[i];
            if (!a.width) continue;
            pass.bind(a, main[i], audit_prep(preprocessed, prep_slot, i), prog_dev_[i]);
            a.iw = iw_dev_[i].data;
            wr_at[i] = desc_words.size();
            desc_words.insert(desc_words.end(), wrs[i].begin(), wrs[i].end());
            sc.add(i, vk::fa_totals_words(a), (uint64_t)a.NS * a.NB);
        }
        scratch_words = sc.place_prefixes();
        if (desc_words.empty()) desc_words.push_back(0);
        desc_words_n = desc_words.size();
        DBuf desc(&c, desc_words);
        for (size_t i = 0; i < NC; i++) args[i].wr = desc.data + wr_at[i];
        c.check_launch("field_audit ingest");
        DBuf scratch(&c, (size_t)(scratch_words ? scratch_words : 1));
        // the device pass: everything from here to the last download is between the two events
        pass.begin();
        if (sc.zeroed) VG_HIP_CHECK(hipMemsetAsync(scratch.data, 0, (size_t)sc.zeroed * 4, st));
        for (size_t i = 0; i < NC; i++)
            if (args[i].width) vk::launch_fa_count(st, args[i], reinterpret_cast<unsigned long long*>(scratch.data + sc.tot_at[i]), scratch.data + sc.tab_at[i]);
        c.check_launch("field_audit count");
        {
            std::vector<uint32_t> tw;
            for (size_t i = 0; i < NC; i++) {
                if (!args[i].width) continue;
                FieldChipStat& cs = rep.chips[i];
                tw.resize(vk::fa_totals_words(args[i]));
                c.download_small(tw.data(), scratch.data + sc.tot_at[i], tw.size() * 4);
                auto u64 = [&](size_t k) { return audit_u64(tw, k); };
                cs.live_records = u64(0); cs.floating_fields = u64(1); cs.floating_rows = u64(2);
                for (size_t m = 0; m < cs.interactions.size(); m++) {
                    FieldInteractionStat& s = cs.interactions[m];
                    s.live_rows = u64(3 + m);
                    for (uint32_t j = 0; j < s.n_fields; j++) s.floating[j] = u64(3 + cs.interactions.size() + slot0[i][m] + j);
                }
            }
        }
        field_audit_finish(rep, o);
        auto slot_of = [&](const FieldEntry& e) { return slot0[e.chip][e.interaction] + e.field; };
        audit_chip_runs(rep.entries, [&](uint32_t, size_t, size_t e1) {
            rows_words = std::max<uint64_t>(rows_words, ((uint64_t)slot_of(rep.entries[e1 - 1]) + 1) * R * RA_ROW_WORDS);
        });
        DBuf out(&c, (size_t)(rows_words ? rows_words : 1));
        audit_chip_runs(rep.entries, [&](uint32_t chip, size_t e0, size_t e1) {
            // the listed slots of one chip: scan, list, one download
            const vk::FaArgs& a = args[chip];
            const uint32_t s_cut = slot_of(rep.entries[e1 - 1]) + 1;  // entries ascend: the listed slots of a chip are below it
            const size_t words = (size_t)s_cut * R * RA_ROW_WORDS;
            VG_HIP_CHECK(hipMemsetAsync(out.data, 0, words * 4, st));  // unused term slots are zero
            vk::launch_fa_scan(st, a, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], s_cut);
            vk::launch_fa_list(st, a, scratch.data + sc.tab_at[chip], scratch.data + sc.pre_at[chip], s_cut, R, out.data);
            c.check_launch("field_audit list");
            std::vector<uint32_t> w(words);
            c.download_small(w.data(), out.data, w.size() * 4);
            for (size_t e = e0; e < e1; e++) {
                FieldEntry& en = rep.entries[e];
                const uint64_t listed = std::min<uint64_t>(en.floating, R);
                en.rows.resize((size_t)listed);
                for (size_t k = 0; k < listed; k++) {
                    const uint32_t* src = w.data() + ((size_t)slot_of(en) * R + k) * RA_ROW_WORDS;
                    en.rows[k].row = src[0]; en.rows[k].n_support = src[1];
                    for (uint32_t x = 0; x < 2 * RA_TERMS; x++) en.rows[k].terms[x] = src[2 + x];
                }
            }
        });
        pass.end(rep);
    }, [&] {
        return std::string("field_audit: the device pool cannot give the pass its scratch: 24 bytes of totals, 8 per interaction and field, and 8 per (field, workgroup of rows) of every chip (" +
                           std::to_string(scratch_words * 4) + " bytes for this witness), " + std::to_string(desc_words_n * 4) + " bytes of interaction weight rows, " + std::to_string(rows_words * 4) +
                           " bytes of listed rows (72 per (listed field, row slot)), plus the working-layout copies of uploaded traces; chip_mask audits fewer chips at a time");
    });
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- link audit (host/link_audit.hpp; kernels/link_audit.hip) ------------------------------------------------------------------------------
LinkReport Prover::link_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed, const LinkAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const LinkAuditOpts o = link_audit_checked_opts(opts_in);
    const auto tr = audit_traces<BusShape>("link_audit", main, preprocessed);
    std::vector<int> prep_slot;
    const BusPlan plan = link_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, prep_slot);
    const uint64_t n = plan.n_slots;
    if (n >= 0xffffffffull) throw std::invalid_argument("link_audit: more than 2^32 - 2 (row, interaction) pairs; record ids are 32-bit");
    const size_t NC = machine_.airs.size(), NB = plan.buses.size();
    LinkReport rep;
    link_audit_blocks(rep, machine_, plan);
    // per chip the mask pass's launch shape (a chip that does not fit the LDS is refused before anything is queued) and its fields' slots
    std::vector<vk::FaArgs> args(NC);
    std::vector<std::vector<uint32_t>> wrs(NC);
    std::vector<uint32_t> lt(4 + NC, 0);  // launch.hpp: the tally's table of field slots
    uint32_t n_fields = 0;
    for (size_t i = 0; i < NC; i++) {
        const AirDesc& air = machine_.airs[i];
        vk::FaArgs& a = args[i];
        a = vk::FaArgs{};
        lt[4 + i] = (uint32_t)lt.size();
        for (auto& it : rep.chips[i]) { lt.push_back(n_fields); n_fields += it.n_fields; }
        if (!air.width || air.interactions.empty()) continue;  // no record, or only constant fields: the zeroed masks are the answer
        wrs[i] = ra_weight_rows(air);
        audit_chip_sizes(a, air, main[i]->height, fri_.interpret_air);
        a.M = (uint32_t)air.interactions.size();
        for (auto& it : rep.chips[i]) { a.NS += it.n_fields; a.F = std::max(a.F, it.n_fields); }
        audit_chip_shape(air, [&] { vk::la_shape(a); });
        a.evaluations = a.K ? (double)a.n * a.width * (a.n == 1 ? 1 : 2) : 0;
        rep.evaluations += a.evaluations;
    }
    lt[0] = n_fields;
    const uint64_t tally_words = vk::la_tally_words(n_fields, (uint32_t)NB);

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const hipStream_t st = pass.stream;

    uint64_t wr_words = 0, n_open = 0;
    audit_or_no_memory(st, [&] {
        // working-layout copies, as prove makes them (traces generated on the device are already column-major Montgomery)
        std::vector<const uint32_t*> mptr(NC, nullptr), pptr(NC, nullptr);
        std::vector<uint64_t> mstride(NC, 0), pstride(NC, 0);
        std::vector<uint64_t> wr_at(NC, 0);
        std::vector<uint32_t> wr_all;
        for (size_t i = 0; i < NC; i++) {
            if (!plan.chips[i].M) continue;  // a chip without interactions is not read
            const vk::DMatView v = pass.working(main[i]);
            mptr[i] = v.data; mstride[i] = v.stride;
            if (prep_slot[i] >= 0) { const vk::DMatView pv = pass.working(preprocessed[(size_t)prep_slot[i]].second); pptr[i] = pv.data; pstride[i] = pv.stride; }
            vk::FaArgs& a = args[i];
            if (!a.width) continue;
            a.main = mptr[i]; a.mstride = mstride[i]; a.prep = pptr[i]; a.pstride = pstride[i];
            a.prog = (const vair::Instr*)prog_dev_[i].data;
            a.iw = iw_dev_[i].data;
            wr_at[i] = wr_all.size();
            wr_all.insert(wr_all.end(), wrs[i].begin(), wrs[i].end());
        }
        if (wr_all.empty()) wr_all.push_back(0);
        wr_words = wr_all.size();
        c.check_launch("link_audit ingest");
        DBuf desc(&c, bus_audit_descriptor(machine_, plan, mptr, mstride, pptr, pstride)), wr_dev(&c, wr_all), lt_dev(&c, lt);
        for (size_t i = 0; i < NC; i++) args[i].wr = wr_dev.data + wr_at[i];

        uint32_t total_inter = 0;
        std::vector<uint32_t> inter_base(NC, 0);
        for (size_t i = 0; i < NC; i++) { inter_base[i] = total_inter; total_inter += plan.chips[i].M; }
        const size_t n_counters = 8 + NB + total_inter;
        const uint64_t na = n ? n : 1;
        DBuf keys2(&c, (size_t)(4 * na)), ids2(&c, (size_t)(2 * na)), cnt(&c, (size_t)na), gid(&c, (size_t)na), head_pos(&c, (size_t)na), sums(&c, (size_t)(4 * na)),
            nrec(&c, (size_t)(2 * na)), mask(&c, (size_t)na), tmask(&c, (size_t)na), sort_tmp(&c, vk::bus_audit_sort_scratch_words(na)), scan_tmp(&c, vk::bus_audit_scan_scratch_words(na)),
            counters(&c, n_counters), tally(&c, (size_t)(2 * tally_words ? 2 * tally_words : 2));
        unsigned long long* keys = (unsigned long long*)keys2.data;
        unsigned long long* sums_p = (unsigned long long*)sums.data;
        // the device pass: everything from here to the last download is between the two events
        pass.begin();
        VG_HIP_CHECK(hipMemsetAsync(counters.data, 0, n_counters * 4, st));
        VG_HIP_CHECK(hipMemsetAsync(sums.data, 0, (size_t)(4 * na) * 4, st));
        VG_HIP_CHECK(hipMemsetAsync(nrec.data, 0, (size_t)(2 * na) * 4, st));
        VG_HIP_CHECK(hipMemsetAsync(mask.data, 0, (size_t)na * 4, st));
        VG_HIP_CHECK(hipMemsetAsync(tally.data, 0, (size_t)(2 * tally_words ? 2 * tally_words : 2) * 4, st));

        for (size_t i = 0; i < NC; i++)
            if (args[i].width) vk::launch_la_masks(st, args[i], (uint32_t)plan.chips[i].first_id, mask.data);
        for (size_t i = 0; i < NC; i++)
            vk::launch_ba_records(st, desc.data, (uint32_t)i, plan.chips[i].height, machine_.airs[i].width, plan.chips[i].M, o.hash_bits, keys, ids2.data, cnt.data,
                                  counters.data + 8 + NB + inter_base[i]);
        int shifts[8], n_shifts = 0;
        for (uint32_t b = 0; b < (o.hash_bits + 7) / 8; b++) shifts[n_shifts++] = 8 * (int)b;
        if (o.hash_bits <= 56) shifts[n_shifts++] = 56;  // the pass that sinks the dead slots (key ~0) behind the live ones
        int half = vk::launch_ba_sort(st, keys, ids2.data, n, sort_tmp.data, shifts, n_shifts, 0);
        vk::launch_ba_groups(st, desc.data, keys + (uint64_t)half * n, ids2.data + (uint64_t)half * n, n, false, gid.data, head_pos.data, scan_tmp.data, counters.data);
        vk::launch_ba_reduce(st, desc.data, ids2.data + (uint64_t)half * n, cnt.data, gid.data, head_pos.data, n, true, sums_p, nrec.data, counters.data);
        c.check_launch("link_audit");
        std::vector<uint32_t> cw(n_counters);
        c.download_small(cw.data(), counters.data, n_counters * 4);
        if (cw[2]) {
            // a key collision (the hash_bits test hook forces it): group by the full padded tuples instead, exactly as Prover::bus_audit does
            VG_HIP_CHECK(hipMemsetAsync(counters.data + 1, 0, (7 + NB) * 4, st));
            VG_HIP_CHECK(hipMemsetAsync(sums.data, 0, (size_t)(4 * na) * 4, st));
            VG_HIP_CHECK(hipMemsetAsync(nrec.data, 0, (size_t)(2 * na) * 4, st));
            const int all[8] = {0, 8, 16, 24, 32, 40, 48, 56};
            half = 0;
            vk::launch_ba_iota(st, ids2.data, n);
            for (int chunk = (int)(plan.wmax + 1 + 1) / 2 - 1; chunk >= 0; chunk--) {
                vk::launch_ba_rekey(st, desc.data, (uint32_t)chunk, ids2.data + (uint64_t)half * n, cnt.data, keys + (uint64_t)half * n, n);
                half = vk::launch_ba_sort(st, keys, ids2.data, n, sort_tmp.data, all, 8, half);
            }
            vk::launch_ba_groups(st, desc.data, keys + (uint64_t)half * n, ids2.data + (uint64_t)half * n, n, true, gid.data, head_pos.data, scan_tmp.data, counters.data);
            vk::launch_ba_reduce(st, desc.data, ids2.data + (uint64_t)half * n, cnt.data, gid.data, head_pos.data, n, false, sums_p, nrec.data, counters.data);
            c.check_launch("link_audit exact");
            c.download_small(cw.data(), counters.data, n_counters * 4);
        }
        const uint32_t n_live = cw[0], n_groups = cw[1];
        const uint32_t* ids = ids2.data + (uint64_t)half * n;
        if (n_groups) VG_HIP_CHECK(hipMemsetAsync(tmask.data, 0xff, (size_t)n_groups * 4, st));
        vk::launch_la_join(st, ids, mask.data, gid.data, n_live, tmask.data);
        vk::launch_la_tally(st, desc.data, lt_dev.data, ids, mask.data, gid.data, head_pos.data, tmask.data, n_live, n_fields, (uint32_t)NB, (unsigned long long*)tally.data);
        c.check_launch("link_audit join");
        std::vector<uint32_t> tw((size_t)(2 * tally_words ? 2 * tally_words : 2));
        c.download_small(tw.data(), tally.data, tw.size() * 4);
        auto u64 = [&](uint64_t k) { return audit_u64(tw, (size_t)k); };
        for (size_t i = 0; i < NC; i++)
            for (size_t m = 0; m < rep.chips[i].size(); m++) {
                LinkInteractionStat& s = rep.chips[i][m];
                s.live_rows = cw[8 + NB + inter_base[i] + m];
                rep.buses[plan.chips[i].bus_slot[m]].live += s.live_rows;
                const uint32_t slot = lt[lt[4 + i] + m];
                for (uint32_t j = 0; j < s.n_fields; j++) { s.floating[j] = u64(slot + j); s.open[j] = u64((uint64_t)n_fields + slot + j); }
            }
        for (size_t b = 0; b < NB; b++) {
            LinkBusStat& bs = rep.buses[b];
            const uint64_t bb = 2ull * n_fields + 66ull * b;
            bs.tuples = u64(bb); bs.open_tuples = u64(bb + 1);
            for (uint32_t j = 0; j < bs.width; j++) { bs.open_in[j] = u64(bb + 2 + j); bs.open_records[j] = u64(bb + 34 + j); }
            n_open += bs.open_tuples;
        }
        rep.total_open = n_open;
        if (n_open) {
            const uint32_t n_rep = (uint32_t)std::min<uint64_t>(n_open, o.max_tuples), R = o.max_records_per_tuple, stride = 8 + plan.wmax + 2 * R;
            DBuf ukeys(&c, (size_t)(4 * n_open)), uvals(&c, (size_t)(2 * n_open)), out(&c, (size_t)n_rep * stride);
            vk::launch_la_select(st, ids, head_pos.data, tmask.data, n_groups, (uint32_t)n_open, (unsigned long long*)ukeys.data, uvals.data, counters.data);
            const int id_bytes[4] = {0, 8, 16, 24};  // keys are 32-bit record ids
            const int uh = vk::launch_ba_sort(st, (unsigned long long*)ukeys.data, uvals.data, n_open, sort_tmp.data, id_bytes, 4, 0);
            vk::launch_la_report(st, desc.data, ids, mask.data, head_pos.data, nrec.data, tmask.data, uvals.data + (uint64_t)uh * n_open, n_rep, R, out.data);
            c.check_launch("link_audit report");
            std::vector<uint32_t> w((size_t)n_rep * stride);
            c.download_small(w.data(), out.data, w.size() * 4);
            for (uint32_t t = 0; t < n_rep; t++) {
                const uint32_t* e = w.data() + (size_t)t * stride;
                const BusStat& bus = plan.buses.at(e[0]);
                LinkTuple lk;
                lk.is_global = bus.is_global; lk.bus_index = bus.bus_index; lk.mask = e[2];
                lk.fields.assign(e + 8, e + 8 + bus.width);
                lk.n_send = e[3]; lk.n_recv = e[4];
                for (uint32_t k = 0; k < e[1] && k < R; k++) {
                    const BusRecord r = plan.decode(e[8 + plan.wmax + 2 * k]);
                    lk.records.push_back(LinkRecord{r.chip, r.row, r.interaction, machine_.airs[r.chip].interactions[r.interaction].is_send() ? 1u : 0u, e[8 + plan.wmax + 2 * k + 1]});
                }
                rep.tuples.push_back(std::move(lk));
            }
        }
        pass.end(rep);
    }, [&] {
        return std::string("link_audit: the device pool cannot give the pass its scratch: 68 bytes for each of the " + std::to_string(n) + " (row, interaction) pairs (the bus audit's " +
                           std::to_string(BUS_AUDIT_BYTES_PER_SLOT) + ", 4 for the record mask, 4 for the tuple mask: " + std::to_string(68 * n) + " bytes), " + std::to_string(8 * tally_words) +
                           " bytes of tallies (16 per field, 528 per bus), " + std::to_string(wr_words * 4) + " bytes of interaction weight rows, 24 for each of the " + std::to_string(n_open) +
                           " open tuples, plus the working-layout copies of uploaded traces");
    });
    link_audit_finish(rep, o);
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- coverage audit (host/coverage_audit.hpp; kernels/coverage_audit.hip) ------------------------------------------------------------------
CoverageReport Prover::coverage_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed,
                                      const CoverageAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const CoverageAuditOpts o = coverage_audit_checked_opts(opts_in);
    const auto tr = audit_traces<ConstraintShape>("coverage_audit", main, preprocessed);
    std::vector<int> prep_slot;
    coverage_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, prep_slot);
    const size_t NC = machine_.airs.size();
    for (auto& air : machine_.airs) audit_refuse_constraints("coverage_audit", air);
    const uint32_t D = o.n_deltas;

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const hipStream_t st = pass.stream;

    CoverageReport rep;
    rep.deltas.assign(o.deltas, o.deltas + D);
    rep.chips.resize(NC);
    uint64_t scratch_words = 0, total_cells_all = 0, table_words = 0;
    audit_or_no_memory(st, [&] {
        // working-layout copies, as prove makes them (traces generated on the device are already column-major Montgomery)
        // per chip: the launch shape, its column flags and its slices of the scratch (u32 words; launch.hpp).  Zeroed: the workgroup tables
        // [GX][cells][4], detected [4] u64; written whole by merge and pack: counts [cells][2] u64, rows [cells][2], packed
        std::vector<vk::CovArgs> args(NC);
        std::vector<uint64_t> wg_at(NC, 0), det_at(NC, 0), cnt_at(NC, 0), row_at(NC, 0), pack_at(NC, 0), cap(NC, 0), flag_at(NC, 0);
        std::vector<uint32_t> flag_words;
        uint64_t zeroed = 0, packed = 0;
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine_.airs[i];
            vk::CovArgs& v = args[i];
            v = vk::CovArgs{};
            vk::MaArgs& a = v.m;
            const uint32_t K = air.program.num_asserts;
            v.M = (uint32_t)air.interactions.size();
            CoverageChipStat& cs = rep.chips[i];
            cs.width = air.width; cs.n_constraints = K; cs.n_interactions = v.M; cs.height = main[i]->height;
            cs.kills.assign((size_t)(K + v.M) * D, 0); cs.sole.assign((size_t)(K + v.M) * D, 0);
            const double evaluations = ma_evaluations(air, main[i]->height, D);
            rep.evaluations += evaluations;
            if (!air.width) continue;
            audit_chip_sizes(a, air, main[i]->height, fri_.interpret_air);
            pass.bind(a, main[i], audit_prep(preprocessed, prep_slot, i), prog_dev_[i]);
            a.iw = iw_dev_[i].data;
            a.evaluations = evaluations;
            a.D = D;
            for (uint32_t k = 0; k < D; k++) a.delta[k] = Fp::from_canonical(o.deltas[k]).v;
            try {
                vk::cov_shape(v, o.max_workgroups);
            } catch (const std::invalid_argument& e) {
                throw std::invalid_argument(std::string(e.what()) + " (chip " + air.name + ")");
            }
            const double baselines = a.K ? (a.n == 1 ? 1.0 : 2.0) * (double)a.n * (a.CY - 1) : 0;  // every column slice evaluates the baselines of its rows
            a.evaluations += baselines; rep.evaluations += baselines;
            const std::vector<uint32_t> fl = ma_column_flags(air);
            bool masks_ok = false;
            const std::vector<uint32_t> bm = ma_bus_masks(air, masks_ok);
            a.bus_walk = masks_ok ? 0u : 1u;
            flag_at[i] = flag_words.size();
            flag_words.insert(flag_words.end(), fl.begin(), fl.end());
            flag_words.insert(flag_words.end(), bm.begin(), bm.end());
            const uint64_t cells = vk::cov_cells(v);
            total_cells_all += cells;
            table_words += 4 * cells * v.GX;
            det_at[i] = zeroed; zeroed += 8;
            wg_at[i] = zeroed; zeroed += 4 * cells * v.GX;
            cap[i] = std::min<uint64_t>(cells, o.max_cells);
            cnt_at[i] = packed; packed += 4 * cells;  // u64s: every offset of this region is even
            row_at[i] = packed; packed += 2 * cells;
            pack_at[i] = packed; packed += vk::cov_packed_words(v, cap[i]);
        }
        scratch_words = zeroed + packed;
        if (flag_words.empty()) flag_words.push_back(0);
        DBuf flags(&c, flag_words);
        for (size_t i = 0; i < NC; i++) args[i].m.flags = flags.data + flag_at[i];
        c.check_launch("coverage_audit ingest");
        DBuf scratch(&c, (size_t)(scratch_words ? scratch_words : 1));
        uint32_t* const z = scratch.data;
        uint32_t* const pk = z + zeroed;
        // the device pass: everything from here to the last download is between the two events
        pass.begin();
        if (zeroed) VG_HIP_CHECK(hipMemsetAsync(z, 0, (size_t)zeroed * 4, st));
        for (size_t i = 0; i < NC; i++) {
            if (!args[i].m.width) continue;
            vk::launch_cov_audit(st, args[i], z + wg_at[i], reinterpret_cast<unsigned long long*>(z + det_at[i]));
            vk::launch_cov_merge(st, args[i], z + wg_at[i], reinterpret_cast<unsigned long long*>(pk + cnt_at[i]), pk + row_at[i]);
            vk::launch_cov_pack(st, args[i], reinterpret_cast<const unsigned long long*>(pk + cnt_at[i]), pk + row_at[i], (uint32_t)cap[i], pk + pack_at[i]);
        }
        c.check_launch("coverage_audit");
        // downloads: per chip its block (detected, the pack's head and sums), then the listed cells — never the cell table itself
        std::vector<uint32_t> w;
        for (size_t i = 0; i < NC; i++) {
            const vk::CovArgs& v = args[i];
            CoverageChipStat& cs = rep.chips[i];
            if (v.m.width) {
                uint32_t dw[8];
                c.download_small(dw, z + det_at[i], sizeof dw);
                for (uint32_t k = 0; k < D; k++) cs.detected[k] = ((uint64_t)dw[2 * k + 1] << 32) | dw[2 * k];
                const size_t TDD = (size_t)(v.m.K + v.M) * D;
                w.resize(2 + 4 * TDD);
                c.download_small(w.data(), pk + pack_at[i], w.size() * 4);
                const uint64_t nonzero = w[0];
                for (size_t k = 0; k < TDD; k++) { cs.kills[k] = ((uint64_t)w[3 + 4 * k] << 32) | w[2 + 4 * k]; cs.sole[k] = ((uint64_t)w[5 + 4 * k] << 32) | w[4 + 4 * k]; }
                rep.total_cells += nonzero;
                const uint64_t take = std::min<uint64_t>(std::min<uint64_t>(nonzero, cap[i]), o.max_cells - rep.cells.size());
                if (take) {
                    w.resize(8 * (size_t)take);
                    c.download_small(w.data(), pk + pack_at[i] + 2 + 4 * TDD, w.size() * 4);
                    for (size_t k = 0; k < take; k++) {
                        const uint32_t* e = &w[8 * k];
                        CoverageCell cell;
                        cell.chip = (uint32_t)i; cell.delta = e[0] % D; cell.column = (e[0] / D) % v.m.width; cell.detector = e[0] / D / v.m.width;
                        cell.kills = ((uint64_t)e[2] << 32) | e[1]; cell.sole = ((uint64_t)e[4] << 32) | e[3]; cell.first_row = e[5]; cell.first_sole_row = e[6];
                        rep.cells.push_back(cell);
                    }
                }
            }
            coverage_classify(cs, D);
        }
        rep.truncated = rep.total_cells > rep.cells.size();
        pass.end(rep);
    }, [&] {
        return std::string("coverage_audit: the device pool cannot give the pass its scratch: per chip 16 bytes per cell (detector, column, delta) and workgroup along its rows (" +
                           std::to_string(table_words * 4) + " bytes for this witness; max_workgroups bounds it), 24 per cell (" + std::to_string(total_cells_all) +
                           " cells for this machine), 16 per (detector, delta), 32 per listed cell (max_cells per chip at most): " + std::to_string(scratch_words * 4) +
                           " bytes in all, plus 12 per column of flags and the working-layout copies of uploaded traces");
    });
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- memory audit (host/memory_audit.hpp; kernels/memory_audit.hip) -------------------------------------------------------------------------
MemoryReport Prover::memory_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed, const MemoryAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const MemoryAuditOpts o = memory_audit_checked_opts(opts_in);
    const auto tr = audit_traces<BusShape>("memory_audit", main, preprocessed);
    std::vector<int> prep_slot;
    BusPlan bus_plan;
    const MemoryPlan plan = memory_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, prep_slot, o, &bus_plan);
    const uint64_t n = plan.n_slots;
    std::vector<uint32_t> entries;
    const std::vector<uint32_t> mt_words = memory_audit_mt(plan, entries);
    MemoryReport rep;
    memory_audit_header(rep, plan, o);

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const size_t NC = machine_.airs.size();
    const hipStream_t st = pass.stream;
    uint64_t n_live = 0;
    audit_or_no_memory(st, [&] {
        // only the chips that receive on the audited bus are read
        std::vector<const uint32_t*> mptr(NC, nullptr), pptr(NC, nullptr);
        std::vector<uint64_t> mstride(NC, 0), pstride(NC, 0);
        for (uint32_t i : entries) {
            const vk::DMatView v = pass.working(main[i]);
            mptr[i] = v.data; mstride[i] = v.stride;
            if (const DeviceTrace* p = audit_prep(preprocessed, prep_slot, i)) { const vk::DMatView pv = pass.working(p); pptr[i] = pv.data; pstride[i] = pv.stride; }
        }
        c.check_launch("memory_audit ingest");
        DBuf desc(&c, bus_audit_descriptor(machine_, bus_plan, mptr, mstride, pptr, pstride)), mt(&c, mt_words);
        const uint64_t na = n ? n : 1;
        // the totals of the keys pass and of the judge, u64 each, zeroed by one memset
        constexpr size_t TOT_WORDS = 2 * (vk::MM_KEY_TOT + vk::MM_JUDGE_TOT);
        DBuf keys2(&c, (size_t)(4 * na)), ids2(&c, (size_t)(2 * na)), sort_tmp(&c, vk::bus_audit_sort_scratch_words(na)), totals(&c, TOT_WORDS);
        unsigned long long* keys = (unsigned long long*)keys2.data;
        unsigned long long* tot = (unsigned long long*)totals.data;
        unsigned long long* cnt = tot + vk::MM_KEY_TOT;
        pass.begin();
        VG_HIP_CHECK(hipMemsetAsync(totals.data, 0, TOT_WORDS * 4, st));
        for (size_t e = 0; e < entries.size(); e++)
            vk::launch_mm_keys(st, desc.data, mt.data, (uint32_t)e, plan.chips[entries[e]].height, (uint32_t)plan.chips[entries[e]].receives.size(), keys, ids2.data, tot);
        c.check_launch("memory_audit keys");
        std::vector<uint32_t> tw(TOT_WORDS, 0);
        c.download_small(tw.data(), totals.data, 2 * vk::MM_KEY_TOT * 4);
        unsigned long long th[vk::MM_KEY_TOT], ch[vk::MM_JUDGE_TOT];
        for (uint32_t k = 0; k < vk::MM_KEY_TOT; k++) th[k] = audit_u64(tw, k);
        n_live = th[0];
        if (!n_live) {
            memory_audit_from_device(rep, plan, th, nullptr, nullptr, 0);
        } else {
            int shifts[8];
            const int n_shifts = memory_audit_shifts(th[1], th[2], n_live < n, shifts);
            const int half = vk::launch_ba_sort(st, keys, ids2.data, n, sort_tmp.data, shifts, n_shifts, 0);
            const uint32_t* ids = ids2.data + (uint64_t)half * n;
            const uint64_t nb = (n_live + 255) / 256;
            DBuf rec(&c, (size_t)(vk::MM_REC * n_live)), mark(&c, (size_t)n_live), block_before(&c, vk::memory_audit_scan_blocks(n_live)), table(&c, (size_t)nb);
            vk::launch_mm_gather(st, desc.data, mt.data, keys + (uint64_t)half * n, ids, n_live, n_live, rec.data, mark.data);
            vk::launch_mm_scan(st, mark.data, n_live, block_before.data);
            vk::launch_mm_judge(st, vk::MM_COUNT, rec.data, ids, mark.data, block_before.data, n_live, n_live, cnt, table.data, 0, nullptr);
            c.check_launch("memory_audit judge");
            c.download_small(tw.data(), totals.data, TOT_WORDS * 4);
            for (uint32_t k = 0; k < vk::MM_JUDGE_TOT; k++) ch[k] = audit_u64(tw, vk::MM_KEY_TOT + k);
            const uint64_t total = ch[6] + ch[7] + ch[8] + ch[9];
            const size_t listed = (size_t)std::min<uint64_t>(total, o.max_findings);
            std::vector<uint32_t> ow(listed * vk::MM_OUT);
            if (listed) {
                DBuf out(&c, ow.size());
                vk::launch_mm_judge(st, vk::MM_LIST, rec.data, ids, mark.data, block_before.data, n_live, n_live, nullptr, table.data, (uint32_t)listed, out.data);
                c.check_launch("memory_audit list");
                c.download_small(ow.data(), out.data, ow.size() * 4);
            }
            memory_audit_from_device(rep, plan, th, ch, ow.data(), listed);
        }
        pass.end(rep);
    }, [&] {
        return std::string("memory_audit: the device pool cannot give the pass its scratch: 24 bytes per slot (two halves of 8-byte keys and 4-byte ids) for each of the " +
                           std::to_string(n) + " (chip, receive, row) slots = " + std::to_string(24 * n) + " bytes, " + std::to_string(vk::bus_audit_sort_scratch_words(n ? n : 1) * 4) +
                           " bytes of digit tables, 32 bytes for each of the " + std::to_string(n_live) + " live records (7 words of record, 1 of mark) = " + std::to_string(32 * n_live) +
                           " bytes, 64 per listed finding, plus the working-layout copies of uploaded traces");
    });
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- program audit (host/program_audit.hpp; kernels/program_audit.hip) ----------------------------------------------------------------------
ProgramReport Prover::program_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed, const ProgramAuditOpts& o) {
    const auto t_host = Clock::now();
    const auto tr = audit_traces<BusShape>("program_audit", main, preprocessed);
    const ProgramPlan plan = program_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, o);
    ProgramReport rep;
    program_audit_header(rep, plan, o);
    const uint64_t H = plan.fetches, T = plan.table_rows, nbj = (H + 255) / 256, nbt = (T + 255) / 256;

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, 3);
    const hipStream_t st = pass.stream;
    size_t listed_hard = 0, listed_wrapped = 0, listed_ranges = 0;
    audit_or_no_memory(st, [&] {
        // only the fetching chip's main trace and the table chip's two traces are read
        vk::PgArgs a{};
        const vk::DMatView fv = pass.working(main[o.fetch_chip]);
        const vk::DMatView tv = o.table_chip == o.fetch_chip ? fv : pass.working(main[o.table_chip]);
        const vk::DMatView pv = pass.working(preprocessed[(size_t)plan.table_prep].second);
        c.check_launch("program_audit ingest");
        a.fmain = fv.data; a.fstride = fv.stride; a.H = H;
        a.tmain = tv.data; a.tmstride = tv.stride; a.tprep = pv.data; a.tpstride = pv.stride;
        a.T = (uint32_t)T; a.rom_len = plan.rom_len; a.n_fields = o.n_fields; a.pc_col = o.pc_col; a.key_col = o.key_col; a.mult_col = o.mult_col;
        a.lds_table = vk::program_audit_lds_table(o.n_fields, T) ? 1u : 0u;
        for (int j = 0; j < 8; j++) { a.field_cols[j] = o.field_cols[j]; a.table_cols[j] = o.table_cols[j]; }
        // the totals (u64) and the fetch counts behind them, zeroed by one memset; the workgroup tables are written whole by the counting passes
        constexpr size_t TOT_WORDS = 2 * vk::PG_TOT;
        DBuf zeroed(&c, TOT_WORDS + (size_t)T), tabs(&c, (size_t)(2 * nbj + 4 * nbt));
        unsigned long long* tot = (unsigned long long*)zeroed.data;
        uint32_t* counts = zeroed.data + TOT_WORDS;
        uint32_t* hard_tab = tabs.data;
        uint32_t* wrap_tab = tabs.data + nbj;
        uint32_t* ttabs = tabs.data + 2 * nbj;
        pass.begin();
        VG_HIP_CHECK(hipMemsetAsync(zeroed.data, 0, zeroed.words * 4, st));
        vk::launch_pg_hist(st, a.fmain + (uint64_t)a.pc_col * a.fstride, H, a.T, counts);
        vk::launch_pg_judge(st, a, vk::PG_COUNT, tot, hard_tab, wrap_tab, 0, 0, 0, nullptr, nullptr);
        vk::launch_pg_table(st, a, vk::PG_COUNT, counts, tot, ttabs, 0, 0, 0, nullptr, nullptr);
        c.check_launch("program_audit count");
        std::vector<uint32_t> tw(TOT_WORDS, 0);
        c.download_small(tw.data(), zeroed.data, TOT_WORDS * 4);
        unsigned long long th[vk::PG_TOT];
        for (uint32_t k = 0; k < vk::PG_TOT; k++) th[k] = audit_u64(tw, k);
        const uint64_t n_key = th[8], n_fetch = th[3] + th[4], n_mult = th[9];
        listed_hard = (size_t)std::min<uint64_t>(n_key + n_fetch + n_mult, o.max_findings);
        listed_wrapped = (size_t)std::min<uint64_t>(th[5], o.max_findings);
        listed_ranges = (size_t)std::min<uint64_t>(th[11], o.max_ranges);
        std::vector<uint32_t> ow((listed_hard + listed_wrapped) * vk::PG_OUT + 2 * listed_ranges);
        if (!ow.empty()) {
            DBuf out(&c, ow.size());
            uint32_t* out_wrap = out.data + listed_hard * vk::PG_OUT;
            uint32_t* ranges = out_wrap + listed_wrapped * vk::PG_OUT;
            // a section that starts at or past the limit lists nothing: its base is clamped to the limit
            const uint32_t hard_base = (uint32_t)std::min<uint64_t>(n_key, listed_hard), mult_base = (uint32_t)std::min<uint64_t>(n_key + n_fetch, listed_hard);
            if (listed_wrapped || hard_base < listed_hard)
                vk::launch_pg_judge(st, a, vk::PG_LIST, tot, hard_tab, wrap_tab, hard_base, (uint32_t)listed_hard, (uint32_t)listed_wrapped, out.data, out_wrap);
            if (listed_ranges || (listed_hard && (n_key || mult_base < listed_hard)))
                vk::launch_pg_table(st, a, vk::PG_LIST, counts, tot, ttabs, mult_base, (uint32_t)listed_hard, (uint32_t)listed_ranges, out.data, ranges);
            c.check_launch("program_audit list");
            c.download_small(ow.data(), out.data, ow.size() * 4);
        }
        program_audit_from_device(rep, th, ow.data(), listed_hard, listed_wrapped, ow.data() + (listed_hard + listed_wrapped) * vk::PG_OUT, listed_ranges);
        pass.end(rep);
    }, [&] {
        return std::string("program_audit: the device pool cannot give the pass its scratch: 4 bytes for each of the " + std::to_string(T) + " table rows (the fetch counts) = " +
                           std::to_string(4 * T) + " bytes, " + std::to_string(8 * vk::PG_TOT) + " bytes of totals, 4 bytes for each of the " + std::to_string(2 * nbj + 4 * nbt) +
                           " workgroup table entries (2 per 256 fetches, 4 per 256 table rows) = " + std::to_string(4 * (2 * nbj + 4 * nbt)) + " bytes, 80 per listed finding (" +
                           std::to_string(listed_hard + listed_wrapped) + "), 8 per listed range (" + std::to_string(listed_ranges) + "), plus the working-layout copies of uploaded traces");
    });
    rep.host_ms = ms_since(t_host);
    return rep;
}

// ---- arithmetic audit (host/arithmetic_audit.hpp; kernels/arithmetic_audit.hip) -------------------------------------------------------------
ArithmeticReport Prover::arithmetic_audit(const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed,
                                          const ArithmeticAuditOpts& opts_in) {
    const auto t_host = Clock::now();
    const ArithmeticAuditOpts o = arithmetic_audit_checked_opts(opts_in);
    const auto tr = audit_traces<BusShape>("arithmetic_audit", main, preprocessed);
    std::vector<int> prep_slot;
    BusPlan bus_plan;
    const ArithmeticPlan plan = arithmetic_audit_plan(machine_, tr.ms, tr.prep_chips, tr.ps, prep_slot, o, &bus_plan);
    ArithmeticReport rep;
    arithmetic_audit_header(rep, plan, o);
    const size_t NE = plan.entries.size();
    const uint64_t n = plan.n_slots;
    std::vector<uint32_t> block_base(NE, 0);
    uint64_t nb = 0;  // the workgroups of all entries, in slot order
    for (size_t e = 0; e < NE; e++) { block_base[e] = (uint32_t)nb; nb += (plan.entries[e].height + 255) / 256; }

    DeviceCtx& c = *ctx_;
    AuditPass pass(c, main.size() + preprocessed.size());
    const size_t NC = machine_.airs.size();
    const hipStream_t st = pass.stream;
    size_t listed_hard = 0, listed_soft = 0;
    audit_or_no_memory(st, [&] {
        // only the chips with an entry are read
        std::vector<const uint32_t*> mptr(NC, nullptr), pptr(NC, nullptr);
        std::vector<uint64_t> mstride(NC, 0), pstride(NC, 0);
        for (auto& e : plan.entries) {
            const size_t i = e.chip;
            if (mptr[i]) continue;
            const vk::DMatView v = pass.working(main[i]);
            mptr[i] = v.data; mstride[i] = v.stride;
            if (const DeviceTrace* p = audit_prep(preprocessed, prep_slot, i)) { const vk::DMatView pv = pass.working(p); pptr[i] = pv.data; pstride[i] = pv.stride; }
        }
        c.check_launch("arithmetic_audit ingest");
        DBuf desc(&c, bus_audit_descriptor(machine_, bus_plan, mptr, mstride, pptr, pstride));
        // per entry its u64 totals, zeroed by one memset; the verdicts and the two workgroup tables are written whole by the judge
        const size_t TOT_WORDS = 2 * (size_t)vk::AR_TOT * NE;
        DBuf totals(&c, TOT_WORDS), verdict(&c, (size_t)n), tabs(&c, (size_t)(2 * nb));
        unsigned long long* tot = (unsigned long long*)totals.data;
        uint32_t* hard_tab = tabs.data;
        uint32_t* soft_tab = tabs.data + nb;
        pass.begin();
        VG_HIP_CHECK(hipMemsetAsync(totals.data, 0, TOT_WORDS * 4, st));
        for (size_t e = 0; e < NE; e++) {
            const ArithmeticPlan::Entry& pe = plan.entries[e];
            vk::launch_ar_judge(st, desc.data, pe.chip, pe.interaction, pe.height, (uint32_t)pe.first_slot, block_base[e], verdict.data, tot + e * vk::AR_TOT, hard_tab, soft_tab);
        }
        c.check_launch("arithmetic_audit judge");
        std::vector<uint32_t> tw(TOT_WORDS, 0);
        c.download_small(tw.data(), totals.data, TOT_WORDS * 4);
        std::vector<unsigned long long> th(TOT_WORDS / 2);
        for (size_t k = 0; k < th.size(); k++) th[k] = audit_u64(tw, k);
        uint64_t n_hard = 0, n_soft = 0;
        for (size_t e = 0; e < NE; e++) { n_hard += th[e * vk::AR_TOT + 3] + th[e * vk::AR_TOT + 4] + th[e * vk::AR_TOT + 5]; n_soft += th[e * vk::AR_TOT + 6] + th[e * vk::AR_TOT + 7]; }
        listed_hard = (size_t)std::min<uint64_t>(n_hard, o.max_findings);
        listed_soft = (size_t)std::min<uint64_t>(n_soft, o.max_findings);
        std::vector<uint32_t> ow((listed_hard + listed_soft) * vk::AR_OUT);
        if (!ow.empty()) {
            DBuf out(&c, ow.size());
            vk::launch_ar_scan(st, hard_tab, soft_tab, nb);
            for (size_t e = 0; e < NE; e++) {
                const ArithmeticPlan::Entry& pe = plan.entries[e];
                const unsigned long long* t = th.data() + e * vk::AR_TOT;
                if (!(t[3] + t[4] + t[5] + t[6] + t[7])) continue;  // an entry without a finding lists nothing
                vk::launch_ar_list(st, desc.data, pe.chip, pe.interaction, pe.is_send, pe.height, (uint32_t)pe.first_slot, block_base[e], verdict.data, hard_tab, soft_tab,
                                   (uint32_t)listed_hard, (uint32_t)listed_soft, out.data, out.data + listed_hard * vk::AR_OUT);
            }
            c.check_launch("arithmetic_audit list");
            c.download_small(ow.data(), out.data, ow.size() * 4);
        }
        arithmetic_audit_from_device(rep, th.data(), vk::AR_TOT, ow.data(), listed_hard, listed_soft);
        pass.end(rep);
    }, [&] {
        return std::string("arithmetic_audit: the device pool cannot give the pass its scratch: 4 bytes for each of the " + std::to_string(n) + " (entry, row) slots (the verdicts) = " +
                           std::to_string(4 * n) + " bytes, " + std::to_string(8 * vk::AR_TOT) + " bytes of totals for each of the " + std::to_string(NE) + " entries, 8 bytes for each of the " +
                           std::to_string(nb) + " workgroups (two tables) = " + std::to_string(8 * nb) + " bytes, 96 per listed finding (" + std::to_string(listed_hard + listed_soft) +
                           "), plus the working-layout copies of uploaded traces");
    });
    rep.host_ms = ms_since(t_host);
    return rep;
}

}  // namespace vhost
