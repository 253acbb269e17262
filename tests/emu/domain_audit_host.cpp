// Stand-alone host program for the sanitizers: fib(N) on the host VM (valida_amd/csrc/workload/basic_vm.hpp), its fourteen main traces and two
// preprocessed traces, then the host domain audit (valida_amd/csrc/host/domain_audit.hpp) over them under several options; then a captured
// three-column chip with one send (a bare field and a mixed one) over edge traces: one row, two rows, values at the class and bitmap-word
// boundaries, p - 1, and all 65536 narrow values.  Prints a few totals.  No GPU, no HIP runtime: the host headers compile with a plain C++
// compiler.
//   domain_audit_host [N]
// Built by tests/test_domain_audit_cpu.py with AddressSanitizer + UBSan and run as a subprocess; exit status 0 = the audits ran to their end.
#include <cstdio>
#include <cstdlib>

#include "../../valida_amd/csrc/workload/basic_vm.hpp"
#include "../../valida_amd/csrc/host/domain_audit.hpp"

int main(int argc, char** argv) {
    const uint32_t n = argc > 1 ? (uint32_t)atoi(argv[1]) : 25u;
    try {
        vwork::BasicVm vm(vwork::fib_program(n));
        vm.run();
        const std::vector<vwork::RowMajor> mt = vm.main_traces();
        const vwork::RowMajor pp = vm.program_preprocessed(), rp = vwork::BasicVm::range_preprocessed();
        std::vector<vhost::ConstraintHostMatrix> main, prep;
        for (auto& t : mt) main.push_back({t.v.data(), t.height, t.width});
        prep.push_back({pp.v.data(), pp.height, pp.width});
        prep.push_back({rp.v.data(), rp.height, rp.width});
        const vhost::MachineDesc machine = vhost::MachineDesc::basic();
        uint64_t words = 0, entries = 0;
        for (int variant = 0; variant < 4; variant++) {
            vhost::DomainAuditOpts o;
            o.max_entries = variant == 1 ? 0 : 1u << 20; o.max_rows_per_entry = variant == 2 ? 0 : 4096; o.max_bits = variant == 3 ? 8 : 16;
            if (variant == 3) { o.lookup_auto = 0; o.lookup_global_mask = 1ull << 3; o.chip_mask = 0x9; }
            const vhost::DomainReport rep = vhost::domain_audit_host(machine, main, {vchips::CHIP_PROGRAM, vchips::CHIP_RANGE}, prep, o);
            words += rep.words().size();
            if (variant == 0) entries = rep.total_entries;
        }
        printf("domain_audit_host: fib(%u): %llu words, fib%u entries %llu\n", n, (unsigned long long)words, n, (unsigned long long)entries);

        using V = vair::VirtualCol;
        vhost::MachineDesc edge;
        vair::Dag d;
        d.width = 3; d.prep_width = 0;
        vair::Interaction it;
        it.fields = {V::single_main(0), V::new_main({{0, 2}, {2, 1}}, 7)}; it.count = V::single_main(1); it.bus_kind = vair::BusKind::Global; it.bus_index = 0;
        it.type = vair::InteractionType::GlobalSend;
        edge.airs.push_back(vhost::MachineDesc::make_air_from_dag("edge", d, {it}));
        const uint32_t sets[8][2] = {{0, 0}, {0, 1}, {255, 255}, {256, 256}, {31, 32}, {65535, 65535}, {65536, 65536}, {vg::P - 1, vg::P - 1}};
        uint64_t distinct = 0;
        for (uint64_t h : {1ull, 2ull, 64ull, 256ull, 65536ull})
            for (int s = 0; s < 9; s++) {
                std::vector<uint32_t> t(h * 3);
                for (uint64_t r = 0; r < h; r++) { t[r * 3] = s < 8 ? sets[s][r & 1] : (uint32_t)((r * 40503u) & 0xffffu); t[r * 3 + 1] = r % 3 != 2; t[r * 3 + 2] = (uint32_t)r; }
                const vhost::DomainReport rep = vhost::domain_audit_host(edge, {{t.data(), h, 3}}, {}, {}, vhost::DomainAuditOpts{});
                distinct += rep.chips[0].cols[0].distinct;
                words += rep.words().size();
            }
        printf("edge traces: %llu distinct values in all\n", (unsigned long long)distinct);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "domain_audit_host: %s\n", e.what());
        return 1;
    }
}
