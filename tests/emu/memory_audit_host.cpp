// Stand-alone host program for the sanitizers: fib(N) on the host VM (valida_amd/csrc/workload/basic_vm.hpp), its fourteen main traces and two
// preprocessed traces, then the host memory audit (valida_amd/csrc/host/memory_audit.hpp) over them under several limits; the same with one
// read of the mem trace tampered; then a captured nine-column `ram` chip with one receive over edge traces: one row, all dead, one address, every
// record its own address, keys at 0 and p - 1, malformed records, 300 findings.  Prints a few totals.  No GPU, no HIP runtime: the host headers
// compile with a plain C++ compiler.
//   memory_audit_host [N]
// Built by tests/test_memory_audit_cpu.py with AddressSanitizer + UBSan and run as a subprocess; exit status 0 = the audits ran to their end.
#include <cstdio>
#include <cstdlib>

#include "../../valida_amd/csrc/workload/basic_vm.hpp"
#include "../../valida_amd/csrc/host/memory_audit.hpp"

int main(int argc, char** argv) {
    const uint32_t n = argc > 1 ? (uint32_t)atoi(argv[1]) : 25u;
    try {
        vwork::BasicVm vm(vwork::fib_program(n));
        vm.run();
        std::vector<vwork::RowMajor> mt = vm.main_traces();
        const vwork::RowMajor pp = vm.program_preprocessed(), rp = vwork::BasicVm::range_preprocessed();
        std::vector<vhost::BusHostMatrix> main, prep;
        for (auto& t : mt) main.push_back({t.v.data(), t.height, t.width});
        prep.push_back({pp.v.data(), pp.height, pp.width});
        prep.push_back({rp.v.data(), rp.height, rp.width});
        const vhost::MachineDesc machine = vhost::MachineDesc::basic();
        const std::vector<int> prep_chips = {vchips::CHIP_PROGRAM, vchips::CHIP_RANGE};
        uint64_t words = 0;
        vhost::MemoryReport rep;
        for (uint32_t cap : {64u, 0u, 1u << 20}) {
            vhost::MemoryAuditOpts o;
            o.max_findings = cap;
            rep = vhost::memory_audit_host(machine, main, prep_chips, prep, o);
            words += rep.words().size();
        }
        printf("memory_audit_host: fib(%u): %llu live, %llu findings, %llu words\n", n, (unsigned long long)rep.live, (unsigned long long)rep.total_findings, (unsigned long long)words);
        // one read of the mem trace returns another byte: the first live row that is a read with a write before it
        vwork::RowMajor& mem = mt[vchips::CHIP_MEM];
        const vair::Interaction& it = machine.airs[vchips::CHIP_MEM].interactions[0];
        const int c_read = it.fields[0].terms[0].col, c_v3 = it.fields[7].terms[0].col;
        uint64_t tampered = 0;
        for (uint64_t r = mem.height / 2; r < mem.height && !tampered; r++)
            if (mem.v[r * mem.width + c_read] == 1) { mem.v[r * mem.width + c_v3] = (mem.v[r * mem.width + c_v3] + 1) % 256; tampered = r; }
        rep = vhost::memory_audit_host(machine, main, prep_chips, prep, vhost::MemoryAuditOpts{});
        printf("tampered: %llu finding%s, the first at row %u (tampered row %llu)\n", (unsigned long long)rep.total_findings, rep.total_findings == 1 ? "" : "s",
               rep.findings.empty() ? 0u : rep.findings[0].row, (unsigned long long)tampered);

        using V = vair::VirtualCol;
        vhost::MachineDesc ram;
        vair::Dag d;
        d.width = 9; d.prep_width = 0;
        vair::Interaction rx;
        for (int k = 0; k < 8; k++) rx.fields.push_back(V::single_main(k));
        rx.count = V::new_main({{0, 1}, {8, 1}}, 0); rx.bus_kind = vair::BusKind::Global; rx.bus_index = 2; rx.type = vair::InteractionType::GlobalReceive;
        ram.airs.push_back(vhost::MachineDesc::make_air_from_dag("ram", d, {rx}));
        uint64_t findings = 0;
        for (uint64_t h : {1ull, 2ull, 64ull, 512ull, 8192ull})
            for (int s = 0; s < 6; s++) {
                std::vector<uint32_t> t(h * 9, 0);
                for (uint64_t r = 0; r < h; r++) {
                    uint32_t* row = t.data() + r * 9;
                    const uint32_t is_read = s == 0 ? 0 : (uint32_t)(r & 1);
                    if (s == 1) continue;                                                             // all dead
                    row[0] = is_read; row[8] = 1 - is_read; row[1] = (uint32_t)r;
                    row[2] = s == 2 ? 40u : s == 3 ? (uint32_t)(8 * r) : s == 4 ? ((r & 2) ? vg::P - 1 : 0u) : 4u * (uint32_t)r;
                    row[7] = s == 5 ? 1 + (uint32_t)(r % 255) : (uint32_t)((r / 2) % 256);
                    if (s == 4) { row[1] = (r & 4) ? vg::P - 1 : 0u; row[3] = (uint32_t)(r % 3); row[4] = (r % 5) ? 0u : 256u; }
                }
                const vhost::MemoryReport e = vhost::memory_audit_host(ram, {{t.data(), h, 9}}, {}, {}, vhost::MemoryAuditOpts{});
                findings += e.total_findings;
                words += e.words().size();
            }
        printf("edge traces: %llu findings in all\n", (unsigned long long)findings);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "memory_audit_host: %s\n", e.what());
        return 1;
    }
}
