// Stand-alone host program for the sanitizers: fib(N) on the host VM (valida_amd/csrc/workload/basic_vm.hpp), its fourteen main traces and two
// preprocessed traces, then the host step audit (valida_amd/csrc/host/step_audit.hpp) over them; prints the report's word count and a few
// totals.  No GPU, no HIP runtime: the host headers compile with a plain C++ compiler.
//   step_audit_host [N]
// Built by tests/test_step_audit_cpu.py with AddressSanitizer + UBSan and run as a subprocess; exit status 0 = the audit ran to its end.
#include <cstdio>
#include <cstdlib>

#include "../../valida_amd/csrc/workload/basic_vm.hpp"
#include "../../valida_amd/csrc/host/step_audit.hpp"

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
        vhost::StepAuditOpts o;
        o.max_entries = 1u << 20; o.max_rows_per_entry = 64;
        const vhost::StepReport rep = vhost::step_audit_host(machine, main, {vchips::CHIP_PROGRAM, vchips::CHIP_RANGE}, prep, o);
        uint64_t exact = 0, loose = 0, bus = 0;
        for (auto& c : rep.chips) { exact += c.exact_cells; loose += c.loose_cells; bus += c.bus_detected; }
        printf("step_audit_host: fib(%u): %zu words, %llu entries, %llu loose cells, %llu exact cells, %llu bus-detected\n", n, rep.words().size(),
               (unsigned long long)rep.total_entries, (unsigned long long)loose, (unsigned long long)exact, (unsigned long long)bus);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "step_audit_host: %s\n", e.what());
        return 1;
    }
}
