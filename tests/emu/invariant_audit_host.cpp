// Stand-alone host program for the sanitizers: fib(N) on the host VM (valida_amd/csrc/workload/basic_vm.hpp), its fourteen main traces and two
// preprocessed traces, then the host invariant audit (valida_amd/csrc/host/invariant_audit.hpp) over them; prints the report's word count and
// a few totals.  No GPU, no HIP runtime: the host headers compile with a plain C++ compiler.
//   invariant_audit_host [N]
// Built by tests/test_invariant_audit_cpu.py with AddressSanitizer + UBSan and run as a subprocess; exit status 0 = the audit ran to its end.
#include <cstdio>
#include <cstdlib>

#include "../../valida_amd/csrc/workload/basic_vm.hpp"
#include "../../valida_amd/csrc/host/invariant_audit.hpp"

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
        vhost::InvariantAuditOpts o;
        o.max_entries = 1u << 20; o.max_rows_per_entry = 64; o.max_terms = 16;
        const vhost::InvariantReport rep = vhost::invariant_audit_host(machine, main, {vchips::CHIP_PROGRAM, vchips::CHIP_RANGE}, prep, o);
        uint64_t relations = 0, every = 0, never = 0;
        for (auto& c : rep.chips) { relations += c.relations; every += c.every; never += c.never; }
        printf("invariant_audit_host: fib(%u): %zu words, %llu entries, %llu relations, %llu enforced on every row, %llu on none\n", n, rep.words().size(),
               (unsigned long long)rep.total_entries, (unsigned long long)relations, (unsigned long long)every, (unsigned long long)never);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "invariant_audit_host: %s\n", e.what());
        return 1;
    }
}
