// Stand-alone host program for the sanitizers: fib(N) on the host VM (valida_amd/csrc/workload/basic_vm.hpp), its fourteen main traces and two
// preprocessed traces, then the host product audit (valida_amd/csrc/host/product_audit.hpp) over them; prints the report's word count and a few
// totals.  No GPU, no HIP runtime: the host headers compile with a plain C++ compiler.
//   product_audit_host [N]
// Built by tests/test_product_audit_cpu.py with AddressSanitizer + UBSan and run as a subprocess; exit status 0 = the audit ran to its end.
#include <cstdio>
#include <cstdlib>

#include "../../valida_amd/csrc/workload/basic_vm.hpp"
#include "../../valida_amd/csrc/host/product_audit.hpp"

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
        vhost::ProductAuditOpts o;
        o.max_entries = 1u << 20; o.max_rows_per_entry = 64; o.max_terms = 16;
        const vhost::ProductReport rep = vhost::product_audit_host(machine, main, {vchips::CHIP_PROGRAM, vchips::CHIP_RANGE}, prep, o);
        uint64_t pairs = 0, every = 0, never = 0, flat = 0;
        for (auto& c : rep.chips) { pairs += c.pairs; every += c.every; never += c.never; }
        for (auto& e : rep.entries) flat += e.flat_rows;
        printf("product_audit_host: fib(%u): %zu words, %llu relations of %llu pairs, %llu enforced on every row, %llu on none, %llu flat rows\n", n, rep.words().size(),
               (unsigned long long)rep.total_entries, (unsigned long long)pairs, (unsigned long long)every, (unsigned long long)never, (unsigned long long)flat);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "product_audit_host: %s\n", e.what());
        return 1;
    }
}
