// Stand-alone host program for the sanitizers: fib(N) on the host VM (valida_amd/csrc/workload/basic_vm.hpp), its fourteen main traces and two
// preprocessed traces, then the host program audit (valida_amd/csrc/host/program_audit.hpp) over them under several limits; the same with
// the cpu trace and the program table tampered seven ways; then a captured two-chip machine over edge traces (heights 1 to 8192, one pc, a pc
// of p - 1, alternating fetched and unfetched words, 300 findings, one and eight fields) and the seven refusals.  Prints a few totals.  No
// GPU, no HIP runtime: the host headers compile with a plain C++ compiler.
//   program_audit_host [N]
// Built by tests/test_program_audit_cpu.py with AddressSanitizer + UBSan and run as a subprocess; exit status 0 = the audits ran to their end.
#include <cstdio>
#include <cstdlib>

#include "../../valida_amd/csrc/workload/basic_vm.hpp"
#include "../../valida_amd/csrc/host/program_audit.hpp"

int main(int argc, char** argv) {
    const uint32_t n = argc > 1 ? (uint32_t)atoi(argv[1]) : 25u;
    try {
        vwork::BasicVm vm(vwork::fib_program(n));
        vm.run();
        std::vector<vwork::RowMajor> mt = vm.main_traces();
        vwork::RowMajor pp = vm.program_preprocessed();
        const vwork::RowMajor rp = vwork::BasicVm::range_preprocessed();
        const vhost::MachineDesc machine = vhost::MachineDesc::basic();
        const std::vector<int> prep_chips = {vchips::CHIP_PROGRAM, vchips::CHIP_RANGE};
        auto audit = [&](const vhost::ProgramAuditOpts& o) {
            std::vector<vhost::BusHostMatrix> main, prep;
            for (auto& t : mt) main.push_back({t.v.data(), t.height, t.width});
            prep.push_back({pp.v.data(), pp.height, pp.width});
            prep.push_back({rp.v.data(), rp.height, rp.width});
            return vhost::program_audit_host(machine, main, prep_chips, prep, o);
        };
        const uint32_t rom_len = (uint32_t)vm.rom.size();  // the table's rows behind it are padding
        uint64_t words = 0;
        vhost::ProgramReport rep;
        for (uint32_t cap : {64u, 0u, 1u << 20}) {
            vhost::ProgramAuditOpts o;
            o.rom_len = rom_len; o.max_findings = cap; o.max_ranges = cap;
            rep = audit(o);
            words += rep.words().size();
        }
        printf("program_audit_host: fib(%u): %llu fetches, %llu of %u words fetched, %llu hard, %llu wrapped, %llu words\n", n, (unsigned long long)rep.fetches,
               (unsigned long long)rep.fetched_words, rep.rom_len, (unsigned long long)rep.hard(), (unsigned long long)rep.kinds[3], (unsigned long long)words);
        vwork::RowMajor& cpu = mt[vchips::CHIP_CPU];
        vwork::RowMajor& prog = mt[vchips::CHIP_PROGRAM];
        const uint64_t row = cpu.height > 100 ? 100 : cpu.height - 1;
        const char* names[7] = {"operand", "wrapped", "pc other word", "pc padding", "pc p - 1", "multiplicity", "key"};
        for (int k = 0; k < 7; k++) {
            uint32_t* cell = k < 2 ? &cpu.v[row * cpu.width + 4] : k < 5 ? &cpu.v[row * cpu.width + 1] : k == 5 ? &prog.v[3 * prog.width] : &pp.v[5 * pp.width];
            const uint32_t old = *cell;
            *cell = k == 0 ? (old + 7) % vg::P : k == 1 ? (uint32_t)(((uint64_t)old + vhost::PG_TWO32) % vg::P) : k == 2 ? (old + 9) % rom_len : k == 3 ? (uint32_t)pp.height - 1 : k == 4 ? vg::P - 1
                  : k == 5 ? (old + 1) % vg::P : 6u;
            vhost::ProgramAuditOpts o;
            o.rom_len = rom_len;
            rep = audit(o);
            printf("%s: %llu hard, %llu wrapped\n", names[k], (unsigned long long)rep.hard(), (unsigned long long)rep.kinds[3]);
            words += rep.words().size();
            *cell = old;
        }

        // the captured machine: a fetcher (pc, f0..f7) and a table (multiplicity; key, w0..w7)
        vhost::MachineDesc rom;
        vair::Dag df, dt;
        df.width = 9; df.prep_width = 0; dt.width = 1; dt.prep_width = 9;
        rom.airs.push_back(vhost::MachineDesc::make_air_from_dag("fetcher", df, {}));
        rom.airs.push_back(vhost::MachineDesc::make_air_from_dag("table", dt, {}));
        uint64_t findings = 0, ranges = 0;
        for (uint64_t h : {1ull, 2ull, 64ull, 512ull, 8192ull})
            for (uint64_t T : {1ull, 32ull, 1024ull})
                for (int s = 0; s < 4; s++)
                    for (uint32_t nf : {1u, 8u}) {
                        std::vector<uint32_t> f(h * 9, 0), m(T, 0), p(T * 9, 0);
                        for (uint64_t i = 0; i < T; i++) {
                            p[i * 9] = (uint32_t)i;
                            for (int j = 0; j < 8; j++) p[i * 9 + 1 + j] = (uint32_t)((i * 2654435761ull + j * 40503ull) % vg::P);
                        }
                        for (uint64_t r = 0; r < h; r++) {
                            const uint32_t pc = s == 0 ? 0u : s == 1 ? (uint32_t)(2 * r % T) : s == 2 ? (uint32_t)(r % T) : ((r % 3) ? (uint32_t)(r % T) : vg::P - 1);
                            f[r * 9] = pc;
                            if (pc < T) {
                                m[pc]++;
                                for (int j = 0; j < 8; j++) f[r * 9 + 1 + j] = p[(uint64_t)pc * 9 + 1 + j];
                                if (s == 2 && r < 300) f[r * 9 + 1] = (f[r * 9 + 1] + 1 + (r & 1 ? vhost::PG_TWO32 - 1 : 0u)) % vg::P;
                            }
                        }
                        vhost::ProgramAuditOpts o;
                        o.fetch_chip = 0; o.pc_col = 0; o.n_fields = nf; o.table_chip = 1; o.key_col = 0; o.mult_col = 0;
                        for (uint32_t j = 0; j < 8; j++) o.field_cols[j] = o.table_cols[j] = 1 + j;
                        o.max_findings = s == 2 ? 300 : 1; o.max_ranges = s == 1 ? 1u << 20 : 2;
                        const vhost::ProgramReport e = vhost::program_audit_host(rom, {{f.data(), h, 9}, {m.data(), T, 1}}, {1}, {{p.data(), T, 9}}, o);
                        findings += e.hard() + e.kinds[3];
                        ranges += e.unfetched_ranges;
                        words += e.words().size();
                    }
        printf("edge traces: %llu findings and %llu ranges in all\n", (unsigned long long)findings, (unsigned long long)ranges);

        std::vector<uint32_t> f(64 * 9, 0), m(32, 0), p(32 * 9, 0);
        m[0] = 64;
        int refused = 0;
        for (int k = 0; k < 7; k++) {
            vhost::ProgramAuditOpts o;
            o.fetch_chip = 0; o.pc_col = 0; o.table_chip = 1;
            uint64_t ph = 32;
            if (k == 0) o.pc_col = 9;         // a column outside its trace
            if (k == 1) o.table_chip = 0;     // a table chip without a preprocessed trace
            if (k == 2) ph = 16;              // a table whose main and preprocessed heights differ
            if (k == 3) o.rom_len = 33;       // rom_len above the table's height
            if (k == 4) o.n_fields = 9;
            if (k == 5) o.reserved = 1;
            if (k == 6) o.max_ranges = (1u << 20) + 1;
            try {
                (void)vhost::program_audit_host(rom, {{f.data(), 64, 9}, {m.data(), 32, 1}}, {1}, {{p.data(), ph, 9}}, o);
            } catch (const std::invalid_argument& e) {
                refused += std::string(e.what()).rfind("program_audit: ", 0) == 0;
            }
        }
        printf("refusals: %d of 7\n", refused);
        return refused == 7 ? 0 : 1;
    } catch (const std::exception& e) {
        fprintf(stderr, "program_audit_host: %s\n", e.what());
        return 1;
    }
}
