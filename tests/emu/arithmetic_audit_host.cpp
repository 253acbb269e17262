// Stand-alone host program for the sanitizers: the host arithmetic audit (valida_amd/csrc/host/arithmetic_audit.hpp) over the BasicMachine's
// witness of fib(N) under several limits and sides, then over the captured one-chip `alu` machine (a receive of 13 bare columns with a count
// column) with the edge corpus planted at heights 1 to 512: every opcode over the extreme words, the shift amounts and divisors at which the
// operation is undefined (no path may divide by zero or INT_MIN by -1: UBSan would stop there), fields of 256 and p - 1, opcodes beside the
// range, the counts 0, 1, 2 and p - 1; and the refusals.  Prints a few totals.  No GPU, no HIP runtime: the host headers compile with a plain
// C++ compiler.
//   arithmetic_audit_host [N]
// Built by tests/test_arithmetic_audit_cpu.py with AddressSanitizer + UBSan and run as a subprocess; exit status 0 = the audits ran to their end.
#include <cstdio>
#include <cstdlib>

#include "../../valida_amd/csrc/workload/basic_vm.hpp"
#include "../../valida_amd/csrc/host/arithmetic_audit.hpp"

namespace {
vhost::MachineDesc alu_machine(int fields, bool send) {
    using V = vair::VirtualCol;
    vair::Interaction it;
    for (int k = 0; k < fields; k++) it.fields.push_back(V::single_main(k));
    it.count = V::single_main(13);
    it.bus_kind = vair::BusKind::Global; it.bus_index = 0; it.type = send ? vair::InteractionType::GlobalSend : vair::InteractionType::GlobalReceive;
    vair::Dag d;
    d.width = 14; d.prep_width = 0;
    vhost::MachineDesc m;
    m.airs.push_back(vhost::MachineDesc::make_air_from_dag("alu", d, {it}));
    return m;
}
void put(std::vector<uint32_t>& t, uint32_t opcode, uint32_t x, uint32_t y, uint32_t z, uint32_t count) {
    t.push_back(opcode);
    for (uint32_t v : {x, y, z})
        for (int j = 0; j < 4; j++) t.push_back((v >> (24 - 8 * j)) & 255u);
    t.push_back(count);
}
}  // namespace

int main(int argc, char** argv) {
    const uint32_t n = argc > 1 ? (uint32_t)atoi(argv[1]) : 25u;
    try {
        vwork::BasicVm vm(vwork::fib_program(n));
        vm.run();
        std::vector<vwork::RowMajor> mt = vm.main_traces();
        const vwork::RowMajor pp = vm.program_preprocessed();
        const vwork::RowMajor rp = vwork::BasicVm::range_preprocessed();
        const vhost::MachineDesc machine = vhost::MachineDesc::basic();
        const std::vector<int> prep_chips = {vchips::CHIP_PROGRAM, vchips::CHIP_RANGE};
        std::vector<vhost::BusHostMatrix> main, prep;
        for (auto& t : mt) main.push_back({t.v.data(), t.height, t.width});
        prep.push_back({pp.v.data(), pp.height, pp.width});
        prep.push_back({rp.v.data(), rp.height, rp.width});
        uint64_t words = 0;
        vhost::ArithmeticReport rep;
        for (uint32_t sides : {1u, 2u, 3u})
            for (uint32_t cap : {64u, 0u, 1u << 20}) {
                vhost::ArithmeticAuditOpts o;
                o.sides = sides; o.max_findings = cap;
                rep = vhost::arithmetic_audit_host(machine, main, prep_chips, prep, o);
                words += rep.words().size();
            }
        printf("arithmetic_audit_host: fib(%u): %llu live of %llu slots, %llu judged, %llu hard, %llu soft, %llu words\n", n, (unsigned long long)rep.live, (unsigned long long)rep.slots,
               (unsigned long long)rep.judged, (unsigned long long)rep.hard(), (unsigned long long)rep.soft(), (unsigned long long)words);

        // the edge corpus on the captured chip
        const uint32_t W[6] = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xffffffffu, 0x00ff00ffu};
        const uint32_t Y[11] = {0u, 1u, 2u, 31u, 32u, 255u, 256u, 0x7fffffffu, 0x80000000u, 0xffffffffu, 0x00ff00ffu};
        std::vector<uint32_t> rows;
        for (uint32_t opcode = 99; opcode <= 119; opcode++)
            for (uint32_t x : W)
                for (uint32_t y : Y)
                    for (uint32_t z : {0u, 1u, x >> (y & 31u), vk::ar_sra(x, y & 31u), vk::ar_sra(x, y ? (uint32_t)__builtin_ctz(y) : 0u), 0xffffffffu}) put(rows, opcode, x, y, z, 1);
        for (uint32_t opcode : {300u, vg::P - 1}) put(rows, opcode, 1, 2, 3, 1);
        for (uint32_t count : {0u, 1u, 2u, vg::P - 1}) put(rows, 102, 3, 5, 16, count);
        for (uint32_t j = 0; j < 12; j++)
            for (uint32_t v : {256u, vg::P - 1}) { put(rows, 100 + j, 0x01020304u, 5, 0, 1); rows[rows.size() - 14 + 1 + j] = v; }
        const uint64_t total = rows.size() / 14;
        const vhost::MachineDesc alu = alu_machine(13, false);
        uint64_t hard = 0, soft = 0, live = 0;
        for (uint64_t h : {1ull, 64ull, 256ull, 512ull})
            for (uint64_t first = 0; first + h <= total; first += h) {
                vhost::ArithmeticAuditOpts o;
                o.max_findings = (uint32_t)(first % 3 == 0 ? 0 : first % 3 == 1 ? 7 : 1u << 20);
                const vhost::ArithmeticReport e = vhost::arithmetic_audit_host(alu, {{rows.data() + first * 14, h, 14}}, {}, {}, o);
                hard += e.hard(); soft += e.soft(); live += e.live;
                words += e.words().size();
            }
        printf("edge corpus: %llu records; %llu live, %llu hard and %llu soft findings over the four heights\n", (unsigned long long)total, (unsigned long long)live,
               (unsigned long long)hard, (unsigned long long)soft);

        std::vector<uint32_t> t(64 * 14, 0);
        int refused = 0;
        for (int k = 0; k < 6; k++) {
            vhost::ArithmeticAuditOpts o;
            vhost::MachineDesc m = k == 0 ? alu_machine(12, false) : k == 1 ? alu_machine(13, true) : alu;
            if (k == 2) o.sides = 0;
            if (k == 3) o.sides = 4;
            if (k == 4) o.max_findings = (1u << 20) + 1;
            if (k == 5) o.reserved = 1;
            try {
                (void)vhost::arithmetic_audit_host(m, {{t.data(), 64, 14}}, {}, {}, o);
            } catch (const std::invalid_argument& e) {
                refused += std::string(e.what()).rfind("arithmetic_audit: ", 0) == 0;
            }
        }
        printf("refusals: %d of 6\n", refused);
        return refused == 6 && hard && soft ? 0 : 1;
    } catch (const std::exception& e) {
        fprintf(stderr, "arithmetic_audit_host: %s\n", e.what());
        return 1;
    }
}
