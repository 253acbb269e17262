// The bound-checking build of field.hpp's lazy sums (VG_LAZY_CHECK: a shadow 128-bit sum beside every 64-bit one; abort when the 64-bit sum would
// wrap, or when a high word has reached 2p where it is folded or finally reduced) as a stand-alone HOST program, compiled with
// -fsanitize=address,undefined and run as a subprocess by tests/test_lazy_sums_cpu.py.  Nothing of it is loaded into Python.
//   lazy_bounds_host <operands file> <results file>
// operands file: records { op, terms, n_items, n_items x words-per-item operand words (item-major) } of u32, ops and shapes as kernels/lazy_probe.hip
// has them (0 fold_hi, 1 ext_mul, 2 lin_dot, 3 ext_dot, 4 lin_dot_loop; here every length 1 .. 64 is accepted for ops 2 and 4, 1 .. 16 for op 3).
// results file: the results of every record in order, item-major.  Exit 0; a broken bound aborts with a line on stderr.
#define VG_LAZY_CHECK 1
#include "../../valida_amd/csrc/field.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace vg {
[[noreturn]] void lazy_check_failed(const char* what, uint64_t t) {
    fprintf(stderr, "lazy bound broken: %s (t = 0x%016llx)\n", what, (unsigned long long)t);
    abort();
}
}  // namespace vg

using vg::Ext5;
using vg::Fp;

static Ext5 ext(const uint32_t* w) { Ext5 e; for (int k = 0; k < 5; k++) e.c[k] = Fp::raw(w[k]); return e; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: lazy_bounds_host <operands> <results>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint32_t> in;
    uint32_t buf[4096];
    for (size_t got; (got = fread(buf, 4, 4096, f)) > 0;) in.insert(in.end(), buf, buf + got);
    fclose(f);
    std::vector<uint32_t> out;
    size_t at = 0;
    uint64_t items = 0;
    while (at < in.size()) {
        if (in.size() - at < 3) { fprintf(stderr, "truncated record header\n"); return 2; }
        const uint32_t op = in[at], terms = in[at + 1], n = in[at + 2];
        at += 3;
        size_t iw;
        if (op == 0 && terms == 0) iw = 2;
        else if (op == 1 && terms == 0) iw = 10;
        else if ((op == 2 || op == 4) && terms >= 1 && terms <= 64) iw = 6 * (size_t)terms;
        else if (op == 3 && terms >= 1 && terms <= 16) iw = 10 * (size_t)terms;
        else { fprintf(stderr, "unknown op %u / length %u\n", op, terms); return 2; }
        if ((in.size() - at) / iw < n) { fprintf(stderr, "truncated record\n"); return 2; }
        for (uint32_t i = 0; i < n; i++, at += iw, items++) {
            const uint32_t* w = in.data() + at;
            if (op == 0) {
                vg::LazyAcc a = vg::LazyAcc::zero();  // the fold through the accumulator, so that its check of the high word applies
                a.t = ((uint64_t)w[1] << 32) | w[0];
                a.shadow = a.t;
                a.fold();
                out.push_back((uint32_t)a.t);
                out.push_back((uint32_t)(a.t >> 32));
                continue;
            }
            Ext5 r;
            if (op == 1) r = ext(w) * ext(w + 5);
            else {
                vg::ExtAcc acc = vg::ExtAcc::zero();
                for (uint32_t c = 0; c < terms; c++) {
                    if (op == 3) acc.mac(ext(w + 10 * c), ext(w + 10 * c + 5));
                    else acc.mac(ext(w + 6 * c), Fp::raw(w[6 * c + 5]));
                }
                r = acc.reduce();
            }
            for (int k = 0; k < 5; k++) out.push_back(r.c[k].v);
        }
    }
    FILE* g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    if (!out.empty() && fwrite(out.data(), 4, out.size(), g) != out.size()) { perror("write"); return 2; }
    fclose(g);
    printf("%llu items within the bounds\n", (unsigned long long)items);
    return 0;
}
