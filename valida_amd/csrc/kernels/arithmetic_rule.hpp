// The arithmetic audit's rule for ONE record, written once for the host twin (host/arithmetic_audit.hpp, which states the contract) and the device
// pass (kernels/arithmetic_audit.hip): plain u32 / u64 integer code, no dependency, no field arithmetic.  Every value handed in is canonical.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VGPU_AR_HD __host__ __device__ inline
#else
#define VGPU_AR_HD inline
#endif

namespace vk {

// The nineteen ALU opcodes of chips/basic_machine.hpp, by opcode - 100
enum : uint32_t {
    AR_ADD = 0, AR_SUB = 1, AR_MUL = 2, AR_DIV = 3, AR_LT = 4, AR_SHL = 5, AR_SHR = 6, AR_AND = 7, AR_OR = 8, AR_XOR = 9, AR_SDIV = 10, AR_NE = 11, AR_MULHU = 12, AR_SRA = 13,
    AR_MULHS = 14, AR_LTE = 15, AR_EQ = 16, AR_SLT = 17, AR_SLE = 18, AR_OPCODES = 19, AR_FIRST_OPCODE = 100
};
enum : uint32_t { AR_MALFORMED = 1, AR_UNDEFINED = 2, AR_WRONG_RESULT = 3, AR_SHIFT_QUOTIENT = 4, AR_ARITHMETIC_SHR = 5 };
// A verdict word: bits 0..2 the kind (0: none), bit 3 LIVE, bit 4 JUDGED, bits 5..9 the opcode index of a judged record, bit 10 a well-formed
// MULHS record whose signed high word differs from the unsigned one, bits 12..23 the mask (kind 1: the fields among 1..12 that are >= 256, bit
// j - 1 for field j; kinds 3, 4, 5: the differing bytes of z, bit j for z[j]) or the reason (kind 2).  A dead slot is 0.
enum : uint32_t { AR_LIVE = 8u, AR_JUDGED = 16u, AR_SIGN_MATTERS = 1u << 10, AR_INDEX_SHIFT = 5, AR_MASK_SHIFT = 12 };

VGPU_AR_HD uint32_t ar_kind(uint32_t word) { return word & 7u; }
VGPU_AR_HD uint32_t ar_index(uint32_t word) { return (word >> AR_INDEX_SHIFT) & 31u; }
VGPU_AR_HD uint32_t ar_mask(uint32_t word) { return (word >> AR_MASK_SHIFT) & 0xfffu; }
VGPU_AR_HD bool ar_is_hard(uint32_t word) { return ar_kind(word) >= AR_MALFORMED && ar_kind(word) <= AR_WRONG_RESULT; }
VGPU_AR_HD bool ar_is_soft(uint32_t word) { return ar_kind(word) >= AR_SHIFT_QUOTIENT; }

// bytes most significant first, as u32_of reads a Word (workload/basic_vm.hpp); every byte below 256
VGPU_AR_HD uint32_t ar_word(const uint32_t* b) { return (b[0] << 24) | (b[1] << 16) | (b[2] << 8) | b[3]; }
// x >> k with the sign replicated, k <= 31
VGPU_AR_HD uint32_t ar_sra(uint32_t x, uint32_t k) { return (x >> k) | ((x >> 31) ? ~(0xffffffffu >> k) : 0u); }

// The verdict of the record (count, opcode, f[0..11] = x[0..3], y[0..3], z[0..3]); *expected: the word the opcode computes (0 when there is none:
// a dead, other, malformed or undefined record).  No path divides by zero or INT_MIN by -1.
VGPU_AR_HD uint32_t ar_judge(uint32_t count, uint32_t opcode, const uint32_t* f, uint32_t* expected) {
    *expected = 0;
    if (!count) return 0;
    if (opcode < AR_FIRST_OPCODE || opcode >= AR_FIRST_OPCODE + AR_OPCODES) return AR_LIVE;
    const uint32_t idx = opcode - AR_FIRST_OPCODE;
    uint32_t word = AR_LIVE | AR_JUDGED | (idx << AR_INDEX_SHIFT), mask = 0;
    for (uint32_t j = 0; j < 12; j++)
        if (f[j] >= 256u) mask |= 1u << j;
    if (mask) return word | AR_MALFORMED | (mask << AR_MASK_SHIFT);
    const uint32_t x = ar_word(f), y = ar_word(f + 4), z = ar_word(f + 8);
    uint32_t reason = 0;
    if ((idx == AR_DIV || idx == AR_SDIV) && y == 0) reason = 1;
    else if (idx == AR_SDIV && x == 0x80000000u && y == 0xffffffffu) reason = 2;
    else if ((idx == AR_SHL || idx == AR_SHR || idx == AR_SRA) && y >= 32u) reason = 3;
    if (reason) return word | AR_UNDEFINED | (reason << AR_MASK_SHIFT);
    const int32_t sx = (int32_t)x, sy = (int32_t)y;
    uint32_t e = 0;
    switch (idx) {
        case AR_ADD: e = x + y; break;
        case AR_SUB: e = x - y; break;
        case AR_MUL: e = x * y; break;
        case AR_MULHU: case AR_MULHS: e = (uint32_t)(((uint64_t)x * y) >> 32); break;  // the reference zero-extends for MULHS too (core.rs:146-158)
        case AR_DIV: e = x / y; break;
        case AR_SDIV: e = (uint32_t)(sx / sy); break;
        case AR_SHL: e = x << y; break;
        case AR_SHR: e = x >> y; break;
        case AR_SRA: e = ar_sra(x, y); break;
        case AR_AND: e = x & y; break;
        case AR_OR: e = x | y; break;
        case AR_XOR: e = x ^ y; break;
        case AR_LT: e = x < y; break;
        case AR_LTE: e = x <= y; break;
        case AR_SLT: e = sx < sy; break;
        case AR_SLE: e = sx <= sy; break;
        case AR_NE: e = x != y; break;
        default: e = x == y; break;  // AR_EQ
    }
    *expected = e;
    if (idx == AR_MULHS && (uint32_t)(((uint64_t)((int64_t)sx * (int64_t)sy)) >> 32) != e) word |= AR_SIGN_MATTERS;
    if (z == e) return word;
    const uint32_t d = z ^ e;
    const uint32_t bytes = ((d >> 24) ? 1u : 0u) | (((d >> 16) & 255u) ? 2u : 0u) | (((d >> 8) & 255u) ? 4u : 0u) | ((d & 255u) ? 8u : 0u);
    uint32_t kind = AR_WRONG_RESULT;
    if (idx == AR_SDIV && (y & (y - 1u)) == 0 && z == ar_sra(x, (uint32_t)__builtin_ctz(y))) kind = AR_SHIFT_QUOTIENT;  // y != 0 here
    else if (idx == AR_SHR && z == ar_sra(x, y)) kind = AR_ARITHMETIC_SHR;
    return word | kind | (bytes << AR_MASK_SHIFT);
}

}  // namespace vk
