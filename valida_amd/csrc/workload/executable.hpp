// Loader of Valida executables: raw machine code or ELF, as the reference's `load_executable_file` reads them.
//
// Restated from (reference file:line):
//   load_executable_file / load_elf_object_file   elf/src/lib.rs:19-120
//   ProgramROM::from_machine_code                 machine/src/program.rs:181-196 (24-byte little-endian records, chunks_exact)
//
// Rules, as written there:
//   - first four bytes 7F 45 4C 46: ELF; anything else: raw machine code (initial pc 0, no static data; a trailing partial record is ignored)
//   - ELF sections count by sh_type and sh_flags alone, compared for equality: text = PROGBITS with ALLOC|EXECINSTR, data = PROGBITS with
//     ALLOC|WRITE, rodata = PROGBITS with ALLOC or 0x32 (ALLOC|MERGE|STRINGS); NOBITS (.bss) is ignored
//   - code image: the text bytes at offset sh_addr of a zero image of max(sh_addr + sh_size) bytes, read as machine code; initial pc =
//     min(sh_addr) / 24
//   - static data: each data / rodata section padded to a multiple of 4 bytes, cell sh_addr + 4i = Word([b0, b1, b2, b3]); a later section
//     overwrites an earlier one at the same address
// The file is untrusted: every offset, size and count is checked before it is used, and nothing is allocated at a size the file chose beyond
// MAX_EXE_INSTRUCTIONS instructions or MAX_EXE_STATIC_CELLS cells.  Refusals are std::invalid_argument with a message (the reference panics).
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>
#include "basic_vm.hpp"

namespace vwork {

constexpr uint64_t MAX_EXE_INSTRUCTIONS = (uint64_t)1 << 22;  // the largest cpu height this repository proves
constexpr uint64_t MAX_EXE_STATIC_CELLS = (uint64_t)1 << 22;

struct Executable {
    std::vector<InstructionWord> code;  // ProgramROM
    std::map<uint32_t, Word> data;      // static data, by address
    uint32_t initial_pc = 0;
};

namespace exe_detail {
inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }
[[noreturn]] inline void refuse(const std::string& why) { throw std::invalid_argument("executable: " + why); }
// [off, off + len) inside a file of n bytes, without overflow
inline bool inside(uint64_t off, uint64_t len, uint64_t n) { return off <= n && len <= n - off; }
}  // namespace exe_detail

// ProgramROM::from_machine_code: u32 opcode, i32 operands[5], little-endian; a trailing partial record is ignored
inline std::vector<InstructionWord> from_machine_code(const uint8_t* p, uint64_t n) {
    using namespace exe_detail;
    const uint64_t count = n / (6 * 4);
    if (count > MAX_EXE_INSTRUCTIONS)
        refuse("machine code of " + std::to_string(count) + " instructions is above the limit of " + std::to_string(MAX_EXE_INSTRUCTIONS) + " instructions");
    std::vector<InstructionWord> out(count);
    for (uint64_t i = 0; i < count; i++) {
        const uint8_t* r = p + 24 * i;
        out[i].opcode = le32(r);
        for (int k = 0; k < 5; k++) out[i].ops[k] = (int32_t)le32(r + 4 + 4 * k);
    }
    return out;
}

inline Executable load_elf(const uint8_t* p, uint64_t n) {
    using namespace exe_detail;
    constexpr uint32_t SHT_PROGBITS = 1;
    constexpr uint64_t SHF_WRITE = 1, SHF_ALLOC = 2, SHF_EXECINSTR = 4;
    if (n < 16) refuse("truncated ELF identification (" + std::to_string(n) + " bytes)");
    const uint8_t cls = p[4], data = p[5];
    if (cls != 1 && cls != 2) refuse("ELF class " + std::to_string(cls) + " is neither ELFCLASS32 nor ELFCLASS64");
    if (data != 1) refuse(data == 2 ? std::string("big-endian ELF is not supported") : "ELF data encoding " + std::to_string(data) + " is not little-endian");
    const bool is64 = cls == 2;
    const uint64_t ehsize = is64 ? 64 : 52, want_shentsize = is64 ? 64 : 40;
    if (n < ehsize) refuse("truncated ELF header (" + std::to_string(n) + " of " + std::to_string(ehsize) + " bytes)");
    const uint64_t shoff = is64 ? le64(p + 0x28) : le32(p + 0x20);
    const uint16_t shentsize = le16(p + (is64 ? 0x3A : 0x2E)), shnum = le16(p + (is64 ? 0x3C : 0x30));
    if (shoff != 0 && shnum == 0) refuse("extended section numbering (e_shnum = 0 with a section table) is not supported");
    if (shnum != 0 && shentsize != want_shentsize)
        refuse("section header size " + std::to_string(shentsize) + " is not " + std::to_string(want_shentsize));
    if (shnum != 0 && !inside(shoff, (uint64_t)shnum * want_shentsize, n))
        refuse("section header table (" + std::to_string(shnum) + " entries at offset " + std::to_string(shoff) + ") lies outside the file of " +
               std::to_string(n) + " bytes");
    struct Sec { uint64_t addr, size, offset; };
    std::vector<Sec> text, datas;
    for (uint16_t s = 0; s < shnum; s++) {
        const uint8_t* h = p + shoff + (uint64_t)s * want_shentsize;
        const uint32_t type = le32(h + 4);
        const uint64_t flags = is64 ? le64(h + 8) : le32(h + 8);
        const uint64_t addr = is64 ? le64(h + 16) : le32(h + 12), offset = is64 ? le64(h + 24) : le32(h + 16), size = is64 ? le64(h + 32) : le32(h + 20);
        if (type != SHT_PROGBITS) continue;
        const bool is_data = flags == (SHF_ALLOC | SHF_WRITE), is_rodata = flags == SHF_ALLOC || flags == 0x32, is_text = flags == (SHF_ALLOC | SHF_EXECINSTR);
        if (!is_data && !is_rodata && !is_text) continue;
        if (!inside(offset, size, n))
            refuse("section " + std::to_string(s) + ": data (" + std::to_string(size) + " bytes at offset " + std::to_string(offset) + ") lies outside the file of " +
                   std::to_string(n) + " bytes");
        (is_text ? text : datas).push_back({addr, size, offset});
    }
    if (text.empty()) refuse("no text section (PROGBITS with flags ALLOC|EXECINSTR)");
    Executable e;
    uint64_t code_size = 0, min_addr = UINT64_MAX;
    const uint64_t max_bytes = MAX_EXE_INSTRUCTIONS * 24 + 23;  // the largest image whose chunks_exact stays within the limit
    for (const Sec& t : text) {
        if (t.addr > max_bytes || t.size > max_bytes - t.addr)
            refuse("code image (text ends at byte " + std::to_string(t.addr) + " + " + std::to_string(t.size) + ") is above the limit of " +
                   std::to_string(MAX_EXE_INSTRUCTIONS) + " instructions");
        code_size = std::max(code_size, t.addr + t.size);
        min_addr = std::min(min_addr, t.addr);
    }
    std::vector<uint8_t> image(code_size, 0);
    for (const Sec& t : text) if (t.size) std::memcpy(image.data() + t.addr, p + t.offset, t.size);
    e.code = from_machine_code(image.data(), image.size());
    e.initial_pc = (uint32_t)(min_addr / 24);
    uint64_t cells = 0;
    for (const Sec& d : datas) {
        const uint64_t nc = (d.size + 3) / 4;
        cells += nc;
        if (cells > MAX_EXE_STATIC_CELLS)
            refuse("static data of more than " + std::to_string(MAX_EXE_STATIC_CELLS) + " cells is above the limit of " + std::to_string(MAX_EXE_STATIC_CELLS) + " cells");
        if (nc && (d.addr > UINT32_MAX || 4 * (nc - 1) > UINT32_MAX - d.addr))
            refuse("data section at address " + std::to_string(d.addr) + " of " + std::to_string(d.size) + " bytes overflows the 32-bit address space");
        for (uint64_t i = 0; i < nc; i++) {
            Word w{{0, 0, 0, 0}};
            for (uint64_t b = 0; b < 4 && 4 * i + b < d.size; b++) w.b[b] = p[d.offset + 4 * i + b];
            e.data[(uint32_t)(d.addr + 4 * i)] = w;
        }
    }
    return e;
}

// load_executable_file (elf/src/lib.rs:19-30)
inline Executable load_executable(const uint8_t* p, uint64_t n) {
    if (n >= 4 && p[0] == 0x7F && p[1] == 0x45 && p[2] == 0x4C && p[3] == 0x46) return load_elf(p, n);
    Executable e;
    e.code = from_machine_code(p, n);
    return e;
}

}  // namespace vwork
