// The bus audit's record addressing on the device, shared by the kernels that walk records by id (kernels/bus_audit.hip; the link audit's join,
// kernels/link_audit.hip): the chip of a record id, its (row, interaction), its bus slot and its fields from the descriptor of
// host/bus_audit.hpp, and the full comparison of two records' padded tuples.
#pragma once
#include "launch.hpp"
#include "interactions.hpp"

namespace vk {

constexpr uint32_t BA_HDR = 4, BA_CHIP_WORDS = 12;  // host/bus_audit.hpp

struct BaChip {
    uint32_t first_id, height, M, table;
    const uint32_t* main; uint64_t mstride;
    const uint32_t* prep; uint64_t pstride;
};
__device__ __forceinline__ BaChip ba_chip(const uint32_t* __restrict__ d, uint32_t chip) {
    const uint32_t* e = d + BA_HDR + chip * BA_CHIP_WORDS;
    BaChip c;
    c.first_id = e[0]; c.height = e[1]; c.M = e[2]; c.table = e[3];
    c.main = (const uint32_t*)(((unsigned long long)e[5] << 32) | e[4]); c.mstride = e[6];
    c.prep = (const uint32_t*)(((unsigned long long)e[8] << 32) | e[7]); c.pstride = e[9];
    return c;
}
// the chip a record id belongs to: the last one whose first id is <= id (chips without interactions own no ids)
__device__ __forceinline__ uint32_t ba_chip_of(const uint32_t* __restrict__ d, uint32_t id) {
    const uint32_t nc = d[0];
    uint32_t c = 0;
    while (c + 1 < nc && d[BA_HDR + (c + 1) * BA_CHIP_WORDS] <= id) c++;
    return c;
}
struct BaRef { BaChip chip; uint32_t row, m, is_send, bus_slot, n_fields, pos; };  // pos: the first FIELD vcol
__device__ __forceinline__ BaRef ba_ref(const uint32_t* __restrict__ d, uint32_t id) {
    BaRef r;
    r.chip = ba_chip(d, ba_chip_of(d, id));
    const uint32_t off = id - r.chip.first_id;
    r.row = off / r.chip.M; r.m = off % r.chip.M;
    const uint32_t* ie = d + r.chip.table + 4 * r.m;
    r.is_send = ie[1]; r.bus_slot = ie[2]; r.n_fields = ie[3];
    r.pos = ie[0] + 2 + 2 * d[ie[0]];  // past the count vcol
    return r;
}
__device__ __forceinline__ uint32_t ba_next_field(const uint32_t* __restrict__ d, BaRef& r) {
    return eval_vcol(d, r.pos, r.chip.main, r.chip.mstride, r.chip.prep, r.chip.pstride, r.row).canonical();
}
__device__ bool ba_same_tuple(const uint32_t* __restrict__ d, uint32_t ida, uint32_t idb) {
    BaRef a = ba_ref(d, ida), b = ba_ref(d, idb);
    if (a.bus_slot != b.bus_slot) return false;
    const uint32_t n = a.n_fields > b.n_fields ? a.n_fields : b.n_fields;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t fa = j < a.n_fields ? ba_next_field(d, a) : 0u, fb = j < b.n_fields ? ba_next_field(d, b) : 0u;
        if (fa != fb) return false;
    }
    return true;
}

}  // namespace vk
