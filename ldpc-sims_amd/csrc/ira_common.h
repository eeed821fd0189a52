// ira_common.h — what the flooding (ira.hip) and the layered (ira_lay.hip) IRA kernels share: the table
// constants, the graph's tables on the host and as kernel arguments, and the 12-byte check state.
#pragma once
#include "common.h"

namespace ldpc {

constexpr int kIZ = 360;       // DVB-S2 lifting (normal and short frames)
constexpr int kIVS = 16;       // table stride: information-variable degree bound
constexpr int kICS = 24;       // table stride: information slots per check bound
constexpr int kIPS = 24;       // parity slots: kIPS (p_j) and kIPS + 1 (p_{j-1}); meta bits 0..25, argmin 27..31

struct IRASpec {
    int q = 0, G = 0, k = 0, n = 0, M = 0, E = 0, maxdv = 0, maxr = 0, device = 0;
    int32_t *vn = nullptr, *vdeg = nullptr, *cn = nullptr, *cdeg = nullptr;  // device tables
    // layered schedule (ira_lay.hip): cnl = cn's entries with the slot's role in its row (bits 17..18: 0 its group
    // meets the row once, 1 / 2 the first / second slot of a group that meets it twice; bits 19..23 the pair's rank
    // in the row), clay[a] = slots | pairs << 8.  lay_pairs: most pairs in one row, -1 when a group meets a row
    // three or more times.
    int32_t *cnl = nullptr, *clay = nullptr;
    int lay_pairs = 0;
};

// The tables are read-only for the whole decode: read through the constant address space so that every (uniform)
// table read is a scalar load.  As plain global pointers the compiler could not rule out that the kernels' own stores
// (app, states) alias them and read several rows with vector loads plus a wait and readfirstlane — one extra
// dependent round trip per task (round 6).
using cint32 = const __attribute__((address_space(4))) int32_t;
struct IRADev {
    cint32 *vn, *vdeg, *cn, *cdeg;
    int q, G, k, n, M;
};

// One check's state, 12 bytes read and written as one dwordx3: the two output magnitudes and the meta word
struct IraState {
    float m1, m2;
    uint32_t meta;
};
static_assert(sizeof(IraState) == 12, "one dwordx3 per check state");

__device__ __forceinline__ IraState ira_ld_i(const IraState* __restrict__ base, int64_t i) { return base[i]; }
__device__ __forceinline__ void ira_st_i(IraState* __restrict__ base, int64_t i, const IraState& s) { base[i] = s; }
__device__ __forceinline__ IraState ira_ld(const IraState* __restrict__ p) { return *p; }

// c2v of slot `slot` from a check state: the argmin slot gets mag2, every other mag1; sign bit from meta
__device__ __forceinline__ float ira_c2v(const IraState& st, int slot) {
    const float mag = ((st.meta >> 27) == (uint32_t)slot) ? st.m2 : st.m1;
    return u2f(f2u(mag) | ((st.meta << (31 - slot)) & 0x80000000u));
}

// Workgroup shape: kIraLanes threads, 6 waves over the 360 positions of one row; lanes past 360 repeat the last
// position and store nothing.
constexpr int kIraLanes = 384;

}  // namespace ldpc
