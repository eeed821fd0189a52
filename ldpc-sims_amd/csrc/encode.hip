// encode.hip — systematic encoders on device (ldpc_encode): codeword = [info ; parity] with
// H * codeword = 0, bit for bit what codes.Encoder / codes.IRAEncoder compute.  Neither kernel multiplies by a
// generator matrix: both solve H's parity part, whose structure makes that linear-time and lane-parallel.
//
// k_qc_encode<C> — the compiled 802.11n codes.  With KB = NB - MB information block columns, block column KB
// holds three circulants (rows 0 and MB-1 with shift a, one middle row x with shift b) and columns KB+1 .. NB-1
// are the dual diagonal (shift 0 in rows i-1 and i of column KB+i).  u_j = information block j as a Z-vector,
// rot(v, s)[z] = v[(z + s) mod Z] (how qc_expand lifts a shift):
//     lam_r   = xor over the information edges (r, j) of rot(u_j, s_rj)
//     S       = xor over all rows of lam_r           (the dual diagonal cancels; column KB leaves rot(p_0, b))
//     p_0     = rot(S, -b)
//     p_1     = lam_0 ^ rot(p_0, a) = lam_0 ^ rot(S, a - b)
//     p_{i+1} = lam_i ^ p_i ^ (i == x ? rot(p_0, b) = S : 0),   i = 1 .. MB-2      (the last row is not needed)
// Dataflow: lane <-> lifting index z.  A lane packs its KB information bits into one word w(z) (bit j = column
// j), the wave's row w[0..Z) goes to LDS once, and lam_r(z) is assembled from bit j of w[(z + s_rj) mod Z]:
// one LDS read per DISTINCT shift, its address the lane base plus a compile-time immediate with one wrap
// select (qc_common.h sel_lanes).  All lam_r sit in one register (bit r); S is its parity; the one or two
// rotations of S go through the same LDS row; the recursion is a prefix xor over the bits of one word.
// Work split: Z <= 32 two codewords per wave in lane halves, Z = 54 one per wave, Z = 81 one per wave with each
// lane covering z and z + 64 in two registers — no workgroup barrier anywhere: a wave's LDS operations run in
// order, and every wave owns its row.  Idle lanes (z >= Z, or no codeword) load and store nothing and are
// never a rotation source: an active lane reads (z + s) mod Z < Z of its own group.
//
// k_ira_encode — staircase (IRA) graphs, from the CSR already on the device: p_c = p_{c-1} ^ s_c, s_c = xor of
// check c's information bits (columns < k).  One workgroup per codeword; a wave takes a contiguous range of
// 64-check blocks: each lane gathers its check's s_c, one ballot gives the block's 64 sums, six shift-xor steps
// on the scalar unit their prefix, the running parity across the wave's blocks stays in a scalar register.  LDS
// holds one prefix word per block and one parity per wave; after the workgroup's one barrier a wave xors the
// parities of the waves before it and every lane writes its p_c as a byte.
#include "qc_common.h"

#include <cstdint>

namespace ldpc {

// ---- 802.11n: structure of the parity part, derived (and checked) per code at compile time ---------------
template <class C>
struct EncTab {
    static constexpr int KB = C::NB - C::MB;
    struct Tab {
        int a, b, x;  // column KB: rows 0 and MB-1 with shift a, row x with shift b
        bool ok;
    };
    static constexpr Tab make() {
        Tab t{-1, -1, -1, true};
        int cnt = 0;
        for (int r = 0; r < C::MB; ++r)
            for (int s = 0; s < C::DEG[r]; ++s) {
                const int j = C::COL[r][s], sh = C::SH[r][s];
                if (j < KB) continue;
                if (j == KB) {
                    ++cnt;
                    if (r == 0) t.a = sh;
                    else if (r == C::MB - 1) t.ok = t.ok && sh == t.a;
                    else {
                        t.ok = t.ok && t.x < 0;
                        t.x = r;
                        t.b = sh;
                    }
                } else {
                    const int i = j - KB;  // dual diagonal: column KB + i in rows i-1 and i, shift 0
                    t.ok = t.ok && sh == 0 && (r == i - 1 || r == i);
                }
            }
        // 3 entries in column KB, 2 in each of the MB-1 diagonal columns
        int par = 0;
        for (int r = 0; r < C::MB; ++r)
            for (int s = 0; s < C::DEG[r]; ++s) par += C::COL[r][s] >= KB;
        t.ok = t.ok && cnt == 3 && t.a >= 0 && t.x > 0 && par == 3 + 2 * (C::MB - 1);
        return t;
    }
    static constexpr Tab T = make();
    // does any information edge carry shift s (the kernel reads the LDS row once per such shift)
    static constexpr bool shift_used(int s) {
        for (int r = 0; r < C::MB; ++r)
            for (int t = 0; t < C::DEG[r]; ++t)
                if (C::COL[r][t] < KB && C::SH[r][t] == s) return true;
        return false;
    }
};

// lanes of component c (z = lane + 64 c; two codewords per wave: z = lane & 31) that are active and whose
// rotation source z + s reaches Z
template <int Z, int CPW, int c>
constexpr uint64_t enc_wrap_mask(int s) {
    uint64_t m = 0;
    for (int l = 0; l < 64; ++l) {
        const int z = (CPW == 2) ? (l & 31) : l + 64 * c;
        if (z < Z && z + s >= Z) m |= 1ull << l;
    }
    return m;
}

template <class C>
__global__ __launch_bounds__(256) void k_qc_encode(const uint8_t* __restrict__ info, int64_t B,
                                                   uint8_t* __restrict__ cwout) {
    constexpr int Z = C::Z, NB = C::NB, MB = C::MB, KB = NB - MB, N = NB * Z, K = KB * Z;
    using E = EncTab<C>;
    static_assert(E::T.ok, "parity part is not [weight-3 column | dual diagonal]");
    static_assert(KB <= 31 && MB <= 16 && Z <= 128, "one word of information bits, one of row sums, two lanes' worth of z");
    constexpr int CPW = (Z <= 32) ? 2 : 1;       // codewords per wave
    constexpr int NC = (Z > 64) ? 2 : 1;         // lifting indices per lane: z = lane + 64 c
    constexpr int ROW = 64 * NC;                 // LDS words per wave
    constexpr int A = E::T.a, Bs = E::T.b, X = E::T.x;
    __shared__ uint32_t Rw[4 * ROW];
    const int lane = threadIdx.x & 63;
    const int half = (CPW == 2) ? (lane >> 5) : 0;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t cw = wave * CPW + half;
    uint32_t* const row = Rw + (threadIdx.x >> 6) * ROW;
    int z[NC], base4[NC];
    bool valid[NC];
    uint32_t w[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        z[c] = (CPW == 2) ? (lane & 31) : lane + 64 * c;
        valid[c] = z[c] < Z && cw < B;
        // rotation base: the lane's own slot; an idle lane reads from its group's slot 0 and never wraps
        base4[c] = 4 * (half * 32 + (z[c] < Z ? z[c] : 0));
        w[c] = 0;
        if (valid[c]) {
            const uint8_t* src = info + cw * K + z[c];
            static_for<0, KB>([&](auto jj) __attribute__((always_inline)) {
                constexpr int j = decltype(jj)::value;
                w[c] |= (uint32_t)(src[j * Z] & 1u) << j;
            });
        }
        row[lane + 64 * c] = w[c];
    }
    __builtin_amdgcn_wave_barrier();
    // value of slot (z + s) mod Z of the lane's group, for component c
    auto rot = [&](auto cc, auto ss) __attribute__((always_inline)) -> uint32_t {
        constexpr int c = decltype(cc)::value, s = decltype(ss)::value;
        constexpr uint64_t wm = enc_wrap_mask<Z, CPW, c>(s);
        int addr = base4[c];
        if constexpr (wm != 0) addr = sel_lanes<wm>(base4[c], base4[c] - 4 * Z);
        return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(row) + addr + 4 * s);
    };
    uint32_t lam[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) lam[c] = 0;
    static_for<0, NC>([&](auto cc) __attribute__((always_inline)) {
        constexpr int c = decltype(cc)::value;
        static_for<0, Z>([&](auto ss) __attribute__((always_inline)) {
            constexpr int s = decltype(ss)::value;
            if constexpr (E::shift_used(s)) {
                uint32_t x = w[c];
                if constexpr (s != 0) x = rot(cc, ss);
                static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
                    constexpr int r = decltype(rr)::value;
                    static_for<0, C::DEG[r]>([&](auto tt) __attribute__((always_inline)) {
                        constexpr int t = decltype(tt)::value;
                        if constexpr (C::COL[r][t] < KB && C::SH[r][t] == s) lam[c] ^= ((x >> C::COL[r][t]) & 1u) << r;
                    });
                });
            }
        });
    });
    // S = xor of all lam_r; its rotations go through the same row (the wave's LDS operations run in order: every
    // read of w above is served before these writes land)
    uint32_t S[NC], p0[NC], sa[NC];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        S[c] = __builtin_popcount(lam[c]) & 1u;
        if constexpr (Bs != 0 || A != Bs) row[lane + 64 * c] = S[c];
    }
    __builtin_amdgcn_wave_barrier();
    static_for<0, NC>([&](auto cc) __attribute__((always_inline)) {
        constexpr int c = decltype(cc)::value;
        constexpr int RP = (Z - Bs) % Z, RA = ((A - Bs) % Z + Z) % Z;
        p0[c] = S[c];
        if constexpr (RP != 0) p0[c] = rot(cc, std::integral_constant<int, RP>{});
        sa[c] = S[c];
        if constexpr (RA != 0) sa[c] = rot(cc, std::integral_constant<int, RA>{});
    });
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        // q: bit 1 = p_1 = lam_0 ^ rot(p_0, a); bit i+1 = lam_i ^ (i == x ? S : 0); p_i = xor of q's bits 1..i
        uint32_t q = ((lam[c] & ((1u << (MB - 1)) - 1u)) << 1) ^ (sa[c] << 1) ^ (S[c] << (X + 1));
        q ^= q << 1;
        q ^= q << 2;
        q ^= q << 4;
        q ^= q << 8;
        const uint32_t par = q | p0[c];  // bit 0 of q is clear
        if (valid[c]) {
            uint8_t* dst = cwout + cw * N + z[c];
            static_for<0, KB>([&](auto jj) __attribute__((always_inline)) {
                constexpr int j = decltype(jj)::value;
                dst[j * Z] = (uint8_t)((w[c] >> j) & 1u);
            });
            static_for<0, MB>([&](auto ii) __attribute__((always_inline)) {
                constexpr int i = decltype(ii)::value;
                dst[(KB + i) * Z] = (uint8_t)((par >> i) & 1u);
            });
        }
    }
}

template <class C>
static int launch_qc_encode(const uint8_t* info, int64_t B, uint8_t* cw, hipStream_t st) {
    constexpr int CPW = (C::Z <= 32) ? 2 : 1;
    const int64_t waves = (B + CPW - 1) / CPW;
    k_qc_encode<C><<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(info, B, cw);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "qc encode kernel launch: %s", hipGetErrorString(e));
    return LDPC_OK;
}

// each compiled 802.11n code has its own Z, and qc_lookup has matched every shift of the graph against its table
bool qc_encode_supports(const QCSpec* s) {
    const int z = qc_z(s);
    return s && (z == Wifi648_12::Z || z == Wifi1296_23::Z || z == Wifi1944_56::Z);
}

int qc_encode(const QCSpec* s, const uint8_t* info, int64_t B, uint8_t* cw, hipStream_t st) {
    switch (qc_z(s)) {
        case Wifi648_12::Z: return launch_qc_encode<Wifi648_12>(info, B, cw, st);
        case Wifi1296_23::Z: return launch_qc_encode<Wifi1296_23>(info, B, cw, st);
        case Wifi1944_56::Z: return launch_qc_encode<Wifi1944_56>(info, B, cw, st);
        default: return set_error(LDPC_EUNSUPPORTED, "no encoder for this QC code");
    }
}

// ---- IRA (staircase) -----------------------------------------------------------------------------------
constexpr int kIraEncThreads = 1024;
constexpr int kIraEncWaves = kIraEncThreads / 64;

__global__ __launch_bounds__(kIraEncThreads) void k_ira_encode(const int32_t* __restrict__ row_ptr,
                                                               const int32_t* __restrict__ col_idx, int m, int k,
                                                               const uint8_t* __restrict__ info,
                                                               uint8_t* __restrict__ cwout) {
    extern __shared__ uint64_t ira_lds[];  // [nblk] prefix words, then [kIraEncWaves] wave parities (uint32)
    const int nblk = (m + 63) >> 6;
    uint64_t* const pre = ira_lds;
    uint32_t* const wpar = reinterpret_cast<uint32_t*>(ira_lds + nblk);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t n = (int64_t)m + k;
    const uint8_t* const u = info + (int64_t)blockIdx.x * k;
    uint8_t* const out = cwout + (int64_t)blockIdx.x * n;
    // a wave's blocks: a contiguous range, so the running parity never leaves the wave until the barrier
    const int per = (nblk + kIraEncWaves - 1) / kIraEncWaves;
    const int b0 = wv * per, b1 = min(b0 + per, nblk);
    uint32_t carry = 0;
    for (int blk = b0; blk < b1; ++blk) {
        const int c = blk * 64 + lane;
        uint32_t s = 0;
        if (c < m) {
            // eight edges at a time, every load unconditional at a clamped address and masked afterwards: the
            // eight column loads, then the eight gathers, are in flight together (a serial loop waits on two
            // dependent round trips per edge)
            const int e1 = row_ptr[c + 1];
            for (int e = row_ptr[c]; e < e1; e += 8) {
                int v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = col_idx[min(e + i, e1 - 1)];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint32_t bit = u[min(v[i], k - 1)];
                    s ^= (e + i < e1 && v[i] < k) ? bit : 0u;
                }
            }
        }
        uint64_t pm = __ballot(s & 1u);  // lanes past m hold 0: bit 63 is the block's parity, ragged or not
        pm ^= pm << 1;
        pm ^= pm << 2;
        pm ^= pm << 4;
        pm ^= pm << 8;
        pm ^= pm << 16;
        pm ^= pm << 32;
        pm ^= carry ? ~0ull : 0ull;
        carry = (uint32_t)(pm >> 63);
        if (lane == 0) pre[blk] = pm;
    }
    if (lane == 0) wpar[wv] = carry;
    // the information bits pass through (bit 0 of each byte)
    for (int i = threadIdx.x; i < k; i += kIraEncThreads) out[i] = u[i] & 1u;
    __syncthreads();
    uint32_t before = 0;  // parity of every check before this wave's range
    for (int q = 0; q < wv; ++q) before ^= wpar[q];
    for (int blk = b0; blk < b1; ++blk) {
        const int c = blk * 64 + lane;
        if (c < m) out[k + c] = (uint8_t)(((uint32_t)(pre[blk] >> lane) & 1u) ^ before);
    }
}

size_t ira_encode_lds(int m) { return (size_t)((m + 63) / 64) * 8 + kIraEncWaves * 4; }

int ira_encode(const int32_t* row_ptr, const int32_t* col_idx, int m, int n, const uint8_t* info, int64_t B,
               uint8_t* cw, hipStream_t st) {
    const size_t lds = ira_encode_lds(m);
    if (lds > 64 * 1024) return set_error(LDPC_EUNSUPPORTED, "IRA encoder: %d checks exceed the workgroup's LDS", m);
    if (B > INT32_MAX) return set_error(LDPC_EINVAL, "IRA encoder: B = %lld exceeds the grid", (long long)B);
    k_ira_encode<<<(unsigned)B, kIraEncThreads, lds, st>>>(row_ptr, col_idx, m, n - m, info, cw);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "ira encode kernel launch: %s", hipGetErrorString(e));
    return LDPC_OK;
}

}  // namespace ldpc
