// qc_sp.h — tanh sum-product register kernel k_qc_sp_st for the 802.11n QC codes with Z <= 64 (see qc.hip for the
// lane layout).  Template only: qc.hip instantiates the fixed-count kernels, qc_es.hip the early-stop ones.
#pragma once
#include "qc_common.h"

#include <cstdint>

namespace ldpc {

#ifndef QC_SP_TPB_EARLY
#define QC_SP_TPB_EARLY 64  // tanh-SP early stop (k_qc_sp_st): 12.35 -> 13.97 M cw/s
#endif
template <bool EARLY>
constexpr int sp_tpb() { return EARLY ? QC_SP_TPB_EARLY : 256; }

// ---- tanh sum-product, register-resident (the reference's algorithm on-chip) ---------------------
// Messages in the variable frame, one VGPR per edge (c2v between iterations, v2c inside one), in log2 units.
// The operations are the oracle's (D, S) form and the generic kernels' (bp_vc.py:16-27, bp_cv.py:22-50
// evaluated as in common.h): per variable, v2c_t = copysign(exp2(-|fma(L, log2 e, S_t)|), .) with S_t the
// O(d) exclusive sum (vn_excl_sums); per check (cn_ds_row), each edge's log2(S/D) of the others' set, clamped
// to the reference's p clamp and to the caller's clamp; final z = fma(ascending sum, ln2/2, L/2).  Same device
// routines, so the values equal the generic GPU path's bit for bit.
#ifndef QC_SP_WAVES_PER_SIMD
#define QC_SP_WAVES_PER_SIMD 4
#endif
// Serial chains (TIE): each edge's exclusive sum / product chain starts after the previous edge's tanh / log
// output (an empty asm ties them): at most one chain in flight, instead of the scheduler interleaving a
// row's d chains and holding their partial products in registers.  Same operations, same order.  Fixed
// iteration count ((648,1/2) 6.45 -> 6.79 M cw/s, A/B) and the Z > 32 early-stop kernel (spill-free with
// it); the Z <= 32 early-stop kernel is 0.5 % slower with it.
#ifndef QC_SP_WAVES_PER_SIMD_EARLY
#define QC_SP_WAVES_PER_SIMD_EARLY 2  // 648 tanh-SP early stop 10.2 -> 12.1 M cw/s (A/B; 3 waves: 11.1)
#endif
// QC_SP_ADDR_MIN_USES (fixed iteration count): lane shifts used at least this many times per iteration get
// their ds_bpermute address computed once before the loop and held in a register (as k_qc_ms_ph), instead of
// a v_cndmask per rotation (the +4 rho folds into the ds_bpermute offset); 0 = off.  A/B (648,1/2) 50 it
// 12.73 -> 13.10 M cw/s, (1296,2/3) 20 it 15.43-15.63 -> 15.83-15.91 (4; 5: 13.00 / 15.61; 3 spills 51 VGPRs)
#ifndef QC_SP_ADDR_MIN_USES
#define QC_SP_ADDR_MIN_USES 4
#endif

// Early stop (EARLY): before iteration it >= 1, the hard decisions of z_it = 0.5 * (L + ascending sum of
// c2v) — the generic VN kernel's hb, same operations — are balloted per block column and rotated into
// each check's frame on the scalar unit (as k_qc_ms_st); a codeword whose syndrome is zero stops with
// iters_used = it and its z_it is parked in its own L region of LDS (its lanes keep computing for the
// wave's other codeword, discarded).  Bitwise equal to the generic path's early stop.
// PASS (the a == 1 rule, common.h cn_ds_row FIX): k_sp_zero_scan lists the waves whose codewords hold an
// exact-zero LLR (zlist: [0] = count, [1 ..] = wave ids, then one flag byte per wave, bit j = its codeword j —
// qc_sp_zflag); 1 = the plain
// loop for the unlisted waves (a listed one returns at once), 2 = the FIX loop for the listed waves (a small grid
// whose waves walk the list, on a second stream beside PASS 1: qc_sp_fork / qc_sp_join) — two kernels, so each
// keeps its own register allocation.
template <class C, bool EARLY, int PASS>
__device__ __forceinline__ void qc_sp_st_wave(int64_t wave_listed, const float* __restrict__ llr, int64_t B, int iters,
                                              float clamp, int flags, uint8_t* __restrict__ bits,
                                              float* __restrict__ soft, int32_t* __restrict__ iters_used,
                                              uint32_t* __restrict__ zlist) {
    constexpr int Z = C::Z, NB = C::NB, MB = C::MB, N = NB * Z;
    constexpr int NE = edge_off<C>(MB);
    static_assert(Z <= 64, "register kernel needs Z <= 64");
    constexpr int CPW = (Z <= 32) ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const int half = (CPW == 2) ? (lane >> 5) : 0;
    const int z = (CPW == 2) ? (lane & 31) : lane;
    const int64_t wave = PASS == 2 ? wave_listed : ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t cw = wave * CPW + half;
    const bool valid = (z < Z) && (cw < B);
    const int zb = lane_zb<Z, CPW>(z);
    const int base4 = (half * 32 + zb) * 4;
    const int base4m = base4 - 4 * Z;
    if constexpr (PASS == 1) {  // a wave whose codewords hold an exact-zero LLR: the a == 1 rule's pass decodes it
        if (wave * CPW < B && qc_sp_zflag(zlist, B)[__builtin_amdgcn_readfirstlane((int)wave)]) return;
    }
    // rotation addresses: "read lane (z + rho) mod Z of my group", one register per frequently used shift
    constexpr int ADDR_MIN = EARLY ? 0 : QC_SP_ADDR_MIN_USES;
    int ra[Z];
    static_for<1, Z>([&](auto rr) __attribute__((always_inline)) {
        constexpr int rho = decltype(rr)::value;
        if constexpr (ADDR_MIN > 0 && rot_uses<C>(rho) >= ADDR_MIN)
            ra[rho] = sel_lanes<wrap_mask<Z, CPW>(Z - rho)>(base4, base4m) + 4 * rho;
    });
    (void)ra;
    auto raddr = [&](auto rr) __attribute__((always_inline)) {
        constexpr int rho = decltype(rr)::value;
        if constexpr (ADDR_MIN > 0 && rot_uses<C>(rho) >= ADDR_MIN) return ra[rho];
        else return sel_lanes<wrap_mask<Z, CPW>(Z - rho)>(base4, base4m) + 4 * rho;
    };
    __shared__ float Ls[(sp_tpb<EARLY>() / 64) * CPW * N];
    const int lbase = ((threadIdx.x >> 6) * CPW + half) * N + z;
    const int lbase4 = lbase * 4;  // bytes (lds_reload)
    {
        const int64_t cwbase = valid ? cw * N : 0;
        const float vmask = valid ? 1.0f : 0.0f;
        static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
            constexpr int j = decltype(jj)::value;
            int t = z + C::PHI[j];
            t -= (t >= Z) ? Z : 0;
            const float x = llr[cwbase + j * Z + (valid ? t : 0)] * vmask;
            if (z < Z) Ls[lbase + j * Z] = -x;  // L = -llr (bp.py:47)
        });
    }
    float msg[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) msg[e] = 0.0f;
    const float cmax2 = sp_cmax2(clamp);  // check outputs in log2 units (common.h)
    constexpr uint64_t ACTIVE = lane_range_mask<Z, CPW>(0, Z);
    uint64_t done_groups = 0;  // lane masks of converged codewords (CPW == 2)
    int used_lo = iters, used_hi = iters;

    constexpr bool FIX = PASS == 2;
    constexpr bool TIE = !EARLY || Z > 32;  // serial chains (above)
    // the rule applies per codeword (common.h): this lane's codeword's bit of the unit's flag
    uint32_t fixm = 0x7fffffffu;
    if constexpr (FIX) fixm = ((qc_sp_zflag(zlist, B)[wave] >> half) & 1u) ? 0x7fffffffu : 0u;
    for (int it = 0; it < iters; ++it) {
        if constexpr (EARLY) {
            if (it > 0) {
                // z of column j from the c2v of the previous iteration (the epilogue's association)
                auto zcol = [&](auto jj) __attribute__((always_inline)) {
                    constexpr int j = decltype(jj)::value;
                    float S = 0.0f;
                    static_for<0, col_deg<C>(j)>([&](auto kk) __attribute__((always_inline)) {
                        S += msg[col_edge<C>(j, decltype(kk)::value)];
                    });
                    return sp_z(lds_reload<4 * j * Z, float>(Ls, lbase4), S);
                };
                // row by row with an early exit (as the min-sum kernels): the columns' hard decisions packed in
                // one register, then each row's parity from ballots of its columns' bits until no codeword of
                // the wave can still be satisfied
                static_assert(NB <= 32, "one hard-decision bit per block column in a 32-bit word");
                uint32_t hd = 0;
                static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
                    constexpr int j = decltype(jj)::value;
                    hd |= Num<float>::bit(zcol(jj)) ? (1u << j) : 0u;
                });
                constexpr uint64_t GA = lane_range_mask<Z, 1>(0, Z), GB = (CPW == 2) ? (GA << 32) : 0;
                uint64_t cand = (GA | GB) & ~done_groups;
                static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
                    constexpr int r = decltype(rr)::value;
                    if (cand) {
                        uint64_t par = 0;
                        static_for<0, C::DEG[r]>([&](auto tt) __attribute__((always_inline)) {
                            constexpr int t = decltype(tt)::value;
                            const uint64_t b = __ballot((hd >> C::COL[r][t]) & 1u) & ACTIVE;
                            par ^= rot_lanes<Z, CPW, C::SHR[r][t]>(b);
                        });
                        if (par & GA) cand &= ~GA;
                        if constexpr (CPW == 2) {
                            if (par & GB) cand &= ~GB;
                        }
                    }
                });
                const uint64_t unsat = (GA | GB) & ~cand;
                if constexpr (CPW == 1) {
                    if (unsat == 0) {  // the wave's codeword converged: its c2v are the output's
                        used_lo = it;
                        break;
                    }
                } else {
                    constexpr uint64_t G0 = lane_range_mask<Z, 1>(0, Z), G1 = G0 << 32;
                    const uint64_t newly = ((unsat & G0) ? 0 : G0) | ((unsat & G1) ? 0 : G1);
                    const uint64_t fresh = newly & ~done_groups;
                    if (fresh) {
                        if (fresh & G0) used_lo = it;
                        if (fresh & G1) used_hi = it;
                        if ((fresh >> lane) & 1ull) {
                            static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
                                constexpr int j = decltype(jj)::value;
                                const float zz = zcol(jj);
                                Ls[lbase + j * Z] = zz;  // parked z (its L is no longer needed)
                            });
                        }
                        done_groups |= fresh;
                        if (done_groups == (G0 | G1)) break;
                    }
                }
            }
        }
        // VC + tanh in the variable frame: c2v -> v2c in place
        if constexpr (!EARLY) __builtin_amdgcn_s_setprio(1);
        // L of column j + LPF is loaded before column j's chain (its address asm precedes the chain's ties),
        // so its LDS latency hides under the chains instead of a lgkmcnt(0) wait per column
        constexpr int LPF = EARLY ? 3 : 0;  // early stop (2 waves/SIMD): (648,1/2) 27.3-27.5 -> 28.1-28.5 M cw/s; fixed count: at its use
        float Lq[LPF > 0 ? LPF : 1];
        static_for<0, LPF>([&](auto qq) __attribute__((always_inline)) {
            constexpr int q = decltype(qq)::value;
            if constexpr (q < NB) Lq[q] = lds_reload<4 * q * Z, float>(Ls, lbase4);
        });
        static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
            constexpr int j = decltype(jj)::value;
            constexpr int dj = col_deg<C>(j);
            float L;
            if constexpr (LPF > 0) {
                L = Lq[j % LPF];
                if constexpr (j + LPF < NB) Lq[j % LPF] = lds_reload<4 * (j + LPF) * Z, float>(Ls, lbase4);
            } else {
                L = lds_reload<4 * j * Z, float>(Ls, lbase4);
            }
            vn_excl_sums<dj, TIE ? 1 : 0>(
                [&](auto kk) __attribute__((always_inline)) { return msg[col_edge<C>(j, decltype(kk)::value)]; },
                [&](auto kk, float S) __attribute__((always_inline)) {
                    constexpr int k = decltype(kk)::value;
                    constexpr int e = col_edge<C>(j, k);
                    msg[e] = vn_signed_a(sp_vn_arg(L, S));  // the (D, S) form's VC output (common.h)
                    if constexpr (TIE)
                        SP_TIE("+v"(msg[e]));  // next edge's chain starts after this output
                });
        });
        // CV in the check frame: gather v2c, exclusive products, log, clamp, scatter c2v back
        if constexpr (!EARLY) __builtin_amdgcn_s_setprio(0);
        static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
            constexpr int r = decltype(rr)::value;
            constexpr int d = C::DEG[r];
            constexpr int e0 = edge_off<C>(r);
            float g[d];
            static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                constexpr int s = C::SHR[r][t];
                if constexpr (s == 0) {
                    g[t] = msg[e0 + t];
                } else {
                    g[t] = bperm(raddr(std::integral_constant<int, s>{}), msg[e0 + t]);
                }
            });
            cn_ds_row<d, TIE ? 1 : 0, 0, DS_BLOCK, FIX>(g, cmax2, fixm);
            static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                constexpr int s = C::SHR[r][t];
                if constexpr (s == 0) {
                    msg[e0 + t] = g[t];
                } else {
                    msg[e0 + t] = bperm(raddr(std::integral_constant<int, Z - s>{}), g[t]);
                }
            });
        });
    }
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int zo = (CPW == 2) ? (tid & 31) : (tid & 63);
    const int64_t wo = PASS == 2 ? wave : (((int64_t)blockIdx.x * blockDim.x + tid) >> 6);
    const int64_t cwo = wo * CPW + ((CPW == 2) ? ((tid >> 5) & 1) : 0);
    const bool parked = EARLY && CPW == 2 && ((done_groups >> (tid & 63)) & 1ull);
    if (zo < Z && cwo < B) {
        static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
            constexpr int j = decltype(jj)::value;
            constexpr int dj = col_deg<C>(j);
            float S = 0.0f;
            static_for<0, dj>([&](auto kk) __attribute__((always_inline)) { S += msg[col_edge<C>(j, decltype(kk)::value)]; });
            const float zz = parked ? Ls[lbase + j * Z] : sp_z(Ls[lbase + j * Z], S);
            int t = zo + C::PHI[j];
            t -= (t >= Z) ? Z : 0;
            const int64_t o = cwo * N + j * Z + t;
            if (bits) bits[o] = (uint8_t)Num<float>::bit(zz);
            if (soft) soft[o] = (flags & LDPC_F_SOFT_Z) ? zz : 1.0f - 1.0f / (1.0f + Num<float>::exp_(-zz));
        });
        if (zo == 0 && iters_used) iters_used[cwo] = (CPW == 2 && ((tid >> 5) & 1)) ? used_hi : used_lo;
    }
}

template <class C, bool EARLY, int PASS = 1>
__global__ __launch_bounds__(256, EARLY ? QC_SP_WAVES_PER_SIMD_EARLY : QC_SP_WAVES_PER_SIMD) void k_qc_sp_st(const float* __restrict__ llr, int64_t B, int iters,
                                                                       float clamp, int flags, uint8_t* __restrict__ bits,
                                                                       float* __restrict__ soft, int32_t* __restrict__ iters_used,
                                                                       uint32_t* __restrict__ zlist) {
    if constexpr (PASS == 2) {  // the listed waves, walked by this grid's waves
        const uint32_t n = zlist[0];
        const uint32_t nw = gridDim.x * (blockDim.x >> 6);
        for (uint32_t i = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6); i < n; i += nw)
            qc_sp_st_wave<C, EARLY, 2>(__builtin_amdgcn_readfirstlane(zlist[1 + i]), llr, B, iters, clamp, flags, bits,
                                       soft, iters_used, zlist);
    } else {
        qc_sp_st_wave<C, EARLY, PASS>(0, llr, B, iters, clamp, flags, bits, soft, iters_used, zlist);
    }
}

}  // namespace ldpc
