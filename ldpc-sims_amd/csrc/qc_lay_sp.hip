// qc_lay_sp.hip — layered (row-serial) tanh sum-product for the 802.11n (1944,5/6) code, Z = 81 (gfx950).
//
// The schedule (include/ldpc_abi.h LDPC_F_LAYERED with LDPC_ALGO_TANH_SP): the checks run in
// ascending order within a sweep, each on the posteriors its predecessors of the same sweep have updated:
//   s_e = APP_v - c2v[e];  c2v[e] = the tanh rule over the check's other s;  APP_v = s_e + c2v[e].
// Every 802.11n block is one circulant, so the 81 checks of a base row touch disjoint variables and run in
// parallel with the serial result.
//
// Dataflow (the unit of the sliced flooding kernels, qc_sl_sp.h: one workgroup of S = 3 waves decodes two
// codewords, one per lane half, 27 active lanes per half; wave k owns check positions p = 3 l + k):
//   * c2v: one VGPR per edge (80) in the check frame for the whole decode.  It never moves.
//   * APP: in LDS for the whole decode, natural order [half][column][variable], in log2 units (L * log2 e on the
//     way in, z = APP * ln 2 / 2 on the way out), updated in place: a layer gathers each edge's APP from slot
//     (p + shift) mod 81 of its column, runs the row, and scatters s + c2v_new to the address it gathered from.
//     A slot is touched by exactly one lane per layer, so one workgroup barrier per layer orders everything:
//     4 per sweep, where the flooding kernel k_qc_sp_rs spends 2 per iteration on twice the iterations.
//     2 x 24 x 81 x 4 B = 15.6 KB per unit (k_qc_sp_rs: 31 KB), so LDS does not bound the occupancy.
//   * addressing: natural order with a wrap select.  The shift is a compile-time constant, so an edge's address is
//     (p >= 81 - shift ? base - 4 * 81 : base) + an immediate: one v_cmp and one v_cndmask per access (formed
//     for the gather and again for the scatter: 4 VALU per edge and layer, against a row that spends about 15 VALU
//     and three transcendentals per edge); the array starts one row into the allocation so that the wrapped base
//     is never negative.  The 27 reads of a half-wave are 3 words apart: distinct banks until the wrap.
//   * idle lanes (l >= 27) repeat the addresses of their wave's lane 0 (a broadcast, qc_common.h idle_alias) and
//     never store; the empty half of an odd batch decodes zeros in its own rows.
//   * the load and the stores run over the workgroup's 192 threads in element order (coalesced), not in the
//     layers' lane order: LDS is the only place APP lives, so nothing needs to agree with the check frame.
//   * early stop, the all-rows form: after the sweep's last barrier every check lane XORs the hard decisions of
//     its edges (a ballot per edge, the parity as a lane mask on the scalar unit), the three waves pool one flag
//     per (wave, half) through LDS behind a fifth barrier, and a stopped half stops storing.  The loop exit is a
//     decision on the pooled flags, so every wave takes it in the same sweep.
// The plain (D, S) form only (common.h): no a == 1 pass.  A codeword with exact-zero LLRs is decoded like any
// other; its messages may sit within 2^-23 (log2 units) of 0 where the ideal value is 0.
#include "qc_common.h"

#include <cstdint>

namespace ldpc {

#ifndef QC_LSP_WAVES_PER_SIMD
#define QC_LSP_WAVES_PER_SIMD 3  // <= 168 VGPRs: 80 c2v + a d = 20 row's s, a and (D, S) sets
#endif
// Register plan, A/B on config [2]'s input (B = 32,768, 25 sweeps, both spill-free at <= 168 VGPRs): rows in one
// block of 20 edges with the scatter addresses formed again after the row (164 VGPRs), 3.86 ms per launch; rows in
// two blocks of 10 with the gather's addresses kept (163 VGPRs), 3.95 ms.  With one block AND kept addresses the
// kernel spills 24-33 VGPRs.
#ifndef QC_LSP_DS_BLOCK
#define QC_LSP_DS_BLOCK 20  // check rows in one block (cn_ds_row), as k_qc_sp_rs
#endif

template <class C, bool EARLY>
__global__ __launch_bounds__(C::S * 64) __attribute__((amdgpu_waves_per_eu(QC_LSP_WAVES_PER_SIMD)))
void k_qc_sp_lay(const float* __restrict__ llr, int64_t B, int iters, float clamp, int flags,
                 uint8_t* __restrict__ bits, float* __restrict__ soft, int32_t* __restrict__ iters_used) {
    constexpr int Z = C::Z, S = C::S, ZL = Z / S, NB = C::NB, MB = C::MB, N = NB * Z, TPB = S * 64;
    constexpr int NE = edge_off<C>(MB);
    static_assert(S > 1 && Z % S == 0 && ZL <= 32, "sliced unit: Z = S * ZL, ZL <= 32");
    static_assert(4 * (N + Z) < 65536, "column and shift ride in the 16-bit ds offset");
    __shared__ float X[Z + 2 * N];  // APP (log2 units) at X[Z + half * N + column * Z + variable]
    __shared__ uint32_t Fl[EARLY ? 2 * S : 1];  // early stop: (wave, half) has an unsatisfied check
    char* const Xb = reinterpret_cast<char*>(X);
    const int k = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // slot of this wave
    const int lane = threadIdx.x & 63, h = lane >> 5, l = lane & 31;
    const int64_t cw0 = (int64_t)blockIdx.x * 2;
    const bool live = l < ZL;
    const int zc = live ? S * l + k : k;  // idle lanes: this wave's first position
    const int base = 4 * (Z + h * N + zc);

    // APP before the first sweep = L = -llr (log2 units); a missing codeword's rows hold zeros
    for (int h2 = 0; h2 < 2; ++h2) {
        const bool have = cw0 + h2 < B;
        const float* const lp = llr + (have ? (cw0 + h2) * N : 0);
        for (int i = threadIdx.x; i < N; i += TPB) X[Z + h2 * N + i] = have ? -lp[i] * kLog2eF32 + 0.0f : 0.0f;
    }
    float msg[NE];  // c2v of every edge (log2 units), check frame
#pragma unroll
    for (int e = 0; e < NE; ++e) msg[e] = 0.0f;
    const float cmax2 = sp_cmax2(clamp);
    bool done0 = cw0 >= B, done1 = cw0 + 1 >= B;  // a missing codeword counts as stopped
    int used0 = iters, used1 = iters;
    __syncthreads();

    // byte address (less the immediate 4 * (column * Z + shift)) of this lane's edge with shift s: the wrap select
    auto addr = [&](int z, int s) __attribute__((always_inline)) { return (s != 0 && z >= Z - s) ? base - 4 * Z : base; };
    for (int it = 0; it < iters; ++it) {
        [[maybe_unused]] const bool act = live && !(h ? done1 : done0);  // a stopped codeword is frozen
        static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
            constexpr int r = decltype(rr)::value;
            constexpr int d = C::DEG[r];
            constexpr int e0 = edge_off<C>(r);
            int z = zc;
            asm volatile("" : "+v"(z));  // this row's addresses are formed here, not hoisted out of the sweep loop
            float sv[d], g[d];
            static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                constexpr int off = 4 * (C::COL[r][t] * Z + C::SH[r][t]);
                sv[t] = *reinterpret_cast<const float*>(Xb + addr(z, C::SH[r][t]) + off) - msg[e0 + t];
                g[t] = vn_signed_a(sv[t]);
            });
            cn_ds_row<d, 1, 0, QC_LSP_DS_BLOCK>(g, cmax2);
            static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                msg[e0 + t] = g[t];
                sv[t] += g[t];
            });
            if (EARLY ? act : live) {
                asm volatile("" : "+v"(z));  // the addresses again (2 VALU per edge), not 20 VGPRs held across the row
                static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                    constexpr int t = decltype(tt)::value;
                    constexpr int off = 4 * (C::COL[r][t] * Z + C::SH[r][t]);
                    *reinterpret_cast<float*>(Xb + addr(z, C::SH[r][t]) + off) = sv[t];
                });
            }
            __syncthreads();
        });
        if constexpr (EARLY) {
            // syndrome of the hard decisions the outputs would carry (z = APP * ln 2 / 2 <= ZTHR), all rows
            constexpr uint64_t LIVE = lane_range_mask<ZL, 2>(0, ZL);
            uint64_t unsat = 0;
            static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
                constexpr int r = decltype(rr)::value;
                int z = zc;
                asm volatile("" : "+v"(z));
                uint64_t par = 0;
                static_for<0, C::DEG[r]>([&](auto tt) __attribute__((always_inline)) {
                    constexpr int t = decltype(tt)::value;
                    constexpr int off = 4 * (C::COL[r][t] * Z + C::SH[r][t]);
                    const float a = *reinterpret_cast<const float*>(Xb + addr(z, C::SH[r][t]) + off);
                    par ^= __ballot(Num<float>::bit(a * kHalfLn2F32));
                });
                unsat |= par;
                asm volatile("" : "+s"(unsat));  // one row's ballots in flight at a time (SGPR budget)
            });
            unsat &= LIVE;
            if (lane == 0) {
                Fl[2 * k] = (uint32_t)((unsat & 0xffffffffull) != 0);
                Fl[2 * k + 1] = (uint32_t)((unsat >> 32) != 0);
            }
            __syncthreads();  // also: every syndrome read of APP precedes the next sweep's stores
            uint32_t u0 = 0, u1 = 0;
#pragma unroll
            for (int q = 0; q < S; ++q) {
                u0 |= Fl[2 * q];
                u1 |= Fl[2 * q + 1];
            }
            if (!done0 && u0 == 0) { done0 = true; used0 = it + 1; }
            if (!done1 && u1 == 0) { done1 = true; used1 = it + 1; }
            if (done0 && done1) break;  // the pooled flags: the same decision in every wave
        }
    }
    // outputs from LDS in element order; the thread id is rebuilt (v_mbcnt, the scalar wave slot), not kept
    // across the loop
    const int te = k * 64 + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    for (int h2 = 0; h2 < 2; ++h2) {
        const int64_t cwo = cw0 + h2;
        if (cwo >= B) break;
        for (int i = te; i < N; i += TPB) {
            const float zz = X[Z + h2 * N + i] * kHalfLn2F32;
            if (bits) bits[cwo * N + i] = (uint8_t)Num<float>::bit(zz);
            if (soft) soft[cwo * N + i] = (flags & LDPC_F_SOFT_Z) ? zz : 1.0f - 1.0f / (1.0f + Num<float>::exp_(-zz));
        }
        if (te == 0 && iters_used) iters_used[cwo] = h2 ? used1 : used0;
    }
}

int qc_launch_sp_lay_wifi1944_56(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft,
                                 int32_t* used, hipStream_t st) {
    using C = Wifi1944_56;
    const unsigned blocks = (unsigned)((B + 1) / 2);  // one unit of S waves per codeword pair
    const dim3 tb(C::S * 64);
    if (p.flags & LDPC_F_EARLY_STOP)
        k_qc_sp_lay<C, true><<<blocks, tb, 0, st>>>((const float*)llr, B, p.iters, p.clamp, p.flags, bits, (float*)soft, used);
    else
        k_qc_sp_lay<C, false><<<blocks, tb, 0, st>>>((const float*)llr, B, p.iters, p.clamp, p.flags, bits, (float*)soft, used);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "layered tanh-SP kernel launch: %s", hipGetErrorString(e));
    return LDPC_OK;
}

}  // namespace ldpc
