// qc_ms.h — float min-sum register kernels for the 802.11n QC codes with Z <= 64 (see qc.hip for the lane layout):
// k_qc_ms_st (stored messages, variable frame) and k_qc_ms_ph (phased, Z <= 32: the headline kernel).  Templates
// only: qc.hip instantiates the fixed-count kernels, qc_es.hip the early-stop ones.
#pragma once
#include "qc_common.h"

#include <cstdint>

namespace ldpc {

// Stored-message variant (fixed iteration count): every edge's c2v message is kept in a VGPR in the
// VARIABLE frame, so the check update needs no reconstruction from a compressed state and the variable
// update no re-compression.  Per iteration: v2c = APP - c2v in place for all edges (APP is then dead),
// then per row: gather v2c into the check frame, two-minimum + sign product, scatter the new c2v back
// (in place) and add it into APP_{it+1} in ascending row order.  Same arithmetic as the
// oracle, operation for operation.  The register kernel is instruction-fetch bound (SQC_ICACHE_BUSY ~
// 100%): this form executes ~12 instead of ~17 instructions (~76 instead of ~124 bytes) per edge, at
// <= 128 VGPRs (4 waves per SIMD).
#ifndef QC_ST_TPB
#define QC_ST_TPB 256  // threads per workgroup of the stored min-sum kernel (whole waves)
#endif
// Early stop: a workgroup's LDS stays allocated until its slowest wave exits, so with waves that leave at
// different iterations one-wave workgroups free CU slots sooner (A/B, profiles/r02/ab/ab_tpb.txt: (648,1/2)
// min-sum early stop 61.9 -> 65.5 M cw/s; fixed-count kernels: 256 / 128 / 64 within noise, 256 kept).
#ifndef QC_ST_TPB_EARLY
#define QC_ST_TPB_EARLY 64
#endif
template <bool EARLY>
constexpr int st_tpb() { return EARLY ? QC_ST_TPB_EARLY : QC_ST_TPB; }
#ifndef QC_ST_WAVES_PER_SIMD
#define QC_ST_WAVES_PER_SIMD 3  // dispatched for Z > 32 ((1296,2/3)): spill-free at 134 VGPRs, 41.0 vs 39.9 M cw/s at 4
                                // waves (2-5 VGPRs spilled; A/B, 20 it)
#endif
#ifndef QC_ST_WAVES_PER_SIMD_EARLY
#define QC_ST_WAVES_PER_SIMD_EARLY 4  // early stop keeps APP_it and the syndrome ballots live: 14-15 VGPRs spill at
                                      // 4 waves, yet 3 waves (spill-free) measured 9 % slower on (1296,2/3)
#endif

template <class C, bool QUANT, bool EARLY, int NORM>
__global__ __launch_bounds__(256, EARLY ? QC_ST_WAVES_PER_SIMD_EARLY : QC_ST_WAVES_PER_SIMD) void k_qc_ms_st(const float* __restrict__ llr, int64_t B, int iters,
                                                                       float clamp, float alpha, float beta, float qmax,
                                                                       float app_max, float qinv, int flags,
                                                                       uint8_t* __restrict__ bits, float* __restrict__ soft,
                                                                       int32_t* __restrict__ iters_used) {
    constexpr int Z = C::Z, NB = C::NB, MB = C::MB, N = NB * Z;
    constexpr int NE = edge_off<C>(MB);
    static_assert(Z <= 64, "register kernel needs Z <= 64");
    constexpr int CPW = (Z <= 32) ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const int half = (CPW == 2) ? (lane >> 5) : 0;
    const int z = (CPW == 2) ? (lane & 31) : lane;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t cw = wave * CPW + half;
    const bool valid = (z < Z) && (cw < B);
    const int zb = lane_zb<Z, CPW>(z);
    const int base4 = (half * 32 + zb) * 4;
    const int base4m = base4 - 4 * Z;
    const int64_t cwbase = valid ? cw * N : 0;
    const float vmask = valid ? 1.0f : 0.0f;
    auto vidx = [&](int zz, int j, int phi) {
        int t = zz + phi;
        t -= (t >= Z) ? Z : 0;
        return cwbase + j * Z + (valid ? t : 0);
    };
    using f4 = __attribute__((ext_vector_type(4))) float;
    constexpr int LSTR = lstr<C>(), NG = (NB + 3) / 4;
    __shared__ __attribute__((aligned(16))) float Ls[st_tpb<EARLY>() * LSTR];  // lane-major L rows (qc_common.h lpos)
    const int lrow = threadIdx.x * LSTR;
#define LS_AT(row, j) Ls[(row) + lpos<C>(j)]
    float app[NB];
    static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
        constexpr int j = decltype(jj)::value;
        float x = llr[vidx(z, j, C::PHI[j])] * vmask;
        if (QUANT) x = fminf(fmaxf(rintf(x * qinv), -qmax), qmax);
        app[j] = -x;  // L
        LS_AT(lrow, j) = app[j];
        app[j] = app[j] + 0.0f;  // APP_0 = L + sum(c2v = +0): -0 -> +0, as the oracle
    });
    if (QUANT) {
#pragma unroll
        for (int j = 0; j < NB; ++j) app[j] = fminf(fmaxf(app[j], -app_max), app_max);
    }
    float msg[NE];  // c2v of every edge (variable frame); v2c in place during an iteration
#pragma unroll
    for (int e = 0; e < NE; ++e) msg[e] = 0.0f;
    // early stop: lanes of each codeword group, converged groups, their iteration counts
    constexpr uint64_t ACTIVE = lane_range_mask<Z, CPW>(0, Z);
    uint64_t done_groups = 0;  // (group lane mask) of converged codewords, CPW == 2
    int used_lo = iters, used_hi = iters;

    for (int it = 0; it < iters; ++it) {
        if constexpr (EARLY) {
            if (it > 0) {
                // syndrome of APP_it: per block column one ballot of the hard decisions (bit = APP <= 2*ZTHR;
                // quantized: APP < 0, the same for integers), then per check row the XOR of its columns'
                // masks rotated into the check frame by the edge's lane shift
                const float thr2 = 2.0f * kZthrF32;
                if constexpr (CPW == 1) {
                    // row by row with an early exit (as in k_qc_ms_ph): the codeword is still
                    // unsatisfied once one row's parity is nonzero, usually at the first row
                    bool sat = true;
                    static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
                        constexpr int r = decltype(rr)::value;
                        if (sat) {
                            uint64_t par = 0;
                            static_for<0, C::DEG[r]>([&](auto tt) __attribute__((always_inline)) {
                                constexpr int t = decltype(tt)::value;
                                const uint64_t b = __ballot(app[C::COL[r][t]] <= thr2) & ACTIVE;
                                par ^= rot_lanes<Z, CPW, C::SHR[r][t]>(b);
                            });
                            if (par & ACTIVE) sat = false;
                        }
                    });
                    if (sat) {  // the wave's codeword satisfies every check: APP_it is the output
                        used_lo = it;
                        break;
                    }
                } else {
                uint64_t par[MB];
#pragma unroll
                for (int r = 0; r < MB; ++r) par[r] = 0;
                static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
                    constexpr int j = decltype(jj)::value;
                    const uint64_t b = __ballot(app[j] <= thr2) & ACTIVE;
                    static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
                        constexpr int r = decltype(rr)::value;
                        constexpr int t = first_slot<C>(r, j);
                        if constexpr (t >= 0) par[r] ^= rot_lanes<Z, CPW, C::SHR[r][t]>(b);
                    });
                });
                uint64_t unsat = 0;
#pragma unroll
                for (int r = 0; r < MB; ++r) unsat |= par[r];
                unsat &= ACTIVE;
                constexpr uint64_t G0 = lane_range_mask<Z, 1>(0, Z), G1 = G0 << 32;
                const uint64_t newly = ((unsat & G0) ? 0 : G0) | ((unsat & G1) ? 0 : G1);
                const uint64_t fresh = newly & ~done_groups;
                if (fresh) {
                    // park the converged codeword's APP_it in its own L region of LDS (L is no longer
                    // needed by it); its lanes keep computing for the other codeword, discarded
                    if (fresh & G0) used_lo = it;
                    if (fresh & G1) used_hi = it;
                    if ((fresh >> lane) & 1ull) {
                        static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
                            constexpr int j = decltype(jj)::value;
                            LS_AT(lrow, j) = app[j];
                        });
                    }
                    done_groups |= fresh;
                    if (done_groups == (G0 | G1)) break;
                }
                }  // two codewords per wave: all rows
            }
        }
        static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
            constexpr int r = decltype(rr)::value;
            static_for<0, C::DEG[r]>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                constexpr int e = edge_off<C>(r) + t;
                float x = app[C::COL[r][t]] - msg[e];
                if constexpr (QUANT) x = fminf(fmaxf(x, -qmax), qmax);
                msg[e] = x;
            });
        });
        float nap[NB];
        f4 Lg[NG];
        static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
            constexpr int r = decltype(rr)::value;
            constexpr int d = C::DEG[r];
            constexpr int e0 = edge_off<C>(r);
            static_for<0, NG>([&](auto gg) __attribute__((always_inline)) {
                constexpr int g = decltype(gg)::value;
                if constexpr (lgroup_row<C>(g) == r) {
                    int lr = lrow;
                    asm volatile("" : "+v"(lr));  // not hoisted out of the iteration (register budget)
                    Lg[g] = *static_cast<const f4*>(__builtin_assume_aligned(&Ls[lr + 4 * g], 16));
                }
            });
            float v[d];
            float mn1, mn2;
            static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                constexpr int s = C::SHR[r][t];
                float x;
                if constexpr (s == 0) {
                    x = msg[e0 + t];
                } else {
                    const int addr = sel_lanes<wrap_mask<Z, CPW>(Z - s)>(base4, base4m) + 4 * s;
                    x = bperm(addr, msg[e0 + t]);
                }
                v[t] = x;
            });
            two_min(v, mn1, mn2);
            const uint32_t tot = xor_all(v) & 0x80000000u;
            // sign of the product folded into the two magnitudes once per row
            const float M1 = __uint_as_float(__float_as_uint(mag_of<NORM>(mn1, alpha, beta, clamp)) ^ tot);
            const float M2 = __uint_as_float(__float_as_uint(mag_of<NORM>(mn2, alpha, beta, clamp)) ^ tot);
            // NORM_PLAIN: compare-free select (med3 of the unsigned magnitudes, XOR): +3.4 % on (1296,2/3), A/B;
            // -1.3 % in the LDS-bound k_qc_ms_ph, which keeps v_cmp/v_cndmask
            const float A1 = mag_of<NORM>(mn1, alpha, beta, clamp), A2 = mag_of<NORM>(mn2, alpha, beta, clamp);
            const uint32_t X = __float_as_uint(M1) ^ __float_as_uint(A2);
            static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                constexpr int j = C::COL[r][t], s = C::SHR[r][t];
                // |v| == min1 picks the min slot; ties imply min2 == min1 and M2 == M1, so the choice cannot
                // change any value (bit-exact against the oracle)
                float c;
                if constexpr (NORM == NORM_PLAIN) {
                    const uint32_t m = __float_as_uint(__builtin_amdgcn_fmed3f(fabsf(v[t]), A1, A2));
                    c = __uint_as_float((X ^ m) ^ (__float_as_uint(v[t]) & 0x80000000u));
                } else {
                    const float mg = (fabsf(v[t]) == mn1) ? M2 : M1;
                    c = __uint_as_float(__float_as_uint(mg) ^ (__float_as_uint(v[t]) & 0x80000000u));
                }
                float cr;
                if constexpr (s == 0) {
                    cr = c;
                } else {
                    const int addr = sel_lanes<wrap_mask<Z, CPW>(s)>(base4, base4m) + 4 * (Z - s);
                    cr = bperm(addr, c);
                }
                msg[e0 + t] = cr;
                if constexpr (first_row<C>(j) == r) nap[j] = Lg[lpos<C>(j) / 4][lpos<C>(j) % 4];
                nap[j] = nap[j] + cr;
            });
        });
#pragma unroll
        for (int j = 0; j < NB; ++j) app[j] = QUANT ? fminf(fmaxf(nap[j], -app_max), app_max) : nap[j];
    }
    // epilogue indices recomputed from the thread id (opaque), so nothing but the loop state is live
    // across the loop (the 4-waves/SIMD register budget is 128)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int zo = (CPW == 2) ? (tid & 31) : (tid & 63);
    const int64_t cwo = (((int64_t)blockIdx.x * blockDim.x + tid) >> 6) * CPW + ((CPW == 2) ? ((tid >> 5) & 1) : 0);
    const bool parked = EARLY && CPW == 2 && ((done_groups >> (tid & 63)) & 1ull);
    if (zo < Z && cwo < B) {
        const int lbo = tid * LSTR;
        static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
            constexpr int j = decltype(jj)::value;
            int t = zo + C::PHI[j];
            t -= (t >= Z) ? Z : 0;
            const int64_t o = cwo * N + j * Z + t;
            const float zz = 0.5f * (parked ? LS_AT(lbo, j) : app[j]);
            if (bits) bits[o] = (uint8_t)(zz <= kZthrF32);
            if (soft) soft[o] = (flags & LDPC_F_SOFT_Z) ? zz : 1.0f - 1.0f / (1.0f + expf(-zz));
        });
        if (zo == 0 && iters_used) iters_used[cwo] = (CPW == 2 && ((tid >> 5) & 1)) ? used_hi : used_lo;
    }
}
#undef LS_AT

// ---- Phased stored-message min-sum (k_qc_ms_ph) ---------------------------------------------------
// The same flooding arithmetic as k_qc_ms_st (and the oracle), operation for operation, regrouped into
// two phases per iteration so that no lane rotation sits on a dependency chain:
//   CN phase, row by row:   msg[e] (v2c, variable frame) -> gathered into the check frame IN PLACE,
//                           two-minimum / sign product, msg[e] = new c2v in the CHECK frame.
//                           Rows are independent: row r+1's gathers overlap row r's arithmetic.
//   VN phase, column by column: msg[e] -> rotated back to the variable frame in place,
//                           APP_j = L_j + sum of c2v in ascending row order (the oracle's order),
//                           msg[e] = APP_j - c2v (v2c of the next iteration).  Columns are independent.
// Nothing but msg[] is live across a phase (APP is per column and transient), so the rotation
// addresses — one per distinct lane shift rho, "read lane (z + rho) mod Z of my group" — are computed
// once before the loop and held in registers (QC_PH_ADDR_MIN_USES) instead of one v_cndmask per ds_bpermute.
// Iteration 0's v2c is L itself (c2v = +0: L - 0 == L bitwise, also for L = -0), so the loop starts at
// the CN phase; the last iteration's VN phase writes the outputs directly instead of forming v2c.
#ifndef QC_PH_ADDR_MIN_USES
#define QC_PH_ADDR_MIN_USES 3  // rotations used >= 3 times per iteration get an address register (A/B: 1 -> spills, 38.5 vs 37.9 M cw/s at 1; 4: 38.3; 6: 37.7; none: 37.0)
#endif
#ifndef QC_PH_WAVES_PER_SIMD
#define QC_PH_WAVES_PER_SIMD 4
#endif
#ifndef QC_PH_ADDR_MIN_USES_EARLY
#define QC_PH_ADDR_MIN_USES_EARLY QC_PH_ADDR_MIN_USES
#endif
// Phase priorities (s_setprio): a SIMD issues from the higher-priority waves first, so raising the phase
// whose waves stall on their own dependences lets their instructions issue the moment they are ready while the
// other phase's independent work fills the gaps.  The fixed-count kernel runs its CN phase (the rotations'
// gathers and the two-minimum chains) at priority 1 and its VN phase at 0: 42.0 -> 43.4-44.0 M cw/s (A/B
// profiles/r04/ab/ab_prio.txt).
// LDS-row rotations (fixed count): lane rotations through a 256-B LDS row per wave instead of ds_bpermute — every
// lane stores its value with ds_write_addtid_b32 (address M0 + 4 * lane: no address VGPR to move), then loads the
// slot of lane (z + rho) with ds_read_b32 at the address the ds_bpermute would have taken.  A wave's LDS
// operations run in order, so one row serves every rotation with no wait or barrier.  Measured on the box
// (scripts/lds_micro.hip, profiles/r02/micro/): 4.31 LDS-pipe cycles per rotation against 6.16 for ds_bpermute
// (which moves an address and a data VGPR in and a data VGPR out) — the resource that binds this kernel.
// Early stop keeps ds_bpermute (A/B: 61.8 vs 61.5 M cw/s; not LDS-bound).
#ifndef QC_PH_WAVES_PER_SIMD_EARLY
#define QC_PH_WAVES_PER_SIMD_EARLY 3  // spill-free (145 VGPRs): 648 min-sum early stop 24.6 -> 57.9 M cw/s (A/B)
#endif

template <class C, bool QUANT, bool EARLY, int NORM>
__global__ __launch_bounds__(256, EARLY ? QC_PH_WAVES_PER_SIMD_EARLY : QC_PH_WAVES_PER_SIMD) void k_qc_ms_ph(const float* __restrict__ llr, int64_t B, int iters,
                                                                       float clamp, float alpha, float beta, float qmax,
                                                                       float app_max, float qinv, int flags,
                                                                       uint8_t* __restrict__ bits, float* __restrict__ soft,
                                                                       int32_t* __restrict__ iters_used) {
    constexpr int Z = C::Z, NB = C::NB, MB = C::MB, N = NB * Z;
    constexpr int NE = edge_off<C>(MB);
    static_assert(Z <= 32, "phased kernel: two codewords per wave (Z <= 32)");
    constexpr int CPW = 2;
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5;
    const int z = lane & 31;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t cw = wave * CPW + half;
    const bool valid = (z < Z) && (cw < B);
    const int zb = lane_zb<Z, CPW>(z);
    const int base4 = (half * 32 + zb) * 4;
    const int base4m = base4 - 4 * Z;
    using f4 = __attribute__((ext_vector_type(4))) float;
    constexpr int LSTR = lstr<C>();
    __shared__ __attribute__((aligned(16))) float Ls[st_tpb<EARLY>() * LSTR];  // lane-major L rows (qc_common.h lpos)
    const int lrow = threadIdx.x * LSTR;
    const int lrow4 = lrow * 4;  // bytes (lds_reload)

    constexpr bool LDSROT = !EARLY;
    __shared__ float Rw[LDSROT ? st_tpb<EARLY>() : 1];  // one 64-lane rotation row per wave
    const int wrow = LDSROT ? (int)(threadIdx.x & ~63u) * 4 : 0;  // this wave's row, bytes from Rw
    const int rb4 = base4 + wrow, rb4m = base4m + wrow;        // read addresses include the row
    if constexpr (LDSROT) {
        // M0 = this wave's row, set once: nothing else in this kernel reads or writes M0 (the CPU test
        // test_kernel_resources.py::test_headline_m0_written_once checks the built code); s_nop 0: an SALU write
        // of M0 needs one wait state before an add-TID LDS instruction reads it
        const unsigned m0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(&Rw[0]) + (unsigned)wrow);
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" ::"s"(m0) : "memory");
    }
    auto xfer = [&](int addr, float x) __attribute__((always_inline)) {
        if constexpr (LDSROT) {
            asm volatile("ds_write_addtid_b32 %0" ::"v"(x) : "memory");
            return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(Rw) + addr);
        } else {
            return bperm(addr, x);
        }
    };
    // rotation addresses, one register per distinct shift used often enough (the others: one v_cndmask
    // per use, as k_qc_ms_st)
    constexpr int AMU = EARLY ? QC_PH_ADDR_MIN_USES_EARLY : QC_PH_ADDR_MIN_USES;
    int ra[Z];
    static_for<1, Z>([&](auto rr) __attribute__((always_inline)) {
        constexpr int rho = decltype(rr)::value;
        if constexpr (rot_uses<C>(rho) >= AMU)
            ra[rho] = sel_lanes<wrap_mask<Z, CPW>(Z - rho)>(rb4, rb4m) + 4 * rho;
    });
    auto rot = [&](auto rr, float x) __attribute__((always_inline)) {  // value of lane (z + rho) mod Z
        constexpr int rho = decltype(rr)::value;
        if constexpr (rho == 0) {
            return x;
        } else if constexpr (rot_uses<C>(rho) >= AMU) {
            return xfer(ra[rho], x);
        } else {
            return xfer(sel_lanes<wrap_mask<Z, CPW>(Z - rho)>(rb4, rb4m) + 4 * rho, x);
        }
    };
    (void)ra;

    // L = -llr (quantized in QUANT mode) into this lane's LDS row; msg = v2c of iteration 0 = APP_0 = L
    float msg[NE];
    {
        const int64_t cwbase = valid ? cw * N : 0;
        const float vmask = valid ? 1.0f : 0.0f;
        float L[NB];
        static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
            constexpr int j = decltype(jj)::value;
            int t = z + C::PHI[j];
            t -= (t >= Z) ? Z : 0;
            float x = llr[cwbase + j * Z + (valid ? t : 0)] * vmask;
            if (QUANT) x = fminf(fmaxf(rintf(x * qinv), -qmax), qmax);
            L[j] = -x;
            Ls[lrow + lpos<C>(j)] = L[j];
            if (QUANT) L[j] = fminf(fmaxf(L[j], -app_max), app_max);  // APP_0 (k_qc_ms_st: app clamp)
        });
        static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
            constexpr int r = decltype(rr)::value;
            static_for<0, C::DEG[r]>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                float x = L[C::COL[r][t]] + 0.0f;  // v2c = APP_0 - c2v(= +0), APP_0 = L + (+0): -0 -> +0
                if constexpr (QUANT) x = fminf(fmaxf(x, -qmax), qmax);
                msg[edge_off<C>(r) + t] = x;
            });
        });
    }
    constexpr uint64_t ACTIVE = lane_range_mask<Z, CPW>(0, Z);
    constexpr uint64_t G0 = lane_range_mask<Z, 1>(0, Z), G1 = G0 << 32;
    uint64_t done_groups = 0;
    int used_lo = iters, used_hi = iters;
    const float thr2 = 2.0f * kZthrF32;

    // CN phase: v2c (variable frame) -> c2v (check frame), in place
    auto cn_phase = [&]() __attribute__((always_inline)) {
        static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
            constexpr int r = decltype(rr)::value;
            constexpr int d = C::DEG[r];
            constexpr int e0 = edge_off<C>(r);
            float v[d];
            static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                v[t] = rot(std::integral_constant<int, C::SHR[r][t]>{}, msg[e0 + t]);
            });
            float mn1, mn2;
            two_min(v, mn1, mn2);
            const uint32_t tot = xor_all(v) & 0x80000000u;
            const float M1 = __uint_as_float(__float_as_uint(mag_of<NORM>(mn1, alpha, beta, clamp)) ^ tot);
            const float M2 = __uint_as_float(__float_as_uint(mag_of<NORM>(mn2, alpha, beta, clamp)) ^ tot);
            static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                const float mg = (fabsf(v[t]) == mn1) ? M2 : M1;
                msg[e0 + t] = __uint_as_float(__float_as_uint(mg) ^ (__float_as_uint(v[t]) & 0x80000000u));
            });
        });
    };
    // Lookahead form (fixed count): rotations happen in place on msg[] (no extra registers), issued one row /
    // column ahead of the arithmetic that consumes them, so each wave keeps several rotations in flight
    auto gather_row = [&](auto rr) __attribute__((always_inline)) {
        constexpr int r = decltype(rr)::value;
        static_for<0, C::DEG[r]>([&](auto tt) __attribute__((always_inline)) {
            constexpr int t = decltype(tt)::value;
            msg[edge_off<C>(r) + t] = rot(std::integral_constant<int, C::SHR[r][t]>{}, msg[edge_off<C>(r) + t]);
        });
    };
    auto math_row = [&](auto rr) __attribute__((always_inline)) {
        constexpr int r = decltype(rr)::value;
        constexpr int d = C::DEG[r];
        constexpr int e0 = edge_off<C>(r);
        float v[d];
        static_for<0, d>([&](auto tt) __attribute__((always_inline)) { v[decltype(tt)::value] = msg[e0 + decltype(tt)::value]; });
        float mn1, mn2;
        two_min(v, mn1, mn2);
        const uint32_t tot = xor_all(v) & 0x80000000u;
        const float M1 = __uint_as_float(__float_as_uint(mag_of<NORM>(mn1, alpha, beta, clamp)) ^ tot);
        const float M2 = __uint_as_float(__float_as_uint(mag_of<NORM>(mn2, alpha, beta, clamp)) ^ tot);
        static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
            constexpr int t = decltype(tt)::value;
            const float mg = (fabsf(v[t]) == mn1) ? M2 : M1;
            msg[e0 + t] = __uint_as_float(__float_as_uint(mg) ^ (__float_as_uint(v[t]) & 0x80000000u));
        });
    };
    auto cn_phase_la = [&]() __attribute__((always_inline)) {
        gather_row(std::integral_constant<int, 0>{});
        static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
            constexpr int r = decltype(rr)::value;
            if constexpr (r + 1 < MB) gather_row(std::integral_constant<int, r + 1>{});
            math_row(rr);
        });
    };
    // VN phase, column j: c2v back to the variable frame, APP_j = L_j + ascending sum; returns APP_j
    f4 Lg;
    auto vn_col = [&](auto pp) __attribute__((always_inline)) {
        constexpr int p = decltype(pp)::value;  // LDS position (columns in first-use order)
        constexpr int j = lcol<C>(p);
        constexpr int dj = col_deg<C>(j);
        if constexpr (p % 4 == 0) {
            Lg = lds_reload<4 * p, f4, 16>(Ls, lrow4);  // not hoisted out of the loop (register budget)
        }
        float a = Lg[p % 4];
        static_for<0, dj>([&](auto kk) __attribute__((always_inline)) {
            constexpr int e = col_edge<C>(j, decltype(kk)::value);
            constexpr int r = edge_row<C>(e), t = e - edge_off<C>(r);
            constexpr int s = C::SHR[r][t];
            msg[e] = rot(std::integral_constant<int, (s == 0) ? 0 : Z - s>{}, msg[e]);
            a = a + msg[e];
        });
        if (QUANT) a = fminf(fmaxf(a, -app_max), app_max);
        return a;
    };
    auto rot_col = [&](auto pp) __attribute__((always_inline)) {  // c2v of column lcol(p) back, in place
        constexpr int j = lcol<C>(decltype(pp)::value);
        static_for<0, col_deg<C>(j)>([&](auto kk) __attribute__((always_inline)) {
            constexpr int e = col_edge<C>(j, decltype(kk)::value);
            constexpr int r = edge_row<C>(e), t = e - edge_off<C>(r);
            constexpr int s = C::SHR[r][t];
            msg[e] = rot(std::integral_constant<int, (s == 0) ? 0 : Z - s>{}, msg[e]);
        });
    };
    auto sum_col = [&](auto pp) __attribute__((always_inline)) {  // APP_j from already rotated c2v
        constexpr int p = decltype(pp)::value;
        constexpr int j = lcol<C>(p);
        if constexpr (p % 4 == 0) {
            Lg = lds_reload<4 * p, f4, 16>(Ls, lrow4);
        }
        float a = Lg[p % 4];
        static_for<0, col_deg<C>(j)>([&](auto kk) __attribute__((always_inline)) { a = a + msg[col_edge<C>(j, decltype(kk)::value)]; });
        if (QUANT) a = fminf(fmaxf(a, -app_max), app_max);
        return a;
    };
    auto v2c_col = [&](auto jj, float a) __attribute__((always_inline)) {
        constexpr int j = decltype(jj)::value;
        static_for<0, col_deg<C>(j)>([&](auto kk) __attribute__((always_inline)) {
            constexpr int e = col_edge<C>(j, decltype(kk)::value);
            float x = a - msg[e];
            if constexpr (QUANT) x = fminf(fmaxf(x, -qmax), qmax);
            msg[e] = x;
        });
    };

    int it = 0;
    // Fixed count: the idle lanes (z >= Z: 10 of 64 at Z = 27) sit the iteration loop out, EXEC-masked — no active
    // lane ever reads them (rotation sources are active slots) — so they stop drawing power: +0.9 % (A/B
    // profiles/r04/ab/ab_mask.txt)
    const bool loop_lane = EARLY || z < Z;
    if (loop_lane) {
    for (; it + 1 < iters; ++it) {
        if constexpr (!EARLY) {
            __builtin_amdgcn_s_setprio(1);
            cn_phase_la();
            __builtin_amdgcn_s_setprio(0);
            rot_col(std::integral_constant<int, 0>{});
            static_for<0, NB>([&](auto pp) __attribute__((always_inline)) {
                constexpr int p = decltype(pp)::value;
                if constexpr (p + 1 < NB) rot_col(std::integral_constant<int, p + 1>{});
                v2c_col(std::integral_constant<int, lcol<C>(p)>{}, sum_col(pp));
            });
        } else {
            cn_phase();
            // APP_{it+1} of every column (kept until the syndrome verdict), hard-decision ballots
            float app[NB];
            // Row by row with an early exit (as the packed kernel's): `cand` starts as the lane
            // groups (codewords) not yet done and loses each one whose row parity is nonzero; the scan stops once
            // neither codeword of the wave can still be satisfied — at low Eb/N0 after the first row.  The
            // ballots are taken at each use.  The decision equals the all-rows form's.
            static_for<0, NB>([&](auto pp) __attribute__((always_inline)) {
                constexpr int p = decltype(pp)::value;
                app[lcol<C>(p)] = vn_col(pp);
            });
            uint64_t cand = (G0 | G1) & ~done_groups;
            static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
                constexpr int r = decltype(rr)::value;
                if (cand) {
                    uint64_t par = 0;
                    static_for<0, C::DEG[r]>([&](auto tt) __attribute__((always_inline)) {
                        constexpr int t = decltype(tt)::value;
                        const uint64_t b = __ballot(app[C::COL[r][t]] <= thr2) & ACTIVE;
                        par ^= rot_lanes<Z, CPW, C::SHR[r][t]>(b);
                    });
                    par &= ACTIVE;
                    if (par & G0) cand &= ~G0;
                    if (par & G1) cand &= ~G1;
                }
            });
            const uint64_t fresh = cand;
            if (fresh) {
                // park the converged codeword's APP in its L row (L is no longer needed by it)
                if (fresh & G0) used_lo = it + 1;
                if (fresh & G1) used_hi = it + 1;
                if ((fresh >> lane) & 1ull) {
                    static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
                        constexpr int j = decltype(jj)::value;
                        Ls[lrow + lpos<C>(j)] = app[j];
                    });
                }
                done_groups |= fresh;
                if (done_groups == (G0 | G1)) break;
            }
            static_for<0, NB>([&](auto jj) __attribute__((always_inline)) { v2c_col(jj, app[decltype(jj)::value]); });
        }
    }
    }  // loop_lane
    // last iteration (or early exit): outputs straight from the VN phase, column by column
    const bool early_exit = EARLY && done_groups == (G0 | G1);
    if (!early_exit && iters > 0) {
        cn_phase();
    }
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int zo = tid & 31;
    const int64_t cwo = (((int64_t)blockIdx.x * blockDim.x + tid) >> 6) * CPW + ((tid >> 5) & 1);
    const bool parked = EARLY && ((done_groups >> (tid & 63)) & 1ull);
    const bool ok = zo < Z && cwo < B;
    static_for<0, NB>([&](auto pp) __attribute__((always_inline)) {
        constexpr int p = decltype(pp)::value;
        constexpr int j = lcol<C>(p);
        float a;
        if (iters > 0 && !early_exit) a = vn_col(pp);
        else a = Ls[lrow + p] + (iters == 0 ? 0.0f : -0.0f);  // iters == 0: APP_0 = L + (+0) (QUANT: clamped
                                                               // below); early exit: parked APP (x + -0 == x)
        if (QUANT && iters == 0) a = fminf(fmaxf(a, -app_max), app_max);
        if (parked) a = Ls[lrow + p];
        if (ok) {
            int t = zo + C::PHI[j];
            t -= (t >= Z) ? Z : 0;
            const int64_t o = cwo * N + j * Z + t;
            const float zz = 0.5f * a;
            if (bits) bits[o] = (uint8_t)(zz <= kZthrF32);
            if (soft) soft[o] = (flags & LDPC_F_SOFT_Z) ? zz : 1.0f - 1.0f / (1.0f + expf(-zz));
        }
    });
    if (ok && zo == 0 && iters_used) iters_used[cwo] = ((tid >> 5) & 1) ? used_hi : used_lo;
}

}  // namespace ldpc
