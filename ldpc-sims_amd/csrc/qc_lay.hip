// qc_lay.hip — layered (row-serial) min-sum for the 802.11n quasi-cyclic codes with Z <= 64 (gfx950).
//
// The schedule (include/ldpc_abi.h LDPC_F_LAYERED): the checks are processed in ascending
// order within a sweep, and each one reads the posteriors its predecessors of the same sweep have already
// updated:  t_e = APP_v - c2v[e];  c2v[e] = min-sum of the check's other t;  APP_v = t_e + c2v[e].
// Every 802.11n block is one circulant, so the Z checks of a base row touch disjoint variables and run in
// parallel on the lanes of a wave with the serial result, bit for bit.
//
// Dataflow (lane <-> lifting index z, two codewords per wave at Z <= 32, as the flooding register kernels):
//   * APP[NB] in VGPRs in a FLOATING FRAME: column j sits in the check frame of the last base row that
//     touched it (lane z holds variable (j, (z + s) mod Z), s that row's shift on j).  The next row, with
//     shift s', first rotates it by rho = (s' - s) mod Z ("value of lane (z + rho) mod Z").  The rows of a
//     column follow each other cyclically (the last hands over to the first of the next sweep), so every rho
//     is a compile-time constant (LayFrames, from C::COL / C::SH); rho == 0 costs nothing.  At most one
//     rotation per edge per sweep, where the flooding kernels rotate twice (gather, scatter).
//   * no rotation at either end: L_j is loaded from global memory in the frame of the column's LAST row and
//     the outputs are stored from that same frame, which every sweep ends in — whatever `iters` is.
//   * the check state never rotates.  Fixed count: one c2v register per edge (STORED, measured faster).
//     Early stop: compressed per base row, the two post-normalisation magnitudes M1 = mag(min1),
//     M2 = mag(min2) and one word with the argmin slot and the sign of every c2v (3 VGPRs per base row); the
//     previous c2v[e] is (slot == argmin ? M2 : M1) with its sign bit, the bits of a stored message.
//   * LDS carries nothing but the rotation transport: one 64-lane row per wave written with
//     ds_write_addtid_b32 (fixed count, Z <= 32), ds_bpermute otherwise — the choice the flooding kernels
//     measured per code.
#include "qc_lay_frames.h"

#include <cstdint>

namespace ldpc {

#ifndef QC_LAY_WAVES_PER_SIMD
#define QC_LAY_WAVES_PER_SIMD 4  // 128 VGPRs: 24 APP + 88 c2v + a row's transients
#endif
#ifndef QC_LAY_WAVES_PER_SIMD_EARLY
#define QC_LAY_WAVES_PER_SIMD_EARLY 4  // spill-free at 86-99 VGPRs; bounded to 96 by 5 waves the (648,1/2) kernels
                                       // spill 4 VGPRs (the all-rows syndrome's 64-bit masks overflow the SGPRs)
#endif
#ifndef QC_LAY_TPB_EARLY
#define QC_LAY_TPB_EARLY 64  // early stop: one-wave workgroups leave the CU as they finish (as QC_ST_TPB_EARLY)
#endif
template <bool EARLY>
constexpr int lay_tpb() { return EARLY ? QC_LAY_TPB_EARLY : 256; }

template <class C, bool EARLY, int NORM>
__global__ __launch_bounds__(256, EARLY ? QC_LAY_WAVES_PER_SIMD_EARLY : QC_LAY_WAVES_PER_SIMD) void k_qc_ms_lay(
    const float* __restrict__ llr, int64_t B, int iters, float clamp, float alpha, float beta, int flags,
    uint8_t* __restrict__ bits, float* __restrict__ soft, int32_t* __restrict__ iters_used) {
    constexpr int Z = C::Z, NB = C::NB, MB = C::MB, N = NB * Z;
    static_assert(Z <= 64, "register kernel needs Z <= 64");
    static_assert(C::MAXDC <= 27, "slot signs and the argmin share one word");
    constexpr int CPW = (Z <= 32) ? 2 : 1;
    // Fixed count: one c2v register per edge (check frame, never rotated) instead of the compressed row state — no
    // reconstruction of the old message and no sign / argmin packing, ~10 instead of ~15 VALU instructions per edge
    // in a kernel bound by VALU issue: A/B on (648,1/2), 25 sweeps, B = 65,536: 1.544 -> 0.848 ms per launch
    // (profiles/layered/), at 119-121 VGPRs (4 waves) instead of 59-69 (7 waves).  Early stop keeps the compressed
    // state: with 88 more registers its all-rows syndrome spills.
    constexpr bool STORED = !EARLY;
    using F = LayFrames<C>;
    const int lane = threadIdx.x & 63;
    const int half = (CPW == 2) ? (lane >> 5) : 0;
    const int z = (CPW == 2) ? (lane & 31) : lane;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t cw = wave * CPW + half;
    const bool valid = (z < Z) && (cw < B);
    // rotation bases: an active lane reads lane z + rho or z + rho - Z of its own group, always an active
    // lane of its own codeword; idle lanes (z >= Z) repeat an active lane's address (qc_common.h idle_alias)
    // and are read by nobody
    const int zb = lane_zb<Z, CPW>(z);
    const int base4 = (half * 32 + zb) * 4;
    const int base4m = base4 - 4 * Z;
    constexpr bool LDSROT = !EARLY && Z <= 32;
    __shared__ float Rw[LDSROT ? lay_tpb<EARLY>() : 1];  // one 64-lane rotation row per wave
    const int wrow = LDSROT ? (int)(threadIdx.x & ~63u) * 4 : 0;
    const int rb4 = base4 + wrow, rb4m = base4m + wrow;
    if constexpr (LDSROT) {
        // M0 = this wave's row, set once (tests/test_kernel_resources.py checks the built code); s_nop 0: an
        // SALU write of M0 needs one wait state before an add-TID LDS instruction reads it
        const unsigned m0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(&Rw[0]) + (unsigned)wrow);
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" ::"s"(m0) : "memory");
    }
    auto rot = [&](auto rr, float x) __attribute__((always_inline)) {  // value of lane (z + rho) mod Z
        constexpr int rho = decltype(rr)::value;
        if constexpr (rho == 0) {
            return x;
        } else {
            const int addr = sel_lanes<wrap_mask<Z, CPW>(Z - rho)>(rb4, rb4m) + 4 * rho;
            if constexpr (LDSROT) {
                // a wave's LDS operations run in order: the row serves every rotation with no wait or barrier
                asm volatile("ds_write_addtid_b32 %0" ::"v"(x) : "memory");
                return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(Rw) + addr);
            } else {
                return bperm(addr, x);
            }
        }
    };

    // APP before the first sweep = L + (+0), L = -llr, loaded in the frame every sweep ends in; lanes without
    // a codeword (z >= Z, or the empty half of the last wave) read element 0 and hold zeros
    float app[NB];
    {
        const int64_t cwbase = valid ? cw * N : 0;
        const float vmask = valid ? 1.0f : 0.0f;
        static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
            constexpr int j = decltype(jj)::value;
            constexpr int s_end = F::T.end[j];
            int t = z + s_end;
            t -= (t >= Z) ? Z : 0;
            const float x = llr[cwbase + j * Z + (valid ? t : 0)] * vmask;
            app[j] = -x + 0.0f;  // an L of -0 gives +0
        });
    }
    // check state per base row (this lane's check of the row): c2v = +0 on every edge
    float mag1[MB], mag2[MB];
    uint32_t pk[MB];  // bit (d-1-t): sign of the c2v of slot t; bits 27..31: the argmin slot
#pragma unroll
    for (int r = 0; r < MB; ++r) {
        mag1[r] = 0.0f;
        mag2[r] = 0.0f;
        pk[r] = 0u;
    }
    [[maybe_unused]] float msg[STORED ? edge_off<C>(MB) : 1];  // c2v per edge, check frame
    if constexpr (STORED) {
#pragma unroll
        for (int e = 0; e < edge_off<C>(MB); ++e) msg[e] = 0.0f;
    }
    // early stop: lane groups of the wave's codewords, the groups that have stopped (a group without a
    // codeword counts as stopped from the start), the sweeps each ran
    constexpr uint64_t ACTIVE = lane_range_mask<Z, CPW>(0, Z);
    constexpr uint64_t G0 = lane_range_mask<Z, 1>(0, Z), G1 = (CPW == 2) ? (G0 << 32) : 0;
    [[maybe_unused]] uint64_t done_groups = 0;
    [[maybe_unused]] int used_lo = iters, used_hi = iters;
    [[maybe_unused]] bool done = false;  // this lane's codeword has stopped: its APP is frozen
    if constexpr (EARLY) {
        const int64_t cw0 = ((int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * CPW;
        if (cw0 >= B) done_groups |= G0;
        if (CPW == 2 && cw0 + 1 >= B) done_groups |= G1;
        done = (done_groups >> lane) & 1ull;
    }

    for (int it = 0; it < iters; ++it) {
        static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
            constexpr int r = decltype(rr)::value;
            constexpr int d = C::DEG[r];
            [[maybe_unused]] const uint32_t idx_old = pk[r] >> 27;
            float a[d], v[d];
            static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                a[t] = rot(std::integral_constant<int, F::T.rho[r][t]>{}, app[C::COL[r][t]]);
            });
            static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                if constexpr (STORED) {
                    v[t] = a[t] - msg[edge_off<C>(r) + t];
                } else {
                    const float om = (idx_old == (uint32_t)t) ? mag2[r] : mag1[r];
                    const float old = __uint_as_float(__float_as_uint(om) | ((pk[r] << (31 - (d - 1 - t))) & 0x80000000u));
                    v[t] = a[t] - old;
                }
            });
            float mn1, mn2;
            two_min(v, mn1, mn2);
            const uint32_t tot = xor_all(v) & 0x80000000u;
            const float M1 = mag_of<NORM>(mn1, alpha, beta, clamp);
            const float M2 = mag_of<NORM>(mn2, alpha, beta, clamp);
            uint32_t sg = 0, id = 0;
            static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                constexpr int j = C::COL[r][t];
                // the min slot is one with |t_e| == min1; if several tie, min2 == min1 and M2 == M1, so neither
                // the choice nor the stored argmin can change a value
                const bool ismin = fabsf(v[t]) == mn1;
                const float mg = ismin ? M2 : M1;
                const float c = __uint_as_float(__float_as_uint(mg) | ((tot ^ __float_as_uint(v[t])) & 0x80000000u));
                if constexpr (STORED) {
                    msg[edge_off<C>(r) + t] = c;
                } else {
                    id = ismin ? (uint32_t)t : id;
                    sg = __builtin_amdgcn_alignbit(sg, __float_as_uint(c), 31);
                }
                const float nx = v[t] + c;
                if constexpr (EARLY) app[j] = done ? a[t] : nx;  // a stopped codeword only changes frame
                else app[j] = nx;
            });
            if constexpr (!STORED) {
                asm("" : "+v"(id));  // keep the argmin a small integer (else the shift folds into per-slot constants)
                mag1[r] = M1;
                mag2[r] = M2;
                pk[r] = sg | (id << 27);
            }
        });
        if constexpr (EARLY) {
            // syndrome of the hard decisions (bit = APP <= 2 * ZTHR) after the full sweep: one ballot per block
            // column in the frame it sits in, brought into each row's frame on the scalar unit
            const float thr2 = 2.0f * kZthrF32;
            uint64_t par[MB];
#pragma unroll
            for (int r = 0; r < MB; ++r) par[r] = 0;
            static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
                constexpr int j = decltype(jj)::value;
                const uint64_t b = __ballot(app[j] <= thr2) & ACTIVE;
                static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
                    constexpr int r = decltype(rr)::value;
                    constexpr int t = first_slot<C>(r, j);
                    if constexpr (t >= 0) par[r] ^= rot_lanes<Z, CPW, (C::SH[r][t] - F::T.end[j] + Z) % Z>(b);
                });
            });
            uint64_t unsat = 0;
#pragma unroll
            for (int r = 0; r < MB; ++r) unsat |= par[r];
            unsat &= ACTIVE;
            const uint64_t sat = ((unsat & G0) ? 0 : G0) | ((CPW == 2 && !(unsat & G1)) ? G1 : 0);
            const uint64_t fresh = sat & ~done_groups;
            if (fresh & G0) used_lo = it + 1;
            if (CPW == 2 && (fresh & G1)) used_hi = it + 1;
            done_groups |= fresh;
            done = (done_groups >> lane) & 1ull;
            if ((done_groups & ACTIVE) == ACTIVE) break;
        }
    }
    // epilogue indices recomputed from the thread id (opaque), so nothing but the loop state is live across
    // the loop; outputs go straight from the frame the sweeps end in
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int zo = (CPW == 2) ? (tid & 31) : (tid & 63);
    const int ho = (CPW == 2) ? ((tid >> 5) & 1) : 0;
    const int64_t cwo = (((int64_t)blockIdx.x * blockDim.x + tid) >> 6) * CPW + ho;
    if (zo < Z && cwo < B) {
        static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
            constexpr int j = decltype(jj)::value;
            constexpr int s_end = F::T.end[j];
            int t = zo + s_end;
            t -= (t >= Z) ? Z : 0;
            const int64_t o = cwo * N + j * Z + t;
            const float zz = 0.5f * app[j];
            if (bits) bits[o] = (uint8_t)(zz <= kZthrF32);
            if (soft) soft[o] = (flags & LDPC_F_SOFT_Z) ? zz : 1.0f - 1.0f / (1.0f + expf(-zz));
        });
        if (zo == 0 && iters_used) iters_used[cwo] = EARLY ? (ho ? used_hi : used_lo) : iters;
    }
}

template <class C>
static int launch_lay(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft, int32_t* used,
                      hipStream_t st) {
    constexpr int CPW = (C::Z <= 32) ? 2 : 1;
    const int64_t waves = (B + CPW - 1) / CPW;
    const bool es = (p.flags & LDPC_F_EARLY_STOP) != 0;
    const int tpb = es ? lay_tpb<true>() : lay_tpb<false>();
    const unsigned blocks = (unsigned)((waves + tpb / 64 - 1) / (tpb / 64));
    const int norm = (p.alpha != 1.0f ? NORM_ALPHA : 0) | (p.beta != 0.0f ? NORM_BETA : 0);
#define LAY(E, N) k_qc_ms_lay<C, E, N><<<blocks, tpb, 0, st>>>((const float*)llr, B, p.iters, p.clamp, p.alpha, p.beta, p.flags, bits, (float*)soft, used)
#define LAY2(N) do { if (es) LAY(true, N); else LAY(false, N); } while (0)
    switch (norm) {
        case NORM_PLAIN: LAY2(NORM_PLAIN); break;
        case NORM_ALPHA: LAY2(NORM_ALPHA); break;
        case NORM_BETA: LAY2(NORM_BETA); break;
        default: LAY2(NORM_BOTH);
    }
#undef LAY2
#undef LAY
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "layered qc kernel launch: %s", hipGetErrorString(e));
    return LDPC_OK;
}

// the compiled codes this unit serves, by lifting size (each compiled 802.11n code has its own Z, and
// qc_lookup has already matched every shift of the graph's base matrix against that code's table)
using LayLaunch = int (*)(const void*, int64_t, const ldpc_params&, uint8_t*, void*, int32_t*, hipStream_t);
static LayLaunch lay_launcher(const QCSpec* s) {
    switch (qc_z(s)) {
        case Wifi648_12::Z: return &launch_lay<Wifi648_12>;
        case Wifi1296_23::Z: return &launch_lay<Wifi1296_23>;
        default: return nullptr;
    }
}

// packed fp16 layered quantized min-sum (qc_lay_pk.hip): the compiled codes with 32 < Z <= 64
bool qc_lay_pk_serves_z(int z);
bool qc_lay_pk_exact(const ldpc_params& p);
int qc_launch_qms_lay_wifi1296_23(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft,
                                  int32_t* used, hipStream_t st);

// layered tanh sum-product (qc_lay_sp.hip): the (1944,5/6) code, Z = 81, APP resident in LDS
int qc_launch_sp_lay_wifi1944_56(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft,
                                 int32_t* used, hipStream_t st);

bool qc_lay_supports(const QCSpec* s, const ldpc_params& p) {
    if (!s || (p.flags & LDPC_F_F64)) return false;
    if (p.algo == LDPC_ALGO_TANH_SP) return qc_z(s) == Wifi1944_56::Z;
    if (!lay_launcher(s)) return false;
    if (p.algo == LDPC_ALGO_QMIN_SUM) return qc_lay_pk_serves_z(qc_z(s)) && qc_lay_pk_exact(p);
    return p.algo == LDPC_ALGO_MIN_SUM;
}

int qc_lay_decode(const QCSpec* s, const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft,
                  int32_t* iters_used, hipStream_t st) {
    if (!qc_lay_supports(s, p)) return set_error(LDPC_EUNSUPPORTED, "no layered kernel for this code / algorithm");
    if (B <= 0) return LDPC_OK;
    if (p.algo == LDPC_ALGO_QMIN_SUM) return qc_launch_qms_lay_wifi1296_23(llr, B, p, bits, soft, iters_used, st);
    if (p.algo == LDPC_ALGO_TANH_SP) return qc_launch_sp_lay_wifi1944_56(llr, B, p, bits, soft, iters_used, st);
    return lay_launcher(s)(llr, B, p, bits, soft, iters_used, st);
}

}  // namespace ldpc
