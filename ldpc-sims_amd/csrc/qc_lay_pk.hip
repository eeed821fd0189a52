// qc_lay_pk.hip — layered (row-serial) quantized min-sum for the 802.11n QC codes with 32 < Z <= 64, that is
// (1296,2/3): TWO codewords per lane as an fp16 pair, one codeword pair per wave (gfx950).
//
// The schedule and its integer specification: include/ldpc_abi.h LDPC_F_LAYERED (quantized form), DESIGN.md §3.9.
// The kernel joins qc_lay.hip's dataflow with qc_pk.hip's arithmetic:
//   * lane <-> lifting index z (54 of 64 lanes active); the low / high fp16 of every register are codewords 2w and
//     2w + 1 of wave w.  Every value is an integer of magnitude <= app_max + 2 qmax <= 2047, so each fp16
//     operation is exact and one v_pk_* instruction advances both codewords.
//   * APP[NB] packed in VGPRs in the FLOATING FRAME of LayFrames<C> (qc_lay_frames.h): a column sits in the check
//     frame of the last base row that touched it and is rotated by the compile-time rho on the way into the
//     next one — at most one ds_bpermute per edge per sweep, and that one moves both codewords.  LLRs are loaded,
//     quantized in fp32 and packed in the frame every sweep ends in (end[j]); the outputs are stored from it: no
//     rotation at either end.
//   * the check state never rotates: one packed c2v register per edge, at early stop too.  The compressed form (per
//     base row the two packed magnitudes, a word of argmin flags and one of c2v signs; 88-89 VGPRs) was built and
//     measured: its 12 extra VALU instructions per edge leave 1.03x of the flooding kernel where the stored form has
//     1.52x (profiles/layered/ab_q5*.json).
//   * LDS carries nothing but ds_bpermute's transport: there are no L rows (APP is the only per-variable state).
// Zero has no sign in the specification; a register here may hold -0.  A zero-magnitude t_e makes min1 = 0, so
// every OTHER output of its check is +-0, and its own output's sign is the product of the others' signs: no
// integer value depends on the sign of a zero.  Hard decisions are `< 0` compares, false for -0.
#include "qc_lay_frames.h"
#include "qc_pk_ops.h"

#include <cstdint>

namespace ldpc {

#ifndef QC_LAY_PK_WAVES_PER_SIMD
#define QC_LAY_PK_WAVES_PER_SIMD 4  // 128 VGPRs: 24 APP + 88 c2v + a row's transients
#endif
#ifndef QC_LAY_PK_WAVES_PER_SIMD_EARLY
#define QC_LAY_PK_WAVES_PER_SIMD_EARLY 3  // stored state + the all-rows syndrome: 161-163 VGPRs (at 4 waves it spills 25)
#endif
#ifndef QC_LAY_PK_TPB_EARLY
#define QC_LAY_PK_TPB_EARLY 64  // early stop: one-wave workgroups leave the CU as they finish (as QC_PK_TPB_EARLY)
#endif
template <bool EARLY>
constexpr int lay_pk_tpb() { return EARLY ? QC_LAY_PK_TPB_EARLY : 256; }

template <class C, bool EARLY, bool BETA>
__global__ __launch_bounds__(256, EARLY ? QC_LAY_PK_WAVES_PER_SIMD_EARLY : QC_LAY_PK_WAVES_PER_SIMD) void k_qc_qms_lay(
    const float* __restrict__ llr, int64_t B, int iters, float qmax, float app_max, float beta, float qinv, int flags,
    uint8_t* __restrict__ bits, float* __restrict__ soft, int32_t* __restrict__ iters_used) {
    constexpr int Z = C::Z, NB = C::NB, MB = C::MB, N = NB * Z;
    static_assert(Z > 32 && Z <= 64, "one codeword pair per wave");
    constexpr int NE = edge_off<C>(MB);
    using F = LayFrames<C>;
    const int z = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t cw0 = wave * 2;  // low fp16: cw0, high: cw0 + 1
    // rotation bases: an active lane reads lane z + rho or z + rho - Z, always an active lane; idle lanes
    // (z >= Z) repeat an active lane's address (qc_common.h idle_alias) and are read by nobody
    const int base4 = lane_zb<Z, 1>(z) * 4;
    const int base4m = base4 - 4 * Z;
    auto rot = [&](auto rr, uint32_t x) __attribute__((always_inline)) {  // value of lane (z + rho) mod Z
        constexpr int rho = decltype(rr)::value;
        if constexpr (rho == 0) return x;
        else return pbperm(sel_lanes<wrap_mask<Z, 1>(Z - rho)>(base4, base4m) + 4 * rho, x);
    };
    // packed constants (SGPRs)
    const uint32_t QM = pk2(qmax, qmax), AM = pk2(app_max, app_max), NAM = pk2(-app_max, -app_max);
    [[maybe_unused]] const uint32_t BT = pk2(beta, beta);

    // APP before the first sweep = L = -sat(rint(llr / qstep), qmax) (the flooding kernels' quantizer, in fp32),
    // loaded in the frame every sweep ends in; lanes and halves without a codeword hold zeros
    uint32_t app[NB];
    {
        const bool v0 = (z < Z) && (cw0 < B), v1 = (z < Z) && (cw0 + 1 < B);
        static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
            constexpr int j = decltype(jj)::value;
            int t = z + F::T.end[j];
            t -= (t >= Z) ? Z : 0;
            const int64_t o = (int64_t)j * Z + t;
            const float x0 = v0 ? llr[cw0 * N + o] : 0.0f;
            const float x1 = v1 ? llr[(cw0 + 1) * N + o] : 0.0f;
            const float q0 = fminf(fmaxf(rintf(x0 * qinv), -qmax), qmax);
            const float q1 = fminf(fmaxf(rintf(x1 * qinv), -qmax), qmax);
            app[j] = pk2(-q0, -q1);
        });
    }
    // check state: the packed c2v of every edge of this lane's checks (check frame, never rotated), 0 at the start
    uint32_t msg[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) msg[e] = 0u;
    // early stop (wave-uniform): 0xffff in the half of a stopped codeword — an absent one counts as stopped from
    // the start — and the sweeps each ran
    constexpr uint64_t ACTIVE = lane_range_mask<Z, 1>(0, Z);
    [[maybe_unused]] uint32_t dmask = 0;
    [[maybe_unused]] int used0 = iters, used1 = iters;
    if constexpr (EARLY) {
        const int64_t w0 = ((int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * 2;
        dmask = (w0 >= B ? 0x0000ffffu : 0u) | (w0 + 1 >= B ? 0xffff0000u : 0u);
    }

    for (int it = 0; it < iters && !(EARLY && dmask == 0xffffffffu); ++it) {
        static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
            constexpr int r = decltype(rr)::value;
            constexpr int d = C::DEG[r];
            constexpr int e0 = edge_off<C>(r);
            uint32_t in[d], v[d], a[d];
            static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                in[t] = rot(std::integral_constant<int, F::T.rho[r][t]>{}, app[C::COL[r][t]]);
            });
            static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                v[t] = psub(in[t], msg[e0 + t]);   // t_e: exact, |t_e| <= app_max + qmax; not saturated
                a[t] = pmin(v[t] & kMag2, QM);     // the magnitude entering the minima is capped at qmax
                if constexpr (BETA) a[t] = pmax(psub(a[t], BT), 0u);  // max(a - beta, 0): monotone, commutes with min
            });
            uint32_t mn1, mn2;
            two_min_pk(a, mn1, mn2);
            const uint32_t X = mn1 ^ mn2 ^ (xor_all_u(v) & kSign2);  // sign product folded in
            static_for<0, d>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                constexpr int j = C::COL[r][t];
                // min(a, mn2) is mn1 for a strict minimum and mn2 otherwise (ties: mn1 == mn2): XOR with mn1 ^ mn2
                // gives the OTHER minimum, bit for bit (qc_pk.hip)
                const uint32_t c = __builtin_amdgcn_bitop3_b32(X ^ pmin(a[t], mn2), v[t], kSign2, 0x78);  // other ^ (v & sign)
                msg[e0 + t] = c;
                const uint32_t nx = pmin(pmax(padd(v[t], c), NAM), AM);
                // a stopped codeword's half changes frame but not value
                if constexpr (EARLY) app[j] = __builtin_amdgcn_bitop3_b32(nx, in[t], dmask, 0xd8);
                else app[j] = nx;
            });
        });
        if constexpr (EARLY) {
            // syndrome of the hard decisions (bit = APP < 0) after the full sweep, per fp16 half: one ballot per
            // block column in the frame it sits in, brought into each row's frame on the scalar unit
            uint32_t fresh = 0;
            static_for<0, 2>([&](auto kk) __attribute__((always_inline)) {
                constexpr int k = decltype(kk)::value;
                uint64_t par[MB];
#pragma unroll
                for (int r = 0; r < MB; ++r) par[r] = 0;
                static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
                    constexpr int j = decltype(jj)::value;
                    const uint64_t b = __ballot(as_h2(app[j])[k] < (_Float16)0) & ACTIVE;
                    static_for<0, MB>([&](auto rr) __attribute__((always_inline)) {
                        constexpr int r = decltype(rr)::value;
                        constexpr int t = first_slot<C>(r, j);
                        if constexpr (t >= 0) par[r] ^= rot_lanes<Z, 1, (C::SH[r][t] - F::T.end[j] + Z) % Z>(b);
                    });
                });
                uint64_t unsat = 0;
#pragma unroll
                for (int r = 0; r < MB; ++r) unsat |= par[r];
                if (!(unsat & ACTIVE)) fresh |= 0xffffu << (16 * k);
            });
            fresh &= ~dmask;
            if (fresh & 0x0000ffffu) used0 = it + 1;
            if (fresh & 0xffff0000u) used1 = it + 1;
            dmask |= fresh;
        }
    }
    // epilogue indices recomputed from the thread id (opaque), so nothing but the loop state is live across
    // the loop; outputs go straight from the frame the sweeps end in
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int zo = tid & 63;
    const int64_t c0 = (((int64_t)blockIdx.x * blockDim.x + tid) >> 6) * 2;
    const bool ok0 = zo < Z && c0 < B, ok1 = zo < Z && c0 + 1 < B;
    static_for<0, NB>([&](auto jj) __attribute__((always_inline)) {
        constexpr int j = decltype(jj)::value;
        int t = zo + F::T.end[j];
        t -= (t >= Z) ? Z : 0;
        const int64_t o = (int64_t)j * Z + t;
        const h2 hv = as_h2(app[j]);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k == 0 ? ok0 : ok1) {
                const int64_t oo = (c0 + k) * N + o;
                const float zz = 0.5f * (float)hv[k];
                if (bits) bits[oo] = (uint8_t)(zz <= kZthrF32);  // APP < 0: zz <= -0.5; a -0 is not
                if (soft) soft[oo] = (flags & LDPC_F_SOFT_Z) ? zz : 1.0f - 1.0f / (1.0f + expf(-zz));
            }
        }
    });
    if (zo == 0 && iters_used) {
        if (ok0) iters_used[c0] = EARLY ? used0 : iters;
        if (ok1) iters_used[c0 + 1] = EARLY ? used1 : iters;
    }
}

template <class C>
static int launch_qms_lay(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft, int32_t* used,
                          hipStream_t st) {
    const bool es = (p.flags & LDPC_F_EARLY_STOP) != 0;
    const int64_t waves = (B + 1) / 2;
    const float qm = (float)p.qmax, am = (float)p.app_max, b = p.beta, qi = 1.0f / p.qstep;
    const int tpb = es ? lay_pk_tpb<true>() : lay_pk_tpb<false>();
    const unsigned blocks = (unsigned)((waves + tpb / 64 - 1) / (tpb / 64));
    const float* x = (const float*)llr;
    float* sf = (float*)soft;
#define LAYPK(E, BT) k_qc_qms_lay<C, E, BT><<<blocks, tpb, 0, st>>>(x, B, p.iters, qm, am, b, qi, p.flags, bits, sf, used)
    if (b != 0.0f) {
        if (es) LAYPK(true, true); else LAYPK(false, true);
    } else {
        if (es) LAYPK(true, false); else LAYPK(false, false);
    }
#undef LAYPK
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "packed layered qc kernel launch: %s", hipGetErrorString(e));
    return LDPC_OK;
}

// fp16 holds every integer up to 2048 exactly; the largest value formed is t_e + c2v[e] before its saturation
bool qc_lay_pk_exact(const ldpc_params& p) { return (int64_t)p.app_max + 2 * (int64_t)p.qmax <= 2047; }
bool qc_lay_pk_serves_z(int z) { return z == Wifi1296_23::Z; }

int qc_launch_qms_lay_wifi1296_23(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft,
                                  int32_t* used, hipStream_t st) {
    return launch_qms_lay<Wifi1296_23>(llr, B, p, bits, soft, used, st);
}

}  // namespace ldpc
