// qc_es.hip — the early-stop register kernels for Z <= 64 (float min-sum: k_qc_ms_ph<C, false, true, N> for
// Z <= 32, k_qc_ms_st<C, false, true, N> above; tanh-SP: k_qc_sp_st<C, true>) in a translation unit of their
// own, built with the default scheduler (build.py): qc.hip's fixed-count kernels use iterative-ILP scheduling,
// under which these kernels' row-wise syndromes spill (A/B profiles/r03/ab/ab_ph_esrows.txt, ab_st_esrows.txt).
#include "qc_ms.h"
#include "qc_sp.h"

#include <cstdint>

namespace ldpc {

template <class C>
static int launch_ms_es(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft, int32_t* used,
                        hipStream_t st) {
    constexpr int CPW = (C::Z <= 32) ? 2 : 1;
    const int64_t waves = (B + CPW - 1) / CPW;
    const int tpb = st_tpb<true>();
    const unsigned blocks = (unsigned)((waves + tpb / 64 - 1) / (tpb / 64));
    const float* x = (const float*)llr;
    float* sf = (float*)soft;
    const int norm = (p.alpha != 1.0f ? NORM_ALPHA : 0) | (p.beta != 0.0f ? NORM_BETA : 0);
#define FE(N)                                                                                                     \
    do {                                                                                                          \
        if constexpr (C::Z <= 32)                                                                                 \
            k_qc_ms_ph<C, false, true, N><<<blocks, tpb, 0, st>>>(x, B, p.iters, p.clamp, p.alpha, p.beta, 0.f, 0.f, 1.f, p.flags, bits, sf, used); \
        else                                                                                                      \
            k_qc_ms_st<C, false, true, N><<<blocks, tpb, 0, st>>>(x, B, p.iters, p.clamp, p.alpha, p.beta, 0.f, 0.f, 1.f, p.flags, bits, sf, used); \
    } while (0)
    switch (norm) {
        case NORM_PLAIN: FE(NORM_PLAIN); break;
        case NORM_ALPHA: FE(NORM_ALPHA); break;
        case NORM_BETA: FE(NORM_BETA); break;
        default: FE(NORM_BOTH);
    }
#undef FE
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "qc kernel launch: %s", hipGetErrorString(e));
    return LDPC_OK;
}
template <class C>
static int launch_sp_es(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft, int32_t* used,
                        hipStream_t st) {
    constexpr int CPW = (C::Z <= 32) ? 2 : 1;
    const int64_t waves = (B + CPW - 1) / CPW;
    const int tpb = sp_tpb<true>();
    const unsigned blocks = (unsigned)((waves + tpb / 64 - 1) / (tpb / 64));
    // the plain pass, and beside it the a == 1 rule's pass for waves with a zero LLR
    uint32_t* zl = qc_sp_zlist();
    hipStream_t s2;
    if (const int rc = qc_sp_fork((const float*)llr, B, C::NB * C::Z, CPW, st, &s2)) return rc;
    k_qc_sp_st<C, true, 2><<<qc_sp_pass2_grid(blocks), tpb, 0, s2>>>((const float*)llr, B, p.iters, p.clamp, p.flags, bits, (float*)soft, used, zl);
    k_qc_sp_st<C, true, 1><<<blocks, tpb, 0, st>>>((const float*)llr, B, p.iters, p.clamp, p.flags, bits, (float*)soft, used, zl);
    if (const int rc = qc_sp_join(st)) return rc;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "qc kernel launch: %s", hipGetErrorString(e));
    return LDPC_OK;
}
int qc_launch_ms_es_wifi648_12(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft,
                               int32_t* used, hipStream_t st) {
    return p.algo == LDPC_ALGO_TANH_SP ? launch_sp_es<Wifi648_12>(llr, B, p, bits, soft, used, st)
                                       : launch_ms_es<Wifi648_12>(llr, B, p, bits, soft, used, st);
}
int qc_launch_ms_es_wifi1296_23(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft,
                                int32_t* used, hipStream_t st) {
    return p.algo == LDPC_ALGO_TANH_SP ? launch_sp_es<Wifi1296_23>(llr, B, p, bits, soft, used, st)
                                       : launch_ms_es<Wifi1296_23>(llr, B, p, bits, soft, used, st);
}

}  // namespace ldpc
