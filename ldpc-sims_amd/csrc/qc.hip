// qc.hip — structure-specialised quasi-cyclic (802.11n) min-sum decoder for gfx950.
//
// One wave decodes CPW codewords entirely in registers for all iterations — one launch per batch, no
// message traffic to HBM (only LLRs in, bits/soft out):
//   * lane <-> lifting index z:  lane (half, z) owns variable (j, z) of every block column j (posterior
//     APP[j] in a VGPR array indexed by compile-time j) and check (r, z) of every block row r; every
//     edge's message is kept in a VGPR.  Z <= 32: two codewords per wave (lane halves); Z <= 64: one.
//   * a circulant with shift s connects check (r, i) to variable (j, (i+s) mod Z), so both directions
//     of the exchange are lane rotations inside the codeword's lane group: ds_bpermute_b32 with a
//     2-instruction address (select between two lane-constant bases, shift folded into an immediate);
//     s == 0 circulants need no exchange at all.
//   * the graph is a compile-time constant (qc_tables.h), so every table lookup, loop bound and
//     register index is resolved at compile time.
// Arithmetic is exactly the oracle's (oracle/ldpc_oracle.c ms_f32_one / qms_one): flooding schedule,
// v2c = APP - c2v_old, APP_new = L + sum c2v in ascending check order, same tie rules, same
// normalisation/offset/clamp sequence, same hard-decision rule; so bits and soft outputs are bit-exact.
// Early stop: the syndrome of APP_it is evaluated from ballots of its hard decisions; a codeword whose
// syndrome is zero is emitted with iters_used = it.
// The kernel templates are in qc_ms.h and qc_sp.h; this unit holds the fixed-count launchers and the dispatch,
// qc_es.hip the early-stop launchers.
#include "qc_ms.h"
#include "qc_sp.h"

#include <cstdint>

namespace ldpc {

struct QCSpec {
    int mb, nb, z;
    const int* col;  // [mb][maxdc]
    const int* sh;
    const int* deg;
    int maxdc;
    const char* name;
    int (*launch_ms)(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft, int32_t* used,
                     hipStream_t st);
};

// float early-stop min-sum (qc_es.hip)
int qc_launch_ms_es_wifi648_12(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft,
                               int32_t* used, hipStream_t st);
int qc_launch_ms_es_wifi1296_23(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft,
                                int32_t* used, hipStream_t st);

// packed quantized kernels (qc_pk.hip)
int qc_launch_qms_pk_wifi648_12(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft,
                                int32_t* used, hipStream_t st);
int qc_launch_qms_pk_wifi1296_23(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft,
                                 int32_t* used, hipStream_t st);

// sliced kernels for Z > 64 (qc_sl.hip)
int qc_launch_sl_wifi1944_56(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft,
                              int32_t* used, hipStream_t st);

template <class C>
static int launch_ms(const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft, int32_t* used,
                     hipStream_t st) {
    constexpr int CPW = (C::Z <= 32) ? 2 : 1;
    const int64_t waves = (B + CPW - 1) / CPW;
    const float* x = (const float*)llr;
    float* sf = (float*)soft;
    if (p.algo == LDPC_ALGO_QMIN_SUM) {
        // two codewords per lane in packed fp16 (qc_pk.hip)
        if constexpr (std::is_same_v<C, Wifi648_12>) return qc_launch_qms_pk_wifi648_12(llr, B, p, bits, soft, used, st);
        else if constexpr (std::is_same_v<C, Wifi1296_23>) return qc_launch_qms_pk_wifi1296_23(llr, B, p, bits, soft, used, st);
        else return set_error(LDPC_EUNSUPPORTED, "no packed quantized kernel for %s", C::NAME);
    }
    if (p.flags & LDPC_F_EARLY_STOP) {  // float min-sum and tanh-SP with early stop: qc_es.hip
        if constexpr (std::is_same_v<C, Wifi648_12>) return qc_launch_ms_es_wifi648_12(llr, B, p, bits, soft, used, st);
        else return qc_launch_ms_es_wifi1296_23(llr, B, p, bits, soft, used, st);
    }
    if (p.algo == LDPC_ALGO_TANH_SP) {
        // the plain pass, and beside it the a == 1 rule's pass for waves with a zero LLR
        const int tpb = sp_tpb<false>();
        const unsigned blocks = (unsigned)((waves + tpb / 64 - 1) / (tpb / 64));
        uint32_t* zl = qc_sp_zlist();
        hipStream_t s2;
        if (const int rc = qc_sp_fork(x, B, C::NB * C::Z, CPW, st, &s2)) return rc;
        k_qc_sp_st<C, false, 2><<<qc_sp_pass2_grid(blocks), tpb, 0, s2>>>(x, B, p.iters, p.clamp, p.flags, bits, sf, used, zl);
        k_qc_sp_st<C, false, 1><<<blocks, tpb, 0, st>>>(x, B, p.iters, p.clamp, p.flags, bits, sf, used, zl);
        if (const int rc = qc_sp_join(st)) return rc;
    } else {
        const int tpb = st_tpb<false>();
        const unsigned blocks = (unsigned)((waves + tpb / 64 - 1) / (tpb / 64));
        const int norm = (p.alpha != 1.0f ? NORM_ALPHA : 0) | (p.beta != 0.0f ? NORM_BETA : 0);
#define FL(N)                                                                                                     \
    do {                                                                                                          \
        if constexpr (C::Z <= 32)                                                                                 \
            k_qc_ms_ph<C, false, false, N><<<blocks, tpb, 0, st>>>(x, B, p.iters, p.clamp, p.alpha, p.beta, 0.f, 0.f, 1.f, p.flags, bits, sf, used); \
        else                                                                                                      \
            k_qc_ms_st<C, false, false, N><<<blocks, tpb, 0, st>>>(x, B, p.iters, p.clamp, p.alpha, p.beta, 0.f, 0.f, 1.f, p.flags, bits, sf, used); \
    } while (0)
        switch (norm) {
            case NORM_PLAIN: FL(NORM_PLAIN); break;
            case NORM_ALPHA: FL(NORM_ALPHA); break;
            case NORM_BETA: FL(NORM_BETA); break;
            default: FL(NORM_BOTH);
        }
#undef FL
    }

    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "qc kernel launch: %s", hipGetErrorString(e));
    return LDPC_OK;
}

#define SPEC(C) {C::MB, C::NB, C::Z, &C::COL[0][0], &C::SH[0][0], &C::DEG[0], C::MAXDC, C::NAME, &launch_ms<C>}
#define SPEC_SL(C, F) {C::MB, C::NB, C::Z, &C::COL[0][0], &C::SH[0][0], &C::DEG[0], C::MAXDC, C::NAME, &F}
static const QCSpec kSpecs[] = {SPEC(Wifi648_12), SPEC(Wifi1296_23), SPEC_SL(Wifi1944_56, qc_launch_sl_wifi1944_56)};
#undef SPEC_SL
#undef SPEC

const QCSpec* qc_lookup(int mb, int nb, int z, const int32_t* shifts) {
    for (const QCSpec& s : kSpecs) {
        if (s.mb != mb || s.nb != nb || s.z != z) continue;
        bool eq = true;
        for (int r = 0; r < mb && eq; ++r) {
            int t = 0;
            for (int j = 0; j < nb; ++j) {
                const int want = (t < s.deg[r] && s.col[r * s.maxdc + t] == j) ? s.sh[r * s.maxdc + t] : -1;
                if (want >= 0) ++t;
                if (shifts[(size_t)r * nb + j] != want) { eq = false; break; }
            }
        }
        if (eq) return &s;
    }
    return nullptr;
}

int qc_z(const QCSpec* s) { return s ? s->z : 0; }

bool qc_supports(const QCSpec* s, const ldpc_params& p) {
    if (!s) return false;
    if (p.flags & LDPC_F_F64) return false;
    if (p.algo == LDPC_ALGO_TANH_SP) return true;  // Z <= 64: k_qc_sp_st; Z = 81: k_qc_sp_sl (both with early stop)
    return p.algo == LDPC_ALGO_MIN_SUM || p.algo == LDPC_ALGO_QMIN_SUM;
}

// tanh-SP: the zero-LLR list of the two-pass kernels (qc_sp_zlist, qc_sp_zflag): a count, at most one id per
// codeword, then one flag byte per codeword
size_t qc_workspace(const QCSpec*, int64_t B, const ldpc_params& p) {
    return p.algo == LDPC_ALGO_TANH_SP ? (size_t)((4 * (B + 1) + B + 255) & ~(int64_t)255) : 0;
}

uint32_t*& qc_sp_zlist() {
    static thread_local uint32_t* f = nullptr;
    return f;
}

// one wave per unit of `cpu` (<= 8) consecutive codewords (n LLRs each, row-major): flag = bit j set when codeword j
// of the unit holds an exact-zero LLR (+-0; the a == 1 rule is per codeword, common.h), the unit listed once when any
// is.  Reads the batch's LLRs once (B n 4 bytes) so that the a == 1 rule's units can run beside the plain pass
// instead of after it.
__global__ __launch_bounds__(256) void k_sp_zero_scan(const float* __restrict__ llr, int64_t B, int n, int cpu,
                                                      int64_t units, uint32_t* __restrict__ zlist) {
    const int64_t u = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (u >= units) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int64_t c0 = u * cpu, c1 = (c0 + cpu < B) ? c0 + cpu : B;
    uint32_t mask = 0;
    for (int64_t c = c0; c < c1; ++c) {
        const float* p = llr + c * n;
        bool z = false;
        int64_t i0 = 0;
        if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const float4* p4 = reinterpret_cast<const float4*>(p);
            const int64_t n4 = n >> 2;
            for (int64_t i = lane; i < n4; i += 64) {
                const float4 v = p4[i];
                z |= (v.x == 0.0f) | (v.y == 0.0f) | (v.z == 0.0f) | (v.w == 0.0f);
            }
            i0 = n4 << 2;
        }
        for (int64_t i = i0 + lane; i < n; i += 64) z |= p[i] == 0.0f;
        mask |= (__ballot(z) != 0 ? 1u : 0u) << (c - c0);
    }
    if (lane == 0) {
        qc_sp_zflag(zlist, B)[u] = (uint8_t)mask;
        if (mask) zlist[1 + atomicAdd(zlist, 1u)] = (uint32_t)u;
    }
}

int qc_sp_fork(const float* llr, int64_t B, int n, int cpu, hipStream_t st, hipStream_t* s2) {
    uint32_t* zl = qc_sp_zlist();
    if (!zl) return set_error(LDPC_EHIP, "tanh-SP zero-LLR pass: no workspace");
    if (cpu < 1 || cpu > 8) return set_error(LDPC_EHIP, "tanh-SP zero-LLR pass: %d codewords per unit (flag byte holds 8)", cpu);
    if (hipMemsetAsync(zl, 0, 4, st) != hipSuccess) return set_error(LDPC_EHIP, "zero-LLR list reset failed");
    const int64_t units = (B + cpu - 1) / cpu;
    k_sp_zero_scan<<<(unsigned)((units + 3) / 4), 256, 0, st>>>(llr, B, n, cpu, units, zl);
    return aux_fork(st, s2);
}

int qc_sp_join(hipStream_t st) { return aux_join(st); }

int qc_decode(const QCSpec* s, const void* llr, int64_t B, const ldpc_params& p, uint8_t* bits, void* soft,
              int32_t* used, char* ws, hipStream_t st) {
    qc_sp_zlist() = (uint32_t*)ws;
    const int rc = s->launch_ms(llr, B, p, bits, soft, used, st);
    qc_sp_zlist() = nullptr;
    return rc;
}

}  // namespace ldpc
