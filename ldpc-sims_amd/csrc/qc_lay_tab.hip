// qc_lay_tab.hip — layered (row-serial) float min-sum for ANY quasi-cyclic code with one circulant per block
// (LDPC_F_LAYERED, the schedule of include/ldpc_abi.h unchanged).  kernel_path "qct-z<Z>-layered".
//
// The compiled layered kernels (qc_lay.hip, qc_lay_pk.hip, qc_lay_sp.hip) take shifts, columns and row degrees from
// a template; this one reads them from a device table at run time, so it serves every lifting ldpc_graph_create
// recognises that has no compiled table: the other 802.11n codes, 802.16e, protographs with punctured columns, a
// base matrix under design.  Each block is one circulant, so the Z checks of a base row touch disjoint variables
// and run in parallel with the serial result, bit for bit.
//
// One workgroup of 256 threads decodes CPG = max(1, 256 / Z) codewords for all sweeps in one launch; thread t owns
// (codeword t / Z, check position t mod Z) of every base row (Z > 256: one codeword, positions t, t + 256, ...).
//   APP          in LDS for the whole decode, natural order [codeword][column][variable].  A layer gathers each edge
//                from slot (p + shift) mod Z of its column and scatters t + c2v to the address it gathered from: one
//                lane touches a slot per layer, so one workgroup barrier per layer orders everything.  Column Z +
//                shift and Z - shift are wave-uniform (one table word per edge, scalar loads through the constant
//                address space); the per-lane part is the wrap select (p >= Z - shift ? base - Z : base).  The array
//                starts one row into the allocation, so the wrapped base is never negative.
//   check state  in LDS, three words per check: M1 = mag(min1), M2 = mag(min2), and the c2v sign of slot t in bit t
//                with the argmin slot in bits 27..31 (hence row degree <= 27), layout [row][word][codeword Z + p] so
//                a wave's accesses are consecutive.  The old c2v of slot t is (t == argmin ? M2 : M1) with its sign
//                bit: the bits of a stored message.
//   row          in registers.  The degree d is a run-time scalar and the slot loop is unrolled to the DMAX bucket
//                (8, 16, 27) with slots >= d skipped by scalar branches, so t[] keeps static indices (no scratch);
//                skipped slots hold +inf, which enters neither the minima nor the sign.  The gathers of a row are
//                issued before the first is used.
//   early stop   after the sweep's last barrier every check lane reads its edges' APP again and XORs the hard
//                decisions; an unsatisfied check raises its codeword's flag and the workgroup's in LDS, read behind
//                one more barrier (two flag rows, alternating by sweep, so clearing never meets a reader).  A stopped
//                codeword stops storing; the workgroup leaves on the pooled flag only.
//   load, store  over all 256 threads in element order (coalesced), from and to LDS; a missing codeword of the last
//                group loads zeros, never stores and counts as stopped.
// LDS: CPG (4 (n + Z) + 12 m) bytes plus the flags; CPG is lowered until that fits, and a code whose single codeword
// does not fit is refused (qct_why).
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "qc_common.h"

namespace ldpc {

using tab32 = const __attribute__((address_space(4))) int32_t;  // uniform index -> scalar load (as ira_common.h)

constexpr int kTabLanes = 256, kTabMaxDeg = 27;
// LDS of a gfx950 workgroup; the slack is left to the compiler's own words
constexpr size_t kTabLds = 160 * 1024, kTabLdsSlack = 256;

// Table, per base row: the degree d, then one word per block in ascending column, (column Z + shift) in bits 0..15
// and (Z - shift) above them; kTabMaxDeg zero words follow the last row, so a row's DMAX words are loaded without a
// bound.  One word per edge rather than a (column Z, shift) pair: a scalar load and an LDS read share a counter, so a
// table load between two gathers makes the second wait for the first; with a word per edge the row's entries (at most
// 27 SGPRs) are all loaded first.  column Z + shift < n < 65536 whenever a codeword fits LDS.
struct QCTSpec {
    int mb, nb, z, dmax, dmin, device;
    int32_t* d_tab;
};

// the row degree made opaque, once per phase of a row: compared once per row and kept, the 27 slot conditions
// (an SGPR pair each) overflow the SGPRs; as a fresh scalar each is an s_cmp at its branch
__device__ __forceinline__ int tab_deg(int d) {
    asm volatile("" : "+s"(d));
    return d;
}
// the APP word this lane's check (position pk of its codeword, base pb, wrapped base pw = pb - Z) has on entry e
// (e is made opaque at each use: unpacked once per row and kept, the two halves of 27 entries overflow the SGPRs)
__device__ __forceinline__ int tab_slot(int e, int pk, int pb, int pw) {
    asm volatile("" : "+s"(e));
    return (pk >= (e >> 16) ? pw : pb) + (e & 0xffff);
}

struct TabArgs {
    tab32* tab;
    int mb, n, Z, cpg;
    const float* llr;
    int64_t B;
    int iters;
    float clamp, alpha, beta;
    uint8_t* bits;
    float* soft;
    int32_t* used;
    int soft_z;
};

template <int DMAX, bool EARLY, int NORM>
__global__ __launch_bounds__(kTabLanes) void k_qc_ms_lay_tab(TabArgs a) {
    static_assert(DMAX <= kTabMaxDeg, "slot signs and the argmin share one word");
    extern __shared__ float lds[];
    const int Z = a.Z, n = a.n, cpg = a.cpg, mb = a.mb;
    const int CZ = cpg * Z;               // checks of one base row in this workgroup
    const int npos = (CZ + kTabLanes - 1) / kTabLanes;  // 1 unless Z > 256
    float* const A = lds;                 // APP at A[Z + c n + column Z + variable]
    uint32_t* const S = reinterpret_cast<uint32_t*>(lds + (size_t)cpg * (n + Z));  // [row][word][c Z + p]
    uint32_t* const Fl = S + (size_t)3 * mb * CZ;  // early stop: [sweep parity][cpg codeword flags, workgroup flag]
    const int tid = threadIdx.x;
    const int cq = Z <= kTabLanes ? tid / Z : 0;
    const int c = cq < cpg ? cq : 0;      // idle threads (tid >= CZ) own nothing
    const int p = tid - cq * Z;
    const int64_t cw0 = (int64_t)blockIdx.x * cpg;
    const int64_t left = (a.B - cw0) * n;
    const int nel = left < (int64_t)cpg * n ? (int)left : cpg * n;  // elements of the codewords this group has

    // APP before the first sweep = L + (+0), L = -llr; zero check states (c2v = +0 on every edge)
    const float* const x = a.llr + cw0 * n;
    for (int i = tid; i < cpg * n; i += kTabLanes) A[Z + i] = i < nel ? -x[i] + 0.0f : 0.0f;
    for (int i = tid; i < 3 * mb * CZ; i += kTabLanes) S[i] = 0u;
    bool done = cq >= cpg || cw0 + c >= a.B;  // this thread's codeword has stopped (or does not exist): frozen
    int used = a.iters;
    __syncthreads();

    const float thr2 = 2.0f * kZthrF32;
    for (int it = 0; it < a.iters; ++it) {
        uint32_t* const F = Fl + (it & 1) * (cpg + 1);
        if (EARLY && tid <= cpg) F[tid] = 0u;  // the layers' barriers order this before the syndrome's writes
        tab32* row = a.tab;
        for (int r = 0; r < mb; ++r) {
            const int d = row[0];
            int w[DMAX];  // the row's entries, all loaded before the first gather (the table's end is padded)
            static_for<0, DMAX>([&](auto SS) __attribute__((always_inline)) { w[decltype(SS)::value] = row[1 + decltype(SS)::value]; });
            for (int k = 0; k < npos; ++k) {
                const int u = tid + k * kTabLanes, pk = p + k * kTabLanes;
                if (u < CZ && !done) {
                    const int pb = Z + c * n + pk, pw = pb - Z;
                    const int su = 3 * r * CZ + u;
                    int ix[DMAX];
                    float raw[DMAX], t[DMAX];
                    const int d1 = tab_deg(d), d2 = tab_deg(d), d3 = tab_deg(d);
                    static_for<0, DMAX>([&](auto SS) __attribute__((always_inline)) {
                        constexpr int s = decltype(SS)::value;
                        if (s < d1) {
                            ix[s] = tab_slot(w[s], pk, pb, pw);
                            raw[s] = A[ix[s]];
                        }
                    });
                    const float M1o = u2f(S[su]), M2o = u2f(S[su + CZ]);
                    const uint32_t wo = S[su + 2 * CZ], ido = wo >> 27;
                    static_for<0, DMAX>([&](auto SS) __attribute__((always_inline)) {
                        constexpr int s = decltype(SS)::value;
                        if (s < d2) {
                            const float om = ido == (uint32_t)s ? M2o : M1o;
                            t[s] = raw[s] - u2f(f2u(om) | ((wo >> s) << 31));
                        } else {
                            t[s] = __builtin_inff();
                        }
                    });
                    float mn1, mn2;
                    two_min(t, mn1, mn2);
                    const uint32_t tot = xor_all(t) & 0x80000000u;
                    const float M1 = mag_of<NORM>(mn1, a.alpha, a.beta, a.clamp);
                    const float M2 = mag_of<NORM>(mn2, a.alpha, a.beta, a.clamp);
                    uint32_t sg = 0, id = 0;
                    static_for<0, DMAX>([&](auto SS) __attribute__((always_inline)) {
                        constexpr int s = decltype(SS)::value;
                        if (s < d3) {
                            // the min slot is one with |t| == min1; if several tie, min2 == min1 and M2 == M1, so
                            // neither the choice nor the stored argmin can change a value
                            const bool ismin = fabsf(t[s]) == mn1;
                            const uint32_t sb = (tot ^ f2u(t[s])) & 0x80000000u;
                            id = ismin ? (uint32_t)s : id;
                            sg |= sb >> (31 - s);
                            A[ix[s]] = t[s] + u2f(f2u(ismin ? M2 : M1) | sb);
                        }
                    });
                    S[su] = f2u(M1);
                    S[su + CZ] = f2u(M2);
                    S[su + 2 * CZ] = sg | (id << 27);
                }
            }
            row += 1 + d;
            __syncthreads();
        }
        if constexpr (EARLY) {
            // the syndrome of the posteriors the sweep left, all rows: the same addresses, a decision xor per check
            bool unsat = false;
            row = a.tab;
            for (int r = 0; r < mb; ++r) {
                const int d = row[0];
                int w[DMAX];
                static_for<0, DMAX>([&](auto SS) __attribute__((always_inline)) { w[decltype(SS)::value] = row[1 + decltype(SS)::value]; });
                for (int k = 0; k < npos; ++k) {
                    const int u = tid + k * kTabLanes, pk = p + k * kTabLanes;
                    if (u < CZ && !done) {
                        const int pb = Z + c * n + pk, pw = pb - Z;
                        float raw[DMAX];
                        const int d1 = tab_deg(d), d2 = tab_deg(d);
                        static_for<0, DMAX>([&](auto SS) __attribute__((always_inline)) {
                            constexpr int s = decltype(SS)::value;
                            if (s < d1) raw[s] = A[tab_slot(w[s], pk, pb, pw)];
                        });
                        bool par = false;
                        static_for<0, DMAX>([&](auto SS) __attribute__((always_inline)) {
                            constexpr int s = decltype(SS)::value;
                            if (s < d2) par ^= raw[s] <= thr2;
                        });
                        unsat |= par;
                    }
                }
                row += 1 + d;
            }
            if (unsat) {
                F[c] = 1u;
                F[cpg] = 1u;
            }
            __syncthreads();  // also: every syndrome read of APP precedes the next sweep's stores
            if (!done && F[c] == 0u) {
                done = true;
                used = it + 1;
            }
            if (F[cpg] == 0u) break;  // the pooled flag: the same decision in every wave
        }
    }

    // z = 0.5 APP from LDS in element order: bits (np.round(p1) rule) and soft (p1 = 1 - sigmoid(z), or z)
    for (int i = tid; i < nel; i += kTabLanes) {
        const float z = 0.5f * A[Z + i];
        const int64_t o = cw0 * n + i;
        if (a.bits) a.bits[o] = (uint8_t)Num<float>::bit(z);
        if (a.soft) a.soft[o] = a.soft_z ? z : 1.0f - 1.0f / (1.0f + Num<float>::exp_(-z));
    }
    if (a.used && cq < cpg && p == 0 && cw0 + c < a.B) a.used[cw0 + c] = used;
}

// ---- host ------------------------------------------------------------------------------------------------

static size_t qct_cw_bytes(const QCTSpec* s) {  // APP (one row of slack) and the check states of one codeword
    return 4 * ((size_t)s->nb * s->z + s->z) + 12 * (size_t)s->mb * s->z;
}
static size_t qct_lds_bytes(const QCTSpec* s, int cpg) { return cpg * qct_cw_bytes(s) + 2 * (size_t)(cpg + 1) * 4; }
// codewords per workgroup: 256 / Z, fewer while they do not fit LDS; 0 when one does not
static int qct_cpg(const QCTSpec* s) {
    int cpg = std::max(1, kTabLanes / s->z);
    while (cpg > 0 && qct_lds_bytes(s, cpg) + kTabLdsSlack > kTabLds) --cpg;
    return cpg;
}

QCTSpec* qct_create(int mb, int nb, int z, const std::vector<std::vector<std::pair<int, int>>>& rows, int device) {
    std::vector<int32_t> tab;
    int dmax = 0, dmin = INT32_MAX;
    for (const auto& row : rows) {
        tab.push_back((int32_t)row.size());
        for (const auto& e : row) tab.push_back((int32_t)(((uint32_t)(e.first * z + e.second) & 0xffffu) | (uint32_t)(z - e.second) << 16));
        dmax = std::max(dmax, (int)row.size());
        dmin = std::min(dmin, (int)row.size());
    }
    tab.insert(tab.end(), kTabMaxDeg, 0);
    int32_t* d_tab = nullptr;
    if (hipMalloc((void**)&d_tab, tab.size() * 4) != hipSuccess) return nullptr;
    if (hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d_tab);
        return nullptr;
    }
    return new QCTSpec{mb, nb, z, dmax, dmin, device, d_tab};
}

void qct_free(QCTSpec* s) {
    if (!s) return;
    (void)hipFree(s->d_tab);
    delete s;
}

int qct_z(const QCTSpec* s) { return s->z; }

const char* qct_why(const QCTSpec* s) {
    static thread_local char buf[320];
    if (s->dmax > kTabMaxDeg || s->dmin < 2) {
        snprintf(buf, sizeof buf, "a quasi-cyclic graph (Z = %d) with base row degrees %d..%d: the table-driven layered "
                 "kernel serves row degrees 2..%d", s->z, s->dmin, s->dmax, kTabMaxDeg);
        return buf;
    }
    if (qct_cpg(s) < 1) {
        snprintf(buf, sizeof buf, "a quasi-cyclic graph with Z = %d, n = %d: the table-driven layered kernel keeps the "
                 "posteriors and check states of a codeword in LDS, and %zu bytes do not fit the %zu bytes of a gfx950 "
                 "workgroup", s->z, s->nb * s->z, qct_cw_bytes(s), kTabLds);
        return buf;
    }
    return nullptr;
}

bool qct_supports(const QCTSpec* s, const ldpc_params& p) {
    if (!s || p.algo != LDPC_ALGO_MIN_SUM || (p.flags & LDPC_F_F64)) return false;
    return qct_why(s) == nullptr;
}

using TabKernel = void (*)(TabArgs);
template <int DMAX>
static TabKernel tab_pick_norm(int norm, bool es) {
#define TAB_K(N) (es ? (TabKernel)k_qc_ms_lay_tab<DMAX, true, N> : (TabKernel)k_qc_ms_lay_tab<DMAX, false, N>)
    switch (norm) {
        case NORM_PLAIN: return TAB_K(NORM_PLAIN);
        case NORM_ALPHA: return TAB_K(NORM_ALPHA);
        case NORM_BETA: return TAB_K(NORM_BETA);
        default: return TAB_K(NORM_BOTH);
    }
#undef TAB_K
}

int qct_decode(const QCTSpec* s, const float* llr, int64_t B, const ldpc_params& p, uint8_t* bits, float* soft,
               int32_t* iters_used, hipStream_t st) {
    if (!qct_supports(s, p)) return set_error(LDPC_EUNSUPPORTED, "no table-driven layered kernel for this graph / algorithm");
    if (B <= 0) return LDPC_OK;
    const int norm = (p.alpha != 1.0f ? NORM_ALPHA : 0) | (p.beta != 0.0f ? NORM_BETA : 0);
    const bool es = (p.flags & LDPC_F_EARLY_STOP) != 0;
    const TabKernel fn = s->dmax <= 8 ? tab_pick_norm<8>(norm, es)
                         : s->dmax <= 16 ? tab_pick_norm<16>(norm, es) : tab_pick_norm<kTabMaxDeg>(norm, es);
    const int cpg = qct_cpg(s);
    const size_t lds = qct_lds_bytes(s, cpg);
    if (lds > 64 * 1024) {  // above 64 KiB the dynamic LDS limit must be asked for
        const hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return set_error(LDPC_EHIP, "table-driven layered kernel: %zu bytes of LDS per workgroup: %s", lds, hipGetErrorString(e));
    }
    TabArgs a{};
    a.tab = (tab32*)s->d_tab;
    a.mb = s->mb; a.n = s->nb * s->z; a.Z = s->z; a.cpg = cpg;
    a.llr = llr;
    a.B = B;
    a.iters = p.iters;
    a.clamp = p.clamp; a.alpha = p.alpha; a.beta = p.beta;
    a.bits = bits;
    a.soft = soft;
    a.used = iters_used;
    a.soft_z = (p.flags & LDPC_F_SOFT_Z) ? 1 : 0;
    fn<<<(unsigned)((B + cpg - 1) / cpg), kTabLanes, lds, st>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "table-driven layered kernel launch: %s", hipGetErrorString(e));
    return LDPC_OK;
}

}  // namespace ldpc
