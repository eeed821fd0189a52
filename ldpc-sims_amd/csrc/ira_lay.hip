// ira_lay.hip — layered min-sum for IRA codes with the DVB-S2 structure (LDPC_F_LAYERED on an IRA graph, the
// schedule of include/ldpc_abi.h: a layer is one row a of the relabelled code, its 360 checks (a, b) run in parallel
// from the posteriors as they stood before the layer).  kernel_path "ira-z360-layered"; DESIGN.md §3.9.
//
// One workgroup of kIraLanes threads decodes one codeword at a time for all its sweeps in one launch; lane b owns
// position b of every row.  Where the data lives:
//   information posteriors   k floats in LDS for the whole decode, natural (group, m) order.  Slot i of check (a, b)
//                            gathers A[g_i 360 + (b - s_i) mod 360] — a contiguous window with one wrap across the
//                            lanes — and scatters to the address it gathered.  (g_i, s_i): scalar loads of the row's
//                            table entries through the constant address space.
//   parity posteriors        parity (a, b) is touched by lane b in layer a (its own check) and by lane b in layer
//                            a + 1 (the staircase): read once per sweep from the slot's workspace (row-major (a, b)),
//                            carried in a register across the layer's barrier, stored once.  Row q - 1's second
//                            touch is lane b + 1 in the NEXT sweep's layer 0: that row lives in a 360-float LDS row.
//   check states             the flooding kernels' 12-byte IraState, one dwordx3 load and one store per check and
//                            sweep, in the slot's workspace.  Nothing in layer a + 1's state or parity posterior
//                            depends on layer a, so they are loaded two layers ahead: the chain of a layer is LDS
//                            gather -> row arithmetic -> LDS scatter -> barrier, with no global round trip on it.
//                            Sweep 0 takes a zero state through a uniform condition: the workspace is never cleared
//                            (the slot's next codeword reuses it).
// A row in which a group appears twice (8 of the 90 rows of DVB-S2 rate 1/2) gives that group's variables two edges
// in the layer: the lanes of the pair's first slot publish new - old to an LDS row indexed by m, a barrier, and the
// lanes of its second slot store APP + (d1 + d2) — a commutative sum, so no lane order enters the result.
// Grid: min(B, slots) workgroups, slots = CUs x resident workgroups per CU (the occupancy query at this LDS size);
// workgroup w decodes codewords w, w + slots, ... in the workspace of slot w (16 M bytes).
#include <stdlib.h>

#include <algorithm>

#include "common.h"
#include "ira_common.h"

namespace ldpc {

// LDS of a gfx950 workgroup (the library's only target); kLayLdsSlack is left to the compiler's own words
// (__syncthreads_or)
constexpr size_t kLayLds = 160 * 1024, kLayLdsSlack = 256;

struct LayArgs {
    cint32 *cnl, *clay;
    int q, k, n, M;
    const float* llr;
    int64_t B;
    int iters;
    float clamp, alpha, beta;
    char* ws;            // slot w: IraState[M] at w * ws_slot, then float[M] parity posteriors at + ws_par
    size_t ws_slot, ws_par;
    uint8_t* bits;
    float* soft;
    int32_t* used;
    int soft_z;
};

enum { LAY_PLAIN = 0, LAY_ALPHA = 1, LAY_BETA = 2, LAY_BOTH = 3 };
// ms_mag with the operations that change nothing left out (alpha == 1: the product is exact; beta == 0: m - 0 == m
// and m >= +0): the same bits
template <int NORM>
__device__ __forceinline__ float lay_mag(float m, float alpha, float beta, float clamp) {
    if constexpr (NORM == LAY_PLAIN) return fminf(m, clamp);
    else if constexpr (NORM == LAY_ALPHA) return fminf(alpha * m, clamp);
    else if constexpr (NORM == LAY_BETA) return fminf(fmaxf(m - beta, 0.0f), clamp);
    else return ms_mag(m, alpha, beta, clamp);
}

template <int MAXR, int NORM, bool ES>
__global__ __launch_bounds__(kIraLanes) void k_ira_lay(LayArgs a) {
    extern __shared__ float lds[];
    float* const A = lds;             // information posteriors [k]
    float* const Hn = lds + a.k;      // posteriors of parity row q - 1 [360]
    float* const D = Hn + kIZ;        // new - old of the first slot of each pair of the running row [pairs][360]
    const int pos = threadIdx.x, p = min(pos, kIZ - 1);
    const bool live = pos < kIZ;
    const int q = a.q, k = a.k, M = a.M;
    IraState* const S = reinterpret_cast<IraState*>(a.ws + (size_t)blockIdx.x * a.ws_slot);
    float* const P = reinterpret_cast<float*>(a.ws + (size_t)blockIdx.x * a.ws_slot + a.ws_par);

    // what a layer needs from the workspace: its state and the posterior of its own parity (row q - 1's is in Hn)
    struct Pre {
        IraState st;
        float own;
    };
    // slot s of row `row` at this lane: the address it gathers and scatters
    auto slot_idx = [&](int e) __attribute__((always_inline)) {
        int m = p - ((e >> 8) & 0x1ff);
        m += m < 0 ? kIZ : 0;
        return (e & 0xff) * kIZ + m;
    };

    for (int64_t cw = blockIdx.x; cw < a.B; cw += gridDim.x) {
        const float* __restrict__ x = a.llr + cw * a.n;
        // APP = L + (+0), L = -llr: information part to LDS as it lies, parity j = a + q b to P[a][b]
        for (int v = pos; v < k; v += kIraLanes) A[v] = -x[v] + 0.0f;
        for (int j = pos; j < M; j += kIraLanes) P[(j % q) * kIZ + j / q] = -x[k + j] + 0.0f;
        __syncthreads();
        if (live) Hn[pos] = P[(q - 1) * kIZ + pos];
        __syncthreads();

        int used = a.iters;
        for (int it = 0; it < a.iters; ++it) {
            // no load sits in a branch (a row past the end repeats the last one; sweep 0 loads a state it does not
            // use), so the compiler can count the loads in flight and wait for the oldest only
            auto fetch = [&](int ra) __attribute__((always_inline)) {
                return Pre{ira_ld_i(S, min(ra, q - 1) * kIZ + p), P[min(ra, q - 2) * kIZ + p]};
            };
            Pre n1 = fetch(0), n2 = fetch(1);
            float carry = 0.0f;  // the posterior of parity (ra - 1, b) as layer ra - 1 left it
            for (int ra = 0; ra < q; ++ra) {
                const Pre cu = n1;
                n1 = n2;
                n2 = fetch(ra + 2);
                const int lay = a.clay[ra];
                const int R = lay & 0xff;
                cint32* row = a.cnl + ra * kICS;
                int ent[MAXR], idx[MAXR];
                float raw[MAXR], t[MAXR];
                static_for<0, MAXR>([&](auto SS) __attribute__((always_inline)) { ent[decltype(SS)::value] = row[decltype(SS)::value]; });
                // MAXR <= 8: every slot gathers (one past R reads the zero-padded entry: A[p], unused), so no LDS
                // read sits in a branch
                static_for<0, MAXR>([&](auto SS) __attribute__((always_inline)) {
                    constexpr int s = decltype(SS)::value;
                    if (MAXR <= 8 || s < R) {
                        idx[s] = slot_idx(ent[s]);
                        raw[s] = A[idx[s]];
                    }
                });
                const bool last = ra == q - 1;
                const bool has_prev = ra > 0 || p > 0;  // check 0 has no p_{-1}
                const float ap0 = last ? Hn[p] : cu.own;
                const float ap1 = ra == 0 ? Hn[max(p - 1, 0)] : carry;
                __builtin_amdgcn_sched_barrier(0);  // the loads of layer ra + 2 and every gather in flight first
                const IraState st = it > 0 ? cu.st : IraState{0.0f, 0.0f, 0u};
                float min1 = __builtin_inff(), min2 = __builtin_inff();
                int arg = -1;
                uint32_t sgn = 0;
                auto take = [&](float v, int s) __attribute__((always_inline)) {
                    const float m = fabsf(v);
                    sgn ^= f2u(v);
                    const bool lt = m < min1;
                    min2 = lt ? min1 : fminf(min2, m);
                    min1 = lt ? m : min1;
                    arg = lt ? s : arg;
                };
                static_for<0, MAXR>([&](auto SS) __attribute__((always_inline)) {
                    constexpr int s = decltype(SS)::value;
                    if (s < R) {
                        t[s] = raw[s] - ira_c2v(st, s);
                        take(t[s], s);
                    }
                });
                const float vp0 = ap0 - ira_c2v(st, kIPS);
                const float vp1 = ap1 - ira_c2v(st, kIPS + 1);
                take(vp0, kIPS);
                if (has_prev) take(vp1, kIPS + 1);
                uint32_t meta = (uint32_t)arg << 27;
                static_for<0, MAXR>([&](auto SS) __attribute__((always_inline)) {
                    constexpr int s = decltype(SS)::value;
                    if (s < R) meta |= ((sgn ^ f2u(t[s])) >> 31) << s;
                });
                meta |= ((sgn ^ f2u(vp0)) >> 31) << kIPS;
                if (has_prev) meta |= ((sgn ^ f2u(vp1)) >> 31) << (kIPS + 1);
                const IraState nst{lay_mag<NORM>(min1, a.alpha, a.beta, a.clamp),
                                   lay_mag<NORM>(min2, a.alpha, a.beta, a.clamp), meta};
                if (live) ira_st_i(S, ra * kIZ + pos, nst);
                // parities: the own one goes on to layer ra + 1 in a register, the predecessor's is final for this sweep
                const float np0 = vp0 + ira_c2v(nst, kIPS);
                const float np1 = vp1 + ira_c2v(nst, kIPS + 1);
                if (ra == 0) {
                    if (live && pos > 0) Hn[pos - 1] = np1;
                } else if (live) {
                    P[(ra - 1) * kIZ + pos] = np1;
                }
                if (last) {
                    if (live) Hn[pos] = np0;
                } else {
                    carry = np0;
                }
                // information variables: one edge in the layer -> t + new; the first slot of a pair publishes new - old
                static_for<0, MAXR>([&](auto SS) __attribute__((always_inline)) {
                    constexpr int s = decltype(SS)::value;
                    if (s < R) {
                        const int kind = (ent[s] >> 17) & 3;
                        const float nw = ira_c2v(nst, s);
                        if (kind == 0) {
                            if (live) A[idx[s]] = t[s] + nw;
                        } else if (kind == 1) {
                            if (live) D[(ent[s] >> 19) * kIZ + (idx[s] - (ent[s] & 0xff) * kIZ)] = nw - ira_c2v(st, s);
                        }
                    }
                });
                if (lay >> 8) {  // (uniform) the row has a pair: its second slot adds both differences to the snapshot
                    __syncthreads();
                    static_for<0, MAXR>([&](auto SS) __attribute__((always_inline)) {
                        constexpr int s = decltype(SS)::value;
                        if (s < R && ((ent[s] >> 17) & 3) == 2) {
                            const float d1 = D[(ent[s] >> 19) * kIZ + (idx[s] - (ent[s] & 0xff) * kIZ)];
                            const float d2 = ira_c2v(nst, s) - ira_c2v(st, s);
                            if (live) A[idx[s]] = raw[s] + (d1 + d2);
                        }
                    });
                }
                __syncthreads();
            }
            if constexpr (ES) {
                // the syndrome of the posteriors the sweep left: the same gathers, a decision xor per check
                bool unsat = false;
                float prevp = 0.0f;
#pragma unroll 4
                for (int ra = 0; ra < q; ++ra) {
                    const float ownp = P[min(ra, q - 2) * kIZ + p];
                    const float own = ra == q - 1 ? Hn[p] : ownp;
                    const float prv = ra == 0 ? Hn[max(p - 1, 0)] : prevp;
                    bool par = Num<float>::bit(0.5f * own);
                    if (ra > 0 || p > 0) par ^= Num<float>::bit(0.5f * prv);
                    const int R = a.clay[ra] & 0xff;
                    cint32* row = a.cnl + ra * kICS;
                    static_for<0, MAXR>([&](auto SS) __attribute__((always_inline)) {
                        constexpr int s = decltype(SS)::value;
                        if (s < R) par ^= Num<float>::bit(0.5f * A[slot_idx(row[s])]);
                    });
                    unsat |= par && live;
                    prevp = own;
                }
                if (!__syncthreads_or(unsat)) {
                    used = it + 1;
                    break;
                }
            }
        }

        // z = 0.5 APP to the natural layout: bits (np.round(p1) rule) and soft (p1 = 1 - sigmoid(z), or z)
        if (live) P[(q - 1) * kIZ + pos] = Hn[pos];
        __syncthreads();
        auto put = [&](int64_t i, float z) __attribute__((always_inline)) {
            if (a.bits) a.bits[i] = (uint8_t)Num<float>::bit(z);
            if (a.soft) a.soft[i] = a.soft_z ? z : 1.0f - 1.0f / (1.0f + Num<float>::exp_(-z));
        };
        const int64_t base = cw * a.n;
        for (int v = pos; v < k; v += kIraLanes) put(base + v, 0.5f * A[v]);
        for (int j = pos; j < M; j += kIraLanes) put(base + k + j, 0.5f * P[(j % q) * kIZ + j / q]);
        if (pos == 0 && a.used) a.used[cw] = used;
        __syncthreads();  // the next codeword's load overwrites A and P
    }
}

// ---- host ------------------------------------------------------------------------------------------------

static size_t lay_lds_bytes(const IRASpec* s) {
    return ((size_t)s->k + kIZ + (size_t)std::max(s->lay_pairs, 0) * kIZ) * sizeof(float);
}

const char* ira_lay_why(const IRASpec* s) {
    static thread_local char buf[256];
    if (s->lay_pairs < 0) return "an IRA graph in which an information group meets one row of checks three or more times";
    if (s->q < 2) return "an IRA graph with q = 1: the two staircase edges of a layer's checks collide";
    if (lay_lds_bytes(s) + kLayLdsSlack > kLayLds) {
        snprintf(buf, sizeof buf, "an IRA code with k = %d: the layered kernel keeps the information posteriors in LDS, "
                 "and %zu bytes do not fit the %zu bytes of a gfx950 workgroup", s->k, lay_lds_bytes(s) + kLayLdsSlack, kLayLds);
        return buf;
    }
    return nullptr;
}

bool ira_lay_supports(const IRASpec* s, const ldpc_params& p) {
    if (!s || p.algo != LDPC_ALGO_MIN_SUM || (p.flags & LDPC_F_F64)) return false;
    return s->maxr <= kICS && ira_lay_why(s) == nullptr;
}

using LayKernel = void (*)(LayArgs);
template <int MAXR>
static LayKernel lay_pick_norm(int norm, bool es) {
#define LAY_K(N) (es ? (LayKernel)k_ira_lay<MAXR, N, true> : (LayKernel)k_ira_lay<MAXR, N, false>)
    switch (norm) {
        case LAY_PLAIN: return LAY_K(LAY_PLAIN);
        case LAY_ALPHA: return LAY_K(LAY_ALPHA);
        case LAY_BETA: return LAY_K(LAY_BETA);
        default: return LAY_K(LAY_BOTH);
    }
#undef LAY_K
}
// the row-slot bounds of the flooding check kernel
static LayKernel lay_pick(const IRASpec* s, const ldpc_params& p) {
    const int norm = (p.alpha != 1.0f ? LAY_ALPHA : 0) | (p.beta != 0.0f ? LAY_BETA : 0);
    const bool es = (p.flags & LDPC_F_EARLY_STOP) != 0;
    if (s->maxr <= 5) return lay_pick_norm<5>(norm, es);
    if (s->maxr <= 6) return lay_pick_norm<6>(norm, es);
    if (s->maxr <= 8) return lay_pick_norm<8>(norm, es);
    return lay_pick_norm<kICS>(norm, es);
}

// workgroups the device holds at once at this LDS size, capped by LDPC_IRA_LAY_SLOTS and the batch; raises the
// kernel's dynamic LDS limit on the way (above 64 KiB it must be asked for).  0 with the error set on failure.
static int64_t lay_slots(const IRASpec* s, LayKernel fn, int64_t B) {
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != s->device) (void)hipSetDevice(s->device);
    int per_cu = 0, cus = 0;
    hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lay_lds_bytes(s));
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)fn, kIraLanes, lay_lds_bytes(s));
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device);
    if (prev >= 0 && prev != s->device) (void)hipSetDevice(prev);
    if (e != hipSuccess || per_cu < 1 || cus < 1) {
        set_error(LDPC_EHIP, "IRA layered kernel: %zu bytes of LDS per workgroup: %s (%d workgroups per CU)",
                  lay_lds_bytes(s), hipGetErrorString(e), per_cu);
        return 0;
    }
    int64_t slots = (int64_t)cus * per_cu;
    const char* env = getenv("LDPC_IRA_LAY_SLOTS");
    if (env && atol(env) > 0) slots = std::min<int64_t>(slots, atol(env));
    return std::max<int64_t>(1, std::min(slots, B));
}

static size_t lay_a256(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t lay_slot_bytes(const IRASpec* s) {
    return lay_a256((size_t)s->M * sizeof(IraState)) + lay_a256((size_t)s->M * sizeof(float));
}

size_t ira_lay_workspace(const IRASpec* s, int64_t B, const ldpc_params& p) {
    return (size_t)lay_slots(s, lay_pick(s, p), B) * lay_slot_bytes(s);
}

int ira_lay_decode(const IRASpec* s, const float* llr, int64_t B, const ldpc_params& p, uint8_t* bits, float* soft,
                   int32_t* iters_used, char* ws, hipStream_t st) {
    const LayKernel fn = lay_pick(s, p);
    const int64_t slots = lay_slots(s, fn, B);
    if (slots < 1) return LDPC_EHIP;
    LayArgs a{};
    a.cnl = (cint32*)s->cnl;
    a.clay = (cint32*)s->clay;
    a.q = s->q; a.k = s->k; a.n = s->n; a.M = s->M;
    a.llr = llr;
    a.B = B;
    a.iters = p.iters;
    a.clamp = p.clamp; a.alpha = p.alpha; a.beta = p.beta;
    a.ws = ws;
    a.ws_slot = lay_slot_bytes(s);
    a.ws_par = lay_a256((size_t)s->M * sizeof(IraState));
    a.bits = bits;
    a.soft = soft;
    a.used = iters_used;
    a.soft_z = (p.flags & LDPC_F_SOFT_Z) ? 1 : 0;
    fn<<<(unsigned)slots, kIraLanes, lay_lds_bytes(s), st>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "IRA layered kernel launch: %s", hipGetErrorString(e));
    return LDPC_OK;
}

}  // namespace ldpc
