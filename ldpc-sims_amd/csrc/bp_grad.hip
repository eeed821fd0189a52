// bp_grad.hip — backward pass of the weighted tanh-SP decoder (ldpc_bp_backward, include/ldpc_abi.h): the
// gradient of soft = f(llr; vn, lw, fin, flw) with respect to all five, from the tape a differentiable forward
// left (common.h BPTape: L, every iteration's v2c and c2v as the generic kernels stored them, generic_impl.h).
//
// Dataflow, walking it = iters-1 .. 0 with two [E][ldb] gradient buffers gx (d loss / d c2v) and gs (d loss / d s,
// s the VC tanh argument), one [n][ldb] buffer gz (d loss / d z) and one [n][ldb] accumulator dl (d loss / d llr):
//
//   k_bp_final_bwd   G [B][n] -> gz, gx = 0.5 fin gz, dl = -0.5 flw gz          (transposed through an LDS tile)
//   k_bp_rank1       fin / fin_llr partials: sum_cw gz x_e, sum_cw gz L          (wave reduction per chunk)
//   per iteration:
//     k_bp_cn_bwd    gx -> gs        per (check, codeword): exclusive (P, Q) sets, O(d), no division
//     k_bp_wgrad     gs, c2v_{it-1}, L -> vn / lw partials: a d_v x d_v GEMM over the batch on MFMA tiles
//     k_bp_vn_bwd    gs -> gx of the previous iteration, dl += -0.5 lw sum_t gs
//   k_bp_wreduce     partials [chunk][N] -> 0.5 * sum in ascending chunk order    (after every partial pass)
//   k_bp_llr_out     dl [n][ldb] -> grad llr [B][n]
//
// Lanes map to codewords in every kernel but k_bp_wgrad (generic kernels' layout: a wave reads 256-byte row
// segments, graph lookups are wave-uniform scalar loads).  Every (node, codeword) element of gx / gs / gz / dl
// has one writer per kernel and the batch sums run chunk by chunk in a fixed order, so there is no atomic and
// the result is the same bits on every run.
//
// Units.  Gradients are in natural units throughout.  The fp32 tape holds v2c as signed a = +-e^{-|2s|} and c2v
// in log2 units (common.h); TapeNum<float> reads tau = sign (1 - a) / (1 + a), 1 - tau^2 = 4 a / (1 + a)^2
// (no cancellation near |tau| = 1) and x = c2v ln 2 from them.  The check node's own derivative comes from the
// taped output instead of a recomputed p: with b = e^{-|x|} = (1 - |p|) / (1 + |p|), dx/dp = 2 / (1 - p^2) =
// (1 + b)^2 / (2 b), and a message passes gradient iff its taped magnitude is below the bound the forward
// clamped it to — the forward's own decision, bit for bit, in both precisions.
#include "generic_impl.h"

namespace ldpc {

constexpr int kBpChunk = 512;                 // codewords per batch-reduction chunk (a multiple of 16)
constexpr float kLn2F32 = 0x1.62e430p-1f;     // fp32(ln 2)

template <typename T> struct TapeNum;
template <> struct TapeNum<float> {
    static constexpr float kXUnit = kLn2F32;  // natural x per taped c2v unit
    __device__ static float tau(float v) {
        const float a = fabsf(v);
        return __builtin_copysignf((1.0f - a) / (1.0f + a), v);
    }
    __device__ static float dtau(float v) {  // 1 - tau^2
        const float a = fabsf(v), r = 1.0f / (1.0f + a);
        return 4.0f * a * r * r;
    }
    __device__ static float eabs(float c) { return __builtin_amdgcn_exp2f(-fabsf(c)); }  // e^{-|x|}
    __device__ static float bound(float clamp, float) { return sp_cmax2(clamp); }
};
template <> struct TapeNum<double> {
    static constexpr double kXUnit = 1.0;
    __device__ static double tau(double v) { return v; }
    __device__ static double dtau(double v) { return 1.0 - v * v; }
    __device__ static double eabs(double c) { return exp(-fabs(c)); }
    // pmax arrives as a kernel argument so that the p bound is evaluated here by the operations cn_tanh_out
    // applies to a clamped p (a compile-time constant could be folded by another log)
    __device__ static double bound(double clamp, double pmax) { return fmin(clamp, log((1.0 + pmax) / (1.0 - pmax))); }
};

// one wave per node, one codeword per lane: 4 nodes per 256-thread workgroup
__device__ __forceinline__ bool node_slot(int nodes, int64_t B, int& node, int64_t& cw) {
    node = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * 4u + (threadIdx.x >> 6)));
    cw = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    return node < nodes && cw < B;
}

// G [B][n] -> gz [n][ldb] (d loss / d z), gx of the last iteration's c2v, dl = d loss / d llr through the final
// layer.  z is recomputed as k_final computes it.
template <typename T>
__global__ __launch_bounds__(256) void k_bp_final_bwd(const int32_t* __restrict__ var_ptr,
                                                      const int32_t* __restrict__ var_edges, const T* __restrict__ L,
                                                      const T* __restrict__ c2v, const T* __restrict__ G, int64_t B,
                                                      int64_t ldb, int n, int soft_z, const T* __restrict__ fin,
                                                      const T* __restrict__ flw, T* __restrict__ gz,
                                                      T* __restrict__ gx, T* __restrict__ dl) {
    __shared__ T gt[64][65];
    const int64_t cw0 = (int64_t)blockIdx.x * 64;
    const int v0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int cr = ty; cr < 64; cr += 4) {
        const int64_t cw = cw0 + cr;
        const int v = v0 + tx;
        if (v < n && cw < B) gt[cr][tx] = G[cw * n + v];
    }
    __syncthreads();
    for (int vr = ty; vr < 64; vr += 4) {
        const int v = v0 + vr;
        const int64_t cw = cw0 + tx;
        if (v < n && cw < B) {
            const int a = var_ptr[v];
            const int d = var_ptr[v + 1] - a;
            const T fl = flw ? flw[v] : T(1);
            T g = gt[tx][vr];
            if (!soft_z) {  // p1 = 1 - sigmoid(z): d p1 / d z = -sigmoid(z) (1 - sigmoid(z))
                T S = T(0);
                for (int k = 0; k < d; ++k)
                    S += (fin ? fin[a + k] : T(1)) * c2v[(int64_t)var_edges[a + k] * ldb + cw];
                const T z = sp_z<T>(fl * L[(int64_t)v * ldb + cw], S);
                const T sg = T(1) / (T(1) + Num<T>::exp_(-z));
                g = -g * sg * (T(1) - sg);
            }
            gz[(int64_t)v * ldb + cw] = g;
            dl[(int64_t)v * ldb + cw] = T(-0.5) * fl * g;
            for (int k = 0; k < d; ++k)
                gx[(int64_t)var_edges[a + k] * ldb + cw] = T(0.5) * (fin ? fin[a + k] : T(1)) * g;
        }
    }
}

// Check node.  With h_e = gate_e gx_e dx_e/dp_e, d loss / d tau_u = sum_{e != u} h_e prod_{w != e,u} tau_w.  A
// set of edges is the pair (P, Q) = (prod tau, sum_e h_e prod_{w != e} tau_w); one more edge u in front gives
// (tau_u P, h_u P + tau_u Q), and two disjoint sets join as (P1 P2, Q1 P2 + P1 Q2), so the sum over the others
// of edge u is the join of its prefix and suffix sets: O(d) products, no division, an exact-zero tau needs no
// special case.  Slots >= d carry (tau, h) = (1, 0), the identity.
template <typename T, int MAXD>
__global__ __launch_bounds__(256) void k_bp_cn_bwd(const int32_t* __restrict__ row_ptr, const T* __restrict__ v2c,
                                                   const T* __restrict__ c2v, const T* __restrict__ gx,
                                                   T* __restrict__ gs, int64_t B, int64_t ldb, T clamp, T pmax, int m) {
    int c;
    int64_t cw;
    if (!node_slot(m, B, c, cw)) return;
    const int a = row_ptr[c];
    const int d = row_ptr[c + 1] - a;
    if (d == 0) return;
    const T bound = TapeNum<T>::bound(clamp, pmax);
    T tau[MAXD], h[MAXD];
    static_for<0, MAXD>([&](auto kk) __attribute__((always_inline)) {
        constexpr int k = decltype(kk)::value;
        const int64_t o = (int64_t)(a + (k < d ? k : d - 1)) * ldb + cw;
        const T v = v2c[o], x = c2v[o], g = gx[o];
        const T b = TapeNum<T>::eabs(x);
        const bool open = (x < T(0) ? -x : x) < bound;
        tau[k] = k < d ? TapeNum<T>::tau(v) : T(1);
        h[k] = (k < d && open) ? g * ((T(1) + b) * (T(1) + b)) / (T(2) * b) : T(0);
    });
    T Ps[MAXD + 1], Qs[MAXD + 1];  // the set of slots u .. MAXD-1
    Ps[MAXD] = T(1);
    Qs[MAXD] = T(0);
    static_for<0, MAXD>([&](auto kk) __attribute__((always_inline)) {
        constexpr int u = MAXD - 1 - decltype(kk)::value;
        Ps[u] = tau[u] * Ps[u + 1];
        Qs[u] = h[u] * Ps[u + 1] + tau[u] * Qs[u + 1];
    });
    T Pp = T(1), Qp = T(0);  // the set of slots 0 .. u-1
    static_for<0, MAXD>([&](auto uu) __attribute__((always_inline)) {
        constexpr int u = decltype(uu)::value;
        if (u < d) {
            const int64_t o = (int64_t)(a + u) * ldb + cw;
            const T dt = Qp * Ps[u + 1] + Pp * Qs[u + 1];
            gs[o] = dt * TapeNum<T>::dtau(v2c[o]);
            Qp = h[u] * Pp + tau[u] * Qp;
            Pp = Pp * tau[u];
        }
    });
}

// Variable node of iteration it: gx_u = 0.5 sum_{t != u} vn_it[t,u] gs_t for the previous iteration's c2v (not at
// it = 0: x^0 = 0 is no variable), dl += -0.5 lw sum_t gs_t, and (sg != null) the plain sum_t gs_t per (variable,
// codeword), from which graphs with a degree above the MFMA tile get their LLR-weight gradient (k_bp_rank1).
template <typename T, int MAXD>
__global__ __launch_bounds__(256) void k_bp_vn_bwd(const int32_t* __restrict__ var_ptr,
                                                   const int32_t* __restrict__ var_edges,
                                                   const int32_t* __restrict__ wofs, const T* __restrict__ vn_it,
                                                   const T* __restrict__ lw_it, const T* __restrict__ gs,
                                                   T* __restrict__ gx, T* __restrict__ dl, T* __restrict__ sg,
                                                   int64_t B, int64_t ldb, int first, int n) {
    int v;
    int64_t cw;
    if (!node_slot(n, B, v, cw)) return;
    const int a = var_ptr[v];
    const int d = var_ptr[v + 1] - a;
    if (d == 0) {
        if (sg) sg[(int64_t)v * ldb + cw] = T(0);
        return;
    }
    const T* wv = vn_it ? vn_it + wofs[v] : nullptr;
    const T lw = lw_it ? lw_it[v] : T(1);
    T g[MAXD];
    int64_t off[MAXD];
    T sum = T(0);
    static_for<0, MAXD>([&](auto kk) __attribute__((always_inline)) {
        constexpr int k = decltype(kk)::value;
        off[k] = (int64_t)var_edges[a + (k < d ? k : d - 1)] * ldb + cw;
        const T x = gs[off[k]];
        g[k] = k < d ? x : T(0);
        sum += g[k];
    });
    dl[(int64_t)v * ldb + cw] += T(-0.5) * lw * sum;
    if (sg) sg[(int64_t)v * ldb + cw] = sum;
    if (first) return;
    static_for<0, MAXD>([&](auto uu) __attribute__((always_inline)) {
        constexpr int u = decltype(uu)::value;
        if (u < d) {
            T acc = T(0);
            static_for<0, MAXD>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value;
                if constexpr (t != u) {
                    if (t < d) acc += (wv ? wv[t * d + u] : T(1)) * g[t];
                }
            });
            gx[off[u]] = T(0.5) * acc;
        }
    });
}

// ---- weight gradients: a batched tiny GEMM over the batch --------------------------------------------------
// d loss / d vn_it[v] = 0.5 Gs Xt with Gs (d_v x B) the gs rows of v's edges and X (d_v x B) the previous c2v
// rows of the same edges: K = the batch.  One wave owns one variable and one chunk of kBpChunk codewords and
// accumulates the 16 x 16 tile D = A B with v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64: A[i][k] and B[k][j]
// both sit in lane (i or j = lane mod 16, k = lane div 16), so lane (i, q) loads four consecutive codewords
// c + 4 q + r of edge row i from gs and from x as one 16- / 32-byte access each and issues four MFMAs, component
// r of both operands as k = q.  Rows >= d_v and codewords >= the chunk's end are fed zeros.  The LLR weight's
// gradient sum_cw L_v sum_t gs_t rides along as B row d_v = L_v where d_v < 16 (column d_v of the tile, summed
// over its rows); at d_v = 16 it takes a second accumulator whose B rows are all L_v.
template <typename T> struct Mfma;
template <> struct Mfma<float> {
    using Acc = __attribute__((ext_vector_type(4))) float;
    __device__ static Acc mac(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    __device__ static int row(int q, int r) { return 4 * q + r; }  // D[4 q + r][lane mod 16] in register r
};
template <> struct Mfma<double> {
    using Acc = __attribute__((ext_vector_type(4))) double;
    __device__ static Acc mac(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    __device__ static int row(int q, int r) { return 4 * r + q; }  // D[4 r + q][lane mod 16] in register pair r
};

template <typename T>
__device__ __forceinline__ void load4(const T* p, bool on, int64_t c, int64_t c1, T (&o)[4]) {
    if (on) {
        using U = __attribute__((ext_vector_type(4))) T;
        const U u = *reinterpret_cast<const U*>(p + c);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (c + r < c1) ? u[r] : T(0);
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = T(0);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_bp_wgrad(const int32_t* __restrict__ var_ptr,
                                                  const int32_t* __restrict__ var_edges,
                                                  const int32_t* __restrict__ wofs, const T* __restrict__ gs,
                                                  const T* __restrict__ xprev, const T* __restrict__ L, int64_t B,
                                                  int64_t ldb, int n, int64_t W, T* __restrict__ part_vn,
                                                  T* __restrict__ part_lw) {
    const int v = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (v >= n) return;
    const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
    const int a = var_ptr[v];
    const int d = var_ptr[v + 1] - a;
    const int64_t ch = blockIdx.y;
    if (d == 0 || d > 16) {  // d > 16 is refused before the launch; an isolated variable has no messages
        if (part_lw && lane == 0) part_lw[ch * n + v] = T(0);
        return;
    }
    const int64_t c0 = ch * kBpChunk, c1 = (c0 + kBpChunk < B) ? c0 + kBpChunk : B;
    const int64_t row = (int64_t)var_edges[a + (i < d ? i : 0)] * ldb;
    const T* Lv = L + (int64_t)v * ldb;
    const bool a_on = i < d;
    const bool b_x = i < d && xprev != nullptr, b_l = i == d;  // i == d only where d < 16
    const T* pb = b_x ? xprev + row : Lv;                      // dereferenced only under b_x || b_l
    typename Mfma<T>::Acc acc = {0, 0, 0, 0}, acc2 = {0, 0, 0, 0};
    for (int64_t cb = c0; cb < c1; cb += 16) {  // wave-uniform: every MFMA runs with all lanes (cb + 16 <= ldb)
        const int64_t c = cb + 4 * q;
        T av[4], bv[4];
        load4<T>(gs + row, a_on, c, c1, av);
        load4<T>(pb, b_x || b_l, c, c1, bv);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = Mfma<T>::mac(av[r], bv[r], acc);
        if (d == 16) {
            T lv[4];
            load4<T>(Lv, true, c, c1, lv);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc2 = Mfma<T>::mac(av[r], lv[r], acc2);
        }
    }
    if (part_vn && i < d) {
        T* o = part_vn + ch * W + wofs[v];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = Mfma<T>::row(q, r);
            if (t < d) o[t * d + i] = (t == i) ? T(0) : acc[r];  // the diagonal is no weight: exactly zero
        }
    }
    // the LLR-weight column: rows >= d are zero (A fed zeros), so the column's sum is over t < d
    const int col = d < 16 ? d : 0;
    const typename Mfma<T>::Acc& lc = d < 16 ? acc : acc2;
    T s = (lc[0] + lc[1]) + (lc[2] + lc[3]);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (part_lw && lane == col) part_lw[ch * n + v] = s;
}

// Rank-1 gradients, one wave per (variable, chunk): part_a[ch][var_ptr[v] + u] = sum_cw gz_v x_u over the chunk
// (xs == null: skipped) and part_b[ch][v] = sum_cw gz_v L_v, by a butterfly over the lanes.
template <typename T>
__global__ __launch_bounds__(256) void k_bp_rank1(const int32_t* __restrict__ var_ptr,
                                                  const int32_t* __restrict__ var_edges, const T* __restrict__ gz,
                                                  const T* __restrict__ xs, const T* __restrict__ L, int64_t B,
                                                  int64_t ldb, int n, int64_t E, T* __restrict__ part_a,
                                                  T* __restrict__ part_b) {
    const int v = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (v >= n) return;
    const int lane = threadIdx.x & 63;
    const int a = var_ptr[v];
    const int d = (xs && part_a) ? var_ptr[v + 1] - a : 0;
    const int64_t ch = blockIdx.y;
    const int64_t c0 = ch * kBpChunk, c1 = (c0 + kBpChunk < B) ? c0 + kBpChunk : B;
    const T* g = gz + (int64_t)v * ldb;
    for (int u = -1; u < d; ++u) {  // u = -1: the L row
        if (u < 0 && !part_b) continue;
        const T* x = u < 0 ? L + (int64_t)v * ldb : xs + (int64_t)var_edges[a + u] * ldb;
        T s = T(0);
        for (int64_t c = c0 + lane; c < c1; c += 64) s += g[c] * x[c];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) {
            if (u < 0) part_b[ch * n + v] = s;
            else part_a[ch * E + a + u] = s;
        }
    }
}

// out[i] = scale * (part[0][i] + part[1][i] + ...), chunks in ascending order
template <typename T>
__global__ __launch_bounds__(256) void k_bp_wreduce(const T* __restrict__ part, int64_t N, int nch, T scale,
                                                    T* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    T s = part[i];
    for (int c = 1; c < nch; ++c) s += part[(int64_t)c * N + i];
    out[i] = scale * s;
}

// dl [n][ldb] -> grad llr [B][n]
template <typename T>
__global__ __launch_bounds__(256) void k_bp_llr_out(const T* __restrict__ dl, T* __restrict__ out, int64_t B, int n,
                                                    int64_t ldb) {
    __shared__ T tile[64][65];
    const int64_t cw0 = (int64_t)blockIdx.x * 64;
    const int v0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int vr = ty; vr < 64; vr += 4) {
        const int v = v0 + vr;
        const int64_t cw = cw0 + tx;
        if (v < n && cw < B) tile[vr][tx] = dl[(int64_t)v * ldb + cw];
    }
    __syncthreads();
    for (int cr = ty; cr < 64; cr += 4) {
        const int64_t cw = cw0 + cr;
        const int v = v0 + tx;
        if (v < n && cw < B) out[cw * n + v] = tile[tx][cr];
    }
}

// ------------------------------------------------------------------------------------------------------------
// Workspace: gx [E][ldb], gs [E][ldb], gz [n][ldb], dl [n][ldb], partials [chunks][max(W, E) + n]
struct BwdLayout {
    size_t gx, gs, gz, dl, part, total;
    int64_t ldb, stride;
    int nch;
};
static BwdLayout bwd_layout(const GenericArgs& g, int64_t B, size_t elem) {
    BwdLayout w{};
    w.ldb = (B + 63) / 64 * 64;
    w.nch = (int)((B + kBpChunk - 1) / kBpChunk);
    w.stride = g.W > g.E ? g.W : g.E;  // the vn / fin partials; the per-variable ones follow
    size_t off = 0;
    w.gx = off;
    off += a256(elem * (size_t)w.ldb * g.E);
    w.gs = off;
    off += a256(elem * (size_t)w.ldb * g.E);
    w.gz = off;
    off += a256(elem * (size_t)w.ldb * g.n);
    w.dl = off;
    off += a256(elem * (size_t)w.ldb * g.n);
    w.part = off;
    off += a256(elem * (size_t)w.nch * (size_t)(w.stride + g.n));
    w.total = off;
    return w;
}

size_t bp_backward_workspace(const GenericArgs& g, int64_t B, const ldpc_params& p) {
    return bwd_layout(g, B, (p.flags & LDPC_F_F64) ? 8 : 4).total;
}

#define BP_DEG_SWITCH(dd, CALL) \
    switch (dd) { case 4: CALL(4); break; case 8: CALL(8); break; case 12: CALL(12); break; case 16: CALL(16); break; \
                  case 20: CALL(20); break; case 24: CALL(24); break; default: CALL(32); }

template <typename T>
static int backward_t(const GenericArgs& g, int64_t B, const ldpc_params& p, const BPWeights& w, const char* tape,
                      const T* G, const ldpc_bp_grads& out, char* ws, hipStream_t st) {
    const int dv = pick_maxd(g.max_dv), dc = pick_maxd(g.max_dc);
    if (dv < 0 || dc < 0) return set_error(LDPC_EUNSUPPORTED, "node degree > 32 not supported by generic kernels");
    if (out.vn && g.max_dv > 16)
        return set_error(LDPC_EUNSUPPORTED, "the edge-weight (vn) gradient needs every variable degree <= 16 (one MFMA "
                                            "tile); this graph has a variable of degree %d", g.max_dv);
    const BPTape tl = bp_tape_layout(g.n, g.E, B, sizeof(T), p.iters);
    const BwdLayout bl = bwd_layout(g, B, sizeof(T));
    const int64_t ldb = bl.ldb;
    const T* L = (const T*)(tape + tl.L);
    T* gx = (T*)(ws + bl.gx);
    T* gs = (T*)(ws + bl.gs);
    T* gz = (T*)(ws + bl.gz);
    T* dl = (T*)(ws + bl.dl);
    T* part_a = (T*)(ws + bl.part);                 // [nch][W] or [nch][E]
    T* part_b = part_a + (int64_t)bl.nch * bl.stride;  // [nch][n]
    const T *w_vn = (const T*)w.vn, *w_lw = (const T*)w.lw, *w_fin = (const T*)w.fin, *w_flw = (const T*)w.flw;
    const dim3 tb(kTB);
    const unsigned gcw = (unsigned)((B + 63) / 64);
    const dim3 gtile(gcw, (unsigned)((g.n + 63) / 64));
    const dim3 gwave((unsigned)((g.n + 3) / 4), (unsigned)bl.nch);
    const T xs = T(0.5) * TapeNum<T>::kXUnit;  // 0.5 and the taped c2v's unit
    auto reduce = [&](const T* part, int64_t N, T scale, T* o) {
        k_bp_wreduce<T><<<(unsigned)((N + kTB - 1) / kTB), tb, 0, st>>>(part, N, bl.nch, scale, o);
    };
    const T* c2v_last = (const T*)(tape + tl.c2v(p.iters - 1));
    k_bp_final_bwd<T><<<gtile, tb, 0, st>>>(g.var_ptr, g.var_edges, L, c2v_last, G, B, ldb, g.n,
                                            (p.flags & LDPC_F_SOFT_Z) ? 1 : 0, w_fin, w_flw, gz, gx, dl);
    if (out.fin || out.fin_llr) {
        k_bp_rank1<T><<<gwave, tb, 0, st>>>(g.var_ptr, g.var_edges, gz, c2v_last, L, B, ldb, g.n, g.E,
                                            out.fin ? part_a : nullptr, out.fin_llr ? part_b : nullptr);
        if (out.fin) reduce(part_a, g.E, xs, (T*)out.fin);
        if (out.fin_llr) reduce(part_b, g.n, T(0.5), (T*)out.fin_llr);
    }
    const bool tile_ok = g.max_dv <= 16;  // else only the LLR-weight gradient is wanted here: through k_bp_rank1
    for (int it = p.iters - 1; it >= 0; --it) {
        const T* v2c = (const T*)(tape + tl.v2c(it));
        const T* c2v = (const T*)(tape + tl.c2v(it));
        const T* xprev = it ? (const T*)(tape + tl.c2v(it - 1)) : nullptr;
        const T* vn_it = w_vn ? w_vn + (int64_t)it * g.W : nullptr;
        const T* lw_it = w_lw ? w_lw + (int64_t)it * g.n : nullptr;
        T* o_vn = out.vn ? (T*)out.vn + (int64_t)it * g.W : nullptr;
        T* o_lw = out.llr_w ? (T*)out.llr_w + (int64_t)it * g.n : nullptr;
#define CNB(D) \
    k_bp_cn_bwd<T, D><<<dim3(gcw, (unsigned)((g.m + 3) / 4)), tb, 0, st>>>(g.row_ptr, v2c, c2v, gx, gs, B, ldb, \
                                                                          (T)p.clamp, (T)kPmaxF64, g.m)
        BP_DEG_SWITCH(dc, CNB)
#undef CNB
        if ((o_vn || o_lw) && tile_ok) {
            k_bp_wgrad<T><<<gwave, tb, 0, st>>>(g.var_ptr, g.var_edges, g.wofs, gs, xprev, L, B, ldb, g.n, g.W,
                                                o_vn ? part_a : nullptr, o_lw ? part_b : nullptr);
            if (o_vn) reduce(part_a, g.W, xs, o_vn);
            if (o_lw) reduce(part_b, g.n, T(0.5), o_lw);
        }
        T* sg = (o_lw && !tile_ok) ? gz : nullptr;  // gz is free once the final layer's gradients are out
        if (it == 0 && !out.llr && !sg) break;      // nothing below the first VC layer is wanted
#define VNB(D) \
    k_bp_vn_bwd<T, D><<<dim3(gcw, (unsigned)((g.n + 3) / 4)), tb, 0, st>>>(g.var_ptr, g.var_edges, g.wofs, vn_it, lw_it, \
                                                                          gs, gx, dl, sg, B, ldb, it == 0, g.n)
        BP_DEG_SWITCH(dv, VNB)
#undef VNB
        if (sg) {
            k_bp_rank1<T><<<gwave, tb, 0, st>>>(g.var_ptr, g.var_edges, sg, (const T*)nullptr, L, B, ldb, g.n, g.E,
                                                (T*)nullptr, part_b);
            reduce(part_b, g.n, T(0.5), o_lw);
        }
    }
    if (out.llr)
        k_bp_llr_out<T><<<gtile, tb, 0, st>>>(dl, (T*)out.llr, B, g.n, ldb);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "bp backward launch: %s", hipGetErrorString(e));
    return LDPC_OK;
}

int bp_backward(const GenericArgs& g, int64_t B, const ldpc_params& p, const BPWeights& w, const char* tape,
                const void* grad_soft, const ldpc_bp_grads& out, char* ws, hipStream_t st) {
    if (p.flags & LDPC_F_F64) return backward_t<double>(g, B, p, w, tape, (const double*)grad_soft, out, ws, st);
    return backward_t<float>(g, B, p, w, tape, (const float*)grad_soft, out, ws, st);
}

}  // namespace ldpc
