/*
 * ldpc_abi.h — C ABI of the MI355X-native LDPC belief-propagation decoder (libldpc_hip.so).
 *
 * Plain C: pointers, sizes and ints only; no torch / HIP types in any signature (hip streams are passed
 * as void*).  Every entry point returns 0 (LDPC_OK) or a negative LDPC_E* code and leaves a message in
 * ldpc_last_error() (thread-local).  The reference (realjwin/ldpc-sims) has no C surface at all: its
 * decode boundary is Python.  Each function below names the reference interface it replaces.
 */
#ifndef LDPC_ABI_H
#define LDPC_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI revision of this header.  2: ldpc_decode gained iters_used (before the stream argument) in round 5 —
 * a caller built against revision 1 would pass its stream where iters_used is read.  Loaders compare
 * ldpc_abi_version() with the revision they were written for and refuse a mismatch (ldpc_amd/_abi.py does). */
#define LDPC_ABI_VERSION 2

typedef struct ldpc_graph ldpc_graph;

enum {
    LDPC_OK = 0,
    LDPC_EINVAL = -1,      /* bad argument (shape, range, null pointer)                */
    LDPC_EHIP = -2,        /* HIP runtime error (message names the call)                */
    LDPC_ENOMEM = -3,      /* device allocation failed / workspace too small            */
    LDPC_EUNSUPPORTED = -4 /* combination of algo/flags not implemented for this graph  */
};

enum {
    LDPC_ALGO_TANH_SP = 0, /* the reference's algorithm: bp/bp.py, bp_vc.py, bp_cv.py     */
    LDPC_ALGO_MIN_SUM = 1, /* normalized/offset min-sum (new; see oracle/ldpc_oracle.c) */
    LDPC_ALGO_QMIN_SUM = 2 /* integer (quantized-LLR) offset min-sum (new)              */
};

enum {
    LDPC_F_EARLY_STOP = 1,    /* stop a codeword once its syndrome is zero                   */
    LDPC_F_DEVICE_PTRS = 2,   /* llr/bits/soft/iters_used are device pointers (else host)     */
    LDPC_F_F64 = 4,           /* tanh-SP in float64: llr/soft are double* (reference .double()) */
    LDPC_F_SOFT_Z = 8,        /* soft_out = z = 0.5*(L + sum c2v) (half posterior LLR, P0/P1)  */
    LDPC_F_FORCE_GENERIC = 16,/* never use a structure-specialised (QC) kernel                 */
    LDPC_F_LAYERED = 32       /* layered (row-serial) schedule instead of flooding, see below  */
};

/* LDPC_F_LAYERED — layered min-sum, fp32, per codeword (conventions of the flooding min-sum: L = -llr, the
 * magnitude rule, the decision rule):
 *
 *   APP_v = L_v + (+0.0f) for every v;  c2v[e] = +0.0f for every edge
 *   for it in 0 .. iters-1:
 *     for check c in ascending order:                                        (row-serial)
 *       for each edge e of c (ascending column):  t_e = APP_v(e) - c2v[e]     (one fp32 subtract)
 *       min1 <= min2 = the two smallest |t_e|, idx = an edge attaining min1, sgn = xor of the sign bits of t_e
 *       c2v[e] = (sgn ^ signbit(t_e)) ? -mag : mag,
 *           mag = min(clamp, max(alpha*m - beta, 0)),  m = (e == idx) ? min2 : min1
 *       APP_v(e) = t_e + c2v[e]                                               (one fp32 add)
 *     LDPC_F_EARLY_STOP: after the full sweep, stop the codeword when H * (APP <= 2*ZTHR) = 0
 *   z_v = 0.5f * APP_v;  bit_v = z_v <= ZTHR;  iters_used = sweeps run
 *
 * Every value is one correctly rounded fp32 operation on defined operands (no contraction, no reordered sum),
 * so the result is defined bit for bit; ties in idx cannot change a value (then min2 == min1).  ZTHR is the
 * hard-decision threshold of every fp32 decoder here (-1.7881392e-07f).  Implemented for the compiled 802.11n
 * codes with Z <= 64, LDPC_ALGO_MIN_SUM, fp32, through ldpc_decode_ex / ldpc_decode (host or device
 * pointers).
 *
 * The same text, unchanged, on any other quasi-cyclic graph: when ldpc_graph_create finds that H is the lifting of a
 * base matrix with one circulant per block (lifting sizes: the divisors of gcd(m, n) in [4, 1024], largest first) and
 * no compiled table or IRA structure matched, a table-driven kernel reads shifts, columns and row degrees from a device
 * table (kernel path "qct-z<Z>-layered").  LDPC_ALGO_MIN_SUM, fp32, base row degrees 2..27, and a codeword's
 * 4 (n + Z) + 12 m bytes must fit the 160 KiB of LDS of a workgroup; otherwise LDPC_EUNSUPPORTED, naming the reason.
 * No workspace.  Flooding, tanh-SP, quantized min-sum and fp64 on such graphs run on the generic kernels as before.
 * Known gap: a graph that matches a compiled table is never offered to this kernel, so layered min-sum on the
 * compiled (1944,5/6) code (Z = 81) still returns LDPC_EUNSUPPORTED.
 *
 * LDPC_F_LAYERED on an IRA (DVB-S2-structured) graph — the same conventions, but a layer is one ROW of checks: with
 * m = 360 q checks, check c = a + q b is (row a, position b), and the 360 checks of a row are parallel:
 *
 *   APP_v = L_v + (+0.0f), L = -llr;  c2v[e] = +0.0f
 *   for it in 0 .. iters-1:
 *     for a in 0 .. q-1:                                        (layer = checks {c : c mod q == a})
 *       every check c of the layer, from the posteriors as they stood BEFORE the layer:
 *         t_e = APP_v(e) - c2v[e];  min1, min2, sgn over the check's t_e;  new_e exactly as the text above
 *       every variable v with ONE edge e in the layer:   APP_v = t_e + new_e
 *       every variable v with TWO edges e1, e2 there:    APP_v = APP_v + ((new_e1 - c2v[e1]) + (new_e2 - c2v[e2]))
 *       c2v[e] = new_e
 *     LDPC_F_EARLY_STOP: after the full sweep, stop the codeword when H * (APP <= 2*ZTHR) = 0
 *   z_v = 0.5f * APP_v;  bit_v = z_v <= ZTHR;  iters_used = sweeps run
 *
 * Every value is one correctly rounded fp32 operation; the two-edge sum is commutative, and the minima and the sign
 * do not depend on the order of a check's edges.  The staircase edges of a layer never share a variable (q >= 2); an
 * information variable has two edges in a layer when its group of 360 meets that row twice (8 of the 90 rows of
 * DVB-S2 rate 1/2).  Implemented for LDPC_ALGO_MIN_SUM, fp32, on any graph with the IRA structure whose n - m
 * information posteriors fit the 160 KiB of LDS of a workgroup and in which no group meets a row three or more
 * times; otherwise LDPC_EUNSUPPORTED, naming the reason.  Needs a kernel workspace (ldpc_workspace_size): 16 m
 * bytes per resident workgroup, not per codeword.
 *
 * LDPC_F_LAYERED with LDPC_ALGO_QMIN_SUM — layered quantized min-sum, integers throughout, per codeword (the
 * quantizer, sign convention and decision rule of the flooding LDPC_ALGO_QMIN_SUM):
 *
 *   q_v = sat(rint(llr_v * (1.0f / qstep)), qmax) in fp32;  L_v = -q_v
 *   APP_v = L_v;  c2v[e] = 0 for every edge
 *   for it in 0 .. iters-1:
 *     for check c in ascending order:                                        (row-serial)
 *       for each edge e of c:  t_e = APP_v(e) - c2v[e]                        (exact, |t_e| <= app_max + qmax)
 *                              a_e = max(min(|t_e|, qmax) - beta, 0)          (magnitudes capped at qmax)
 *       min1 <= min2 = the two smallest a_e, idx = an edge attaining min1, sgn = xor over e of (t_e < 0)
 *       c2v[e] = (sgn ^ (t_e < 0)) ? -m : m,   m = (e == idx) ? min2 : min1
 *       APP_v(e) = sat(t_e + c2v[e], app_max)
 *     LDPC_F_EARLY_STOP: after the full sweep, stop the codeword when H * (APP < 0) = 0
 *   z_v = 0.5f * APP_v;  bit_v = (APP_v < 0);  iters_used = sweeps run
 *
 * t_e is not saturated to qmax (that would cap every posterior at 2 qmax): only the magnitude entering the minima
 * is.  Zero has no sign: a zero t_e makes every other output of its check zero and its own output does not depend
 * on its own sign, so an implementation may carry -0 and z is defined by value, not by bit pattern.  Ties in idx
 * cannot change a value.  Implemented for the compiled codes with 32 < Z <= 64 ((1296,2/3)) in packed fp16, exact
 * while app_max + 2*qmax <= 2047; a larger bound, or another lifting size, returns LDPC_EUNSUPPORTED.
 *
 * LDPC_F_LAYERED with LDPC_ALGO_TANH_SP — layered tanh sum-product, fp32, per codeword (conventions of the flooding
 * tanh-SP: L = -llr, the decision rule, the message cap = min(clamp, log 16777215), the fp32 module's p clamp):
 *
 *   APP_v = L_v for every v;  c2v[e] = 0 for every edge
 *   for sweep in 0 .. iters-1:
 *     for check c in ascending order:                                        (row-serial)
 *       s_e    = APP_v(e) - c2v[e]                                  for each edge e of c
 *       c2v[e] = sign * min(cap, log((1+|p|)/(1-|p|))),  p = prod_{e' != e} tanh(s_e'/2),
 *                sign = xor of the sign bits of the other s_e'
 *       APP_v(e) = s_e + c2v[e]
 *     LDPC_F_EARLY_STOP: after the full sweep, stop the codeword when H * (z <= ZTHR) = 0; a stopped codeword is frozen
 *   z_v = APP_v / 2;  bit_v = z_v <= ZTHR;  iters_used = sweeps run
 *
 * Defined by value, not bit for bit: the check rule is evaluated in the (D, S) form in log2 units, as every fp32
 * tanh-SP kernel here, and held to 1e-5 * max(1, |z|) against the text above in float64
 * (tests/test_gpu_layered_sp.py).  The plain form only: the reference has no layered schedule, so there is no
 * golden whose exact zeros must be reproduced, and a codeword with exact-zero LLRs is decoded like any other — its
 * messages may sit within 2^-23 (log2 units) of 0 where the ideal value is 0.  Implemented for the compiled
 * 802.11n (1944,5/6) code (Z = 81) only; every other code returns LDPC_EUNSUPPORTED.
 *
 * Every other combination (tanh-SP on another code, LDPC_F_F64, LDPC_F_FORCE_GENERIC, a graph with neither quasi-cyclic nor
 * IRA structure, quantized min-sum on IRA graphs or on liftings without a compiled table, min-sum on the compiled Z = 81 code, ldpc_decode_weighted, ldpc_decode_x0,
 * ldpc_decode_bits_host) returns LDPC_EUNSUPPORTED and says which.  The flag is additive: ldpc_params and LDPC_ABI_VERSION are unchanged, and nothing changes while it is
 * clear.  The 802.11n forms need no kernel workspace. */

typedef struct {
    int32_t iters;   /* iterations (maximum when LDPC_F_EARLY_STOP)                         */
    int32_t algo;    /* LDPC_ALGO_*                                                          */
    int32_t flags;   /* LDPC_F_*                                                             */
    float clamp;     /* c2v clamp, the reference's clamp_value (bp/bp.py:47)                 */
    float alpha;     /* min-sum normalisation (1 = plain min-sum; QMIN_SUM requires 1)       */
    float beta;      /* min-sum offset (float algo) / integer offset >= 0 (QMIN_SUM; a
                        non-integer beta is LDPC_EINVAL there)                               */
    int32_t qmax;    /* QMIN_SUM: message/LLR saturation (15 = 5-bit signed)                 */
    int32_t app_max; /* QMIN_SUM: posterior saturation                                       */
    float qstep;     /* QMIN_SUM: LLR quantizer step; q = sat(rint(llr * (1.0f / qstep)), qmax)
                        in fp32 (reciprocal multiply, not division: the two can round
                        differently at .5 boundaries)                                         */
} ldpc_params;

/* Build a Tanner graph from H in CSR form (rows = checks, ascending columns).  Replaces
 * generate_masks(H) (pytorch/bp/masking.py:12-147) and BeliefPropagation.__init__ (bp/bp.py:20-39):
 * the graph is built once and reused, instead of dense E x E masks rebuilt per decode_bits call
 * (ofdm/ofdm_functions.py:143/145).  If H is the lifting of a base matrix for which a specialised
 * kernel is compiled in (802.11n codes), the handle carries it. */
int ldpc_graph_create(int32_t m, int32_t n, int32_t nnz, const int32_t* row_ptr, const int32_t* col_idx,
                      int32_t device, ldpc_graph** out);

/* Same, from a QC base matrix: shifts[mb*nb] row-major, -1 = null block, lifting size z. */
int ldpc_graph_create_qc(int32_t mb, int32_t nb, int32_t z, const int32_t* shifts, int32_t device,
                         ldpc_graph** out);

int ldpc_graph_destroy(ldpc_graph* g);

/* m, n, nnz (=E, the reference's layer_size(), bp/bp.py:61-62), and the QC lifting size of the
 * specialised kernel in use (0 = generic CSR kernels). */
int ldpc_graph_info(const ldpc_graph* g, int32_t* m, int32_t* n, int32_t* nnz, int32_t* qc_z);

/* The kernel family a decode with these params runs on this graph: "qc-z<Z>" (register-resident
 * quasi-cyclic kernels, 802.11n), "qc-z<Z>-layered" (the same codes with LDPC_F_LAYERED), "ira-z360" (DVB-S2-structured IRA codes, min-sum, fixed count or early
 * stop), "ira-z360-layered" (the same graphs with LDPC_F_LAYERED), "qct-z<Z>-layered" (LDPC_F_LAYERED min-sum on a
 * quasi-cyclic graph without a compiled table, Z the lifting size found) or
 * "generic-csr" (any H).  Introspection only (benchmarks label their records with it); NULL on bad
 * arguments.  The string is thread-local and valid until the next call on this thread.  No reference
 * counterpart: the reference has one code path (dense masks, bp/masking.py). */
const char* ldpc_kernel_path(const ldpc_graph* g, const ldpc_params* p);

/* Device bytes ldpc_decode_ex needs as caller-provided workspace for a batch of B codewords. */
int ldpc_workspace_size(const ldpc_graph* g, int64_t B, const ldpc_params* p, size_t* bytes);

/* Decode B codewords.  Replaces BeliefPropagation.forward(x=0, llr, clamp) -> p1 (bp/bp.py:43-51) and
 * the batch loop of decode_bits (ofdm/ofdm_functions.py:152-161).
 *   llr[B][n]     log P(bit=1)/P(bit=0), the reference's convention (ofdm_functions.py:72);
 *                 float* (double* with LDPC_F_F64).
 *   bits_out[B][n] 0/1 hard decisions, np.round(p1) semantics (ties -> 0).  May be NULL.
 *   soft_out[B][n] p1 = 1 - sigmoid(z) (or z with LDPC_F_SOFT_Z); float* (double* with F64).  May be NULL.
 *   iters_used[B] iterations run per codeword (== iters unless early stop).  May be NULL.
 *   workspace     device buffer of >= ldpc_workspace_size bytes, or NULL to use a per-graph internal
 *                 one (then the call is synchronous and serialised per graph).
 *   stream        hipStream_t as void* (NULL = default stream).  With LDPC_F_DEVICE_PTRS and a caller
 *                 workspace the call is asynchronous on the stream and graph-capturable; with host
 *                 pointers it copies in/out and returns after the stream synchronises. */
int ldpc_decode_ex(const ldpc_graph* g, const void* llr, int64_t B, const ldpc_params* p, uint8_t* bits_out,
                   void* soft_out, int32_t* iters_used, void* workspace, size_t workspace_bytes, void* stream);

/* Convenience form (float llr, internal workspace, alpha 1 / beta 0 / qmax 15 / app_max 127 / qstep 1) —
 * the signature SURVEY.md §8(b) sketches: iters_used[B] (may be NULL) as in ldpc_decode_ex.  Replaces the
 * same reference interface (bp/bp.py:43-51, ofdm/ofdm_functions.py:152-161); LDPC_F_F64 is ignored. */
int ldpc_decode(const ldpc_graph* g, const float* llr, int64_t B, int32_t iters, float clamp, int32_t algo,
                int32_t flags, uint8_t* bits_out, float* soft_out, int32_t* iters_used, void* stream);

/* Weighted BP — the reference module with trained (non-unit) VC weights: layers[i][0].input_weight
 * (E x E, masked by mask_v) and llr_weight (1 x n) per iteration, final_layer[0].input_weight (n x E) and
 * llr_weight (pytorch/bp/bp_vc.py:16-27, bp/bp.py:27-39).  Compact layout (element type = the decode
 * precision, DEVICE pointers, any may be NULL = all ones):
 *   vn      [iters][W]  vn[it*W + wofs[v] + t*d_v + u] = weight of var-slot u's c2v into var-slot t's v2c
 *                       (slot = position among v's edges in ascending check order; u == t unused);
 *                       W = sum_v d_v^2, wofs[v] = sum_{v' < v} d_v'^2
 *   llr     [iters][n]  per-variable LLR weight of each iteration
 *   fin     [E]         final layer: fin[var_ptr[v] + u] = weight of var-slot u into z_v
 *   fin_llr [n]
 * v2c = tanh(0.5 * (llr_w * L + sum_{u != t} w_tu * c2v_u)); z = 0.5 * (fin_llr * L + sum_u fin_u c2v_u).
 * tanh sum-product only, no early stop; always runs the generic CSR kernels (query the workspace with
 * LDPC_F_FORCE_GENERIC set). */
typedef struct ldpc_bp_weights {
    const void* vn;
    const void* llr;
    const void* fin;
    const void* fin_llr;
} ldpc_bp_weights;

int ldpc_weights_layout(const ldpc_graph* g, int64_t* vn_per_iter, int64_t* fin_len);
int ldpc_decode_weighted(const ldpc_graph* g, const void* llr, int64_t B, const ldpc_params* p,
                         const ldpc_bp_weights* w, uint8_t* bits_out, void* soft_out, int32_t* iters_used,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Training: the gradient of the weighted tanh-SP forward above (the reference's hand-written autograd Functions,
 * pytorch/bp/bp_vc.py:34-58 and bp_cv.py:57-96, on the GPU).  The differentiated function, in natural units:
 *
 *   L = -llr, x^0 = 0
 *   for it in 0 .. iters-1, variable v with edge slots t, u:
 *       s_t = 0.5 * (lw_it[v] * L_v + sum_{u != t} vn_it[t,u] * x_u),   tau_t = tanh(s_t)
 *     check c with edges e:
 *       p_e = prod_{e' != e} tau_e',  ph = clamp(p_e, +-(1 - 1e-7)),  x_e = clamp(log((1 + ph) / (1 - ph)), +-clamp)
 *   z_v = 0.5 * (fin_llr[v] * L_v + sum_u fin[var_ptr[v] + u] * x_u);  soft = z (LDPC_F_SOFT_Z) or 1 - sigmoid(z)
 *
 * Given G = d loss / d soft [B][n], ldpc_bp_backward returns the mathematical gradient of that function with
 * respect to vn [iters][W], the LLR weights [iters][n], fin [E], fin_llr [n] and llr [B][n].
 *   - A message whose magnitude was limited by either bound passes no gradient (torch.clamp's rule away from
 *     equality); the bound is min(clamp, log((1 + pmax) / (1 - pmax))), pmax = 1 - 1e-7, in fp64 and the merged
 *     log2-unit bound of the fp32 kernels (min(fp32(clamp * log2 e), 24)) in fp32.  The reference's own CV
 *     backward is straight-through at the p clamp and is NOT followed.
 *   - d p_e / d tau_u is formed from exclusive products, never by dividing by tau, so an exact-zero tau (an
 *     exact-zero LLR at iteration 0) needs no special case.
 *   - vn[0] (x^0 = 0) and the diagonal compact positions (u == t) have exactly zero gradient.
 *   - LDPC_F_EARLY_STOP, any algo but LDPC_ALGO_TANH_SP, and initial messages are LDPC_EUNSUPPORTED; iters >= 1.
 *   - fp32 and fp64 (LDPC_F_F64).  The result is bitwise reproducible: no floating-point atomics, the batch is
 *     reduced in a fixed order.
 *   - The vn gradient needs every variable degree <= 16 (one MFMA tile); a larger degree is LDPC_EUNSUPPORTED
 *     when out->vn is wanted, and the other gradients are still served.
 *
 * The tape holds L [n][ldb], every iteration's v2c [E][ldb] and c2v [E][ldb] as the generic kernels store them
 * (codeword-minor, ldb = B rounded up to 64; fp32: v2c = +-e^{-|2s|} and c2v in log2 units) and one zero-LLR flag
 * per codeword: elem * ldb * (n + 2 * E * iters) + ldb bytes.  ldpc_bp_forward_tape runs the kernels of
 * ldpc_decode_weighted on the tape's slices, so its soft_out is bitwise that function's.  All pointers are DEVICE
 * pointers (LDPC_F_DEVICE_PTRS is implied) and every call is asynchronous on stream; w may be NULL (all ones).
 * ldpc_bp_grads: NULL = not wanted; each wanted array is overwritten. */
typedef struct ldpc_bp_grads {
    void* vn;
    void* llr_w;
    void* fin;
    void* fin_llr;
    void* llr;
} ldpc_bp_grads;

int ldpc_bp_tape_size(const ldpc_graph* g, int64_t B, const ldpc_params* p, size_t* tape_bytes,
                      size_t* backward_ws_bytes);
int ldpc_bp_forward_tape(const ldpc_graph* g, const void* llr, int64_t B, const ldpc_params* p,
                         const ldpc_bp_weights* w, void* soft_out, void* tape, size_t tape_bytes, void* stream);
int ldpc_bp_backward(const ldpc_graph* g, int64_t B, const ldpc_params* p, const ldpc_bp_weights* w,
                     const void* tape, size_t tape_bytes, const void* grad_soft, const ldpc_bp_grads* out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* BeliefPropagation.forward(x, llr, clamp) with NON-ZERO initial messages x (pytorch/bp/bp.py:43-47: the
 * first layer consumes x exactly as later layers consume the previous c2v).  x0: DEVICE [B][E] in the
 * reference's check-order edge numbering (masking.py:84-88), element type = the decode precision; NULL =
 * zeros.  w: optional weights as ldpc_decode_weighted (NULL = plain BP).  Requires LDPC_F_DEVICE_PTRS when
 * x0 is given; tanh sum-product without early stop; generic CSR kernels (workspace as LDPC_F_FORCE_GENERIC). */
int ldpc_decode_x0(const ldpc_graph* g, const void* llr, int64_t B, const ldpc_params* p, const ldpc_bp_weights* w,
                   const void* x0, uint8_t* bits_out, void* soft_out, int32_t* iters_used, void* workspace,
                   size_t workspace_bytes, void* stream);

/* The drop-in decode_bits (pytorch/ofdm/ofdm_functions.py:131-163) end to end from HOST memory: rows
 * codewords of float64 llr[rows][n] (log P1/P0) -> out[rows][n] float64 0.0/1.0 (np.round(p1) semantics).
 * The caller passes rows = (N // batch_size) * batch_size and leaves the remainder rows zero, as the
 * reference does (:133-135); every batch is independent, so the batches are decoded in chunks of `chunk`
 * codewords (0 = ~16 MB of float32 LLRs) through a two-slot pinned staging ring: the host converts chunk
 * c+1 to float32 (the reference's torch.tensor(..., dtype=torch.float), :156) while the GPU copies in,
 * decodes and copies out chunk c on its own stream, and the host expands chunk c-1's uint8 bits to float64.
 * `threads` host threads for the staging copies (0 = min(16, hardware threads)).  p: float32 arithmetic on
 * host buffers (LDPC_F_F64 / LDPC_F_DEVICE_PTRS / LDPC_F_SOFT_Z are EINVAL); synchronous. */
int ldpc_decode_bits_host(const ldpc_graph* g, const double* llr, int64_t rows, const ldpc_params* p, double* out,
                          int64_t chunk, int32_t threads);

/* Error counting on device, the metrics of evaluate_quantized.py:139-141 for one SNR point:
 *   counts[0] += bit errors over the first info_bits positions of each codeword (coded BER numerator)
 *   counts[1] += codewords with any error over all n positions              (coded BLER numerator)
 *   counts[2] += B
 * bits, ref: device uint8 [B][n]; counts: device int64[3] (accumulated, not cleared). */
int ldpc_count_errors(const uint8_t* bits, const uint8_t* ref, int64_t B, int32_t n, int32_t info_bits,
                      int64_t* counts, void* stream);

/* BPSK/AWGN channel on device: llr[b][v] = -2 y / sigma^2 with y = (1 - 2 c[b][v]) + sigma * N(0,1),
 * N from a counter-based generator keyed by (seed, b0 + b, v).  codeword may be NULL (all-zero).
 * Distributionally equal to the reference's QPSK-OFDM path for rate-1/2 at SNR = Eb/N0
 * (ofdm_functions.py:17-35,63-78). */
int ldpc_awgn_llr(const uint8_t* codeword, float* llr, int64_t B, int32_t n, float sigma, uint64_t seed,
                  int64_t b0, void* stream);

/* Uniform random information bits on device: out[b][i] = bit of Philox(key = seed, counter = (b0+b)*k + i),
 * so the bits of global codeword b0+b do not depend on how a sweep is sharded.  out: device uint8 [B][k]. */
int ldpc_random_bits(uint8_t* out, int64_t B, int32_t k, uint64_t seed, int64_t b0, void* stream);

/* Systematic encoding on device: codeword[b] = [info[b] ; parity], H * codeword = 0.
 *   info      device uint8 [B][k], k = n - m; only bit 0 of each byte is used
 *   codeword  device uint8 [B][n], values 0/1; must not overlap info
 * Asynchronous on stream, graph-capturable, needs no workspace.  Implemented for graphs carrying a compiled
 * 802.11n QC code (Z = 27, 54, 81) and for IRA (staircase) graphs; any other graph: LDPC_EUNSUPPORTED.  The
 * parity part of H is invertible for these codes, so the parity bits are unique: the result is defined bit for
 * bit.  Additive: LDPC_ABI_VERSION is unchanged. */
int ldpc_encode(const ldpc_graph* g, const uint8_t* info, int64_t B, uint8_t* codeword, void* stream);

/* "qc-z<Z>-dualdiag", "ira-staircase", or "none" (thread-local string, as ldpc_kernel_path). */
const char* ldpc_encoder_path(const ldpc_graph* g);

/* OFDM transmitter, the reference's modulate_bits + transmit_symbols (ofdm/ofdm_functions.py:17-35):
 * bits[nsym * bits_per_symbol] (uint8, device) -> symbols (QPSK bits_per_symbol = 2, the reference's
 * mapping; 16-QAM = 4, Gray per dimension, new) -> blocks of ofdm_size -> unitary IDFT -> + complex AWGN
 * of per-dimension variance 1/(2 snr).  rx_out / tx_out: interleaved complex float [nsym][2] (tx_out may
 * be NULL).  Noise of stream sample sym0 + i is keyed by (seed, sym0 + i). nsym % ofdm_size == 0. */
int ldpc_ofdm_tx(const uint8_t* bits, int64_t nsym, int32_t ofdm_size, int32_t bits_per_symbol, float snr,
                 uint64_t seed, int64_t sym0, float* rx_out, float* tx_out, void* stream);

/* OFDM receiver, the reference's demodulate_signal (ofdm_functions.py:63-78): unitary DFT per block,
 * LLR = log P(1)/P(0) per bit with noise_power 0.5/snr (QPSK: the reference's closed form; 16-QAM:
 * exact log-sum-exp).  llr_out: float [nsym * bits_per_symbol]; sym_out (may be NULL): [nsym][2]. */
int ldpc_ofdm_demod(const float* rx, int64_t nsym, int32_t ofdm_size, int32_t bits_per_symbol, float snr,
                    float* llr_out, float* sym_out, void* stream);

/* ADC quantizer — replaces quantizer (pytorch/ofdm/ofdm_functions.py:37-51) and the AGC of gen_qdata
 * (:118-128).  rx / q_out: complex64 interleaved DEVICE buffers [nsym].  Exactly one of clip_ratio (AGC:
 * clip = std(rx) * clip_ratio computed on device over these nsym samples, as np.std of the complex
 * signal) or clip_value (fixed clip) must be > 0.  Arithmetic in fp64 as the reference:
 * step = 2 clip / (2^b - 1), q = clip(step * floor(x/step + .5), -(2^b/2) step + 1, (2^b/2) step - 1).
 * clip_out (optional, device double) receives the clip used in AGC mode.  Asynchronous on stream. */
int ldpc_adc_quantize(const float* rx, int64_t nsym, int32_t num_bits, double clip_ratio, double clip_value,
                      float* q_out, double* clip_out, void* stream);

const char* ldpc_last_error(void);
int ldpc_device_count(void);
const char* ldpc_version(void);
/* LDPC_ABI_VERSION of the header the library was built from (compare before binding any other symbol). */
int ldpc_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ABI_H */
