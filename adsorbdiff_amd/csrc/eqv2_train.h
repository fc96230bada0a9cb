#pragma once
#include "../../include/adsorbdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* EquiformerV2 training operators (csrc/eqv2_train.hip, adsorbdiff_amd/eqv2_train_step.py): the exported C
 * entries of the training step, declared here, next to their translation unit.  adsorbdiff_amd/lib.py binds them from this
 * text with the parser it uses for include/adsorbdiff_hip.h, whose types (adf_eqv2_t, adf_batch, status codes) they use.
 *
 * The edge side of a training step of the EquiformerV2 denoiser, forward and backward, as stateless entries on caller-owned
 * DEVICE float32 buffers; the handle is read for its dimensions and constant tables only (never for weights or workspaces,
 * except adf_op_eq_edge_scalars, which reads the bound atom_radii).  Exact f32 arithmetic.  No float atomics: every sum over
 * edges or rows runs in one fixed order, so two calls on the same input give the same bits.  ld* are row strides in floats.
 *
 * Layouts.  Node features [N, S, C], S = (lmax+1)^2, degree-major.  Edges sorted by target: eptr [N+1].  wig [E, DR]: the
 * kept Wigner rows of an edge as the forward forms them (degree l at its offset, row-major [2 min(l,mmax)+1][2l+1]).  A
 * tensor in an edge's own frame is [E, S_r, W] with the S_r coefficients |m| <= mmax ORDER-MAJOR: m = 0 for l = 0..lmax,
 * then per m the +m entries (l = m..lmax) followed by the -m entries (so2_ops.py / so3.py:83-103). */

/* The graph of a batch built with the handle's own kernels (adf_eqv2_forward's: top-K radius graph, or the list of
 * adf_eqv2_set_edges while one is in force), handed out: eptr [N+1], src / dst [E] int32, vec [E,3] (target -> source
 * image), wig [E, DR].  cap_edges: rows the edge arrays hold; *num_edges (host) receives E; E > cap_edges: ADF_EOVERFLOW and
 * nothing is copied.  Synchronises the stream once (E is read back).  Flags: adf_eqv2_check_flags. */
int32_t adf_eqv2_export_graph(adf_eqv2_t h, const adf_batch* b, int64_t cap_edges, int32_t* eptr, int32_t* src, int32_t* dst,
                              float* vec, float* wig, int64_t* num_edges, void* stream);

/* C (+)= A W^T + bias for any M, N, K: A [M,K] (lda), W [N,K] (ldw: a column block of a wider weight is a view), C [M,N]
 * (ldc); bias may be NULL; acc_C: add into C.  Every element is one f32 sum over k = 0..K-1 in index order. */
int32_t adf_op_eq_linear_fwd(const float* A, int32_t lda, const float* W, int32_t ldw, const float* bias, float* C,
                             int32_t ldc, int32_t acc_C, int64_t M, int32_t N, int32_t K, void* stream);
/* Its backward from dC [M,N]: dA [M,K] (optional) = dC W, written or (acc_dA) added; dW [N,K] (lddw; optional, needs A) and
 * db [N] (optional) are ADDED into.  dW and db are sums over the M rows in index order inside one workgroup. */
int32_t adf_op_eq_linear_bwd(const float* A, int32_t lda, const float* W, int32_t ldw, const float* dC, int32_t ldc, float* dA,
                             int32_t ldda, int32_t acc_dA, float* dW, int32_t lddw, float* db, int64_t M, int32_t N, int32_t K,
                             void* stream);
/* y = x sigmoid(x) on n elements, and dx = dy silu'(x). */
int32_t adf_op_eq_silu_fwd(const float* x, float* y, int64_t n, void* stream);
int32_t adf_op_eq_silu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);

/* Input rows of a radial MLP: out [E, NB + 2 EC] = [Gaussian basis of |vec| - r[Z_src] - r[Z_dst] | semb[Z_src] |
 * temb[Z_dst]] (NB = num_distance_basis, EC = edge_channels; semb / temb [max_num_elements, EC]; Z [N] int32). */
int32_t adf_op_eq_edge_scalars(adf_eqv2_t h, const int32_t* Z, const int32_t* src, const int32_t* dst, const float* vec,
                               const float* semb, const float* temb, int64_t E, float* out, void* stream);

/* Rotate-in: out [E, S_r, 2C] = radial * (D[rows |m| <= mmax] [x[src] | x[dst]]), order-major; radial [E, RW 2C], RW =
 * sum_m (lmax - m + 1): the weight of order m, degree l, channel c at ((offset of m) + l - m) 2C + c, shared by +m and -m. */
int32_t adf_op_eq_rotate_in_fwd(adf_eqv2_t h, const float* x, const int32_t* src, const int32_t* dst, const float* wig,
                                const float* radial, int64_t E, float* out, void* stream);
/* Its backward: dradial [E, RW 2C] and dx [N, S, C] are written.  dx[n] sums first n's incoming edges in list order (the
 * target half of the channels), then its outgoing edges in the order of sperm (the source half): sptr [N+1] / sperm [E] =
 * the edge numbers sorted by source, ties in list order. */
int32_t adf_op_eq_rotate_in_bwd(adf_eqv2_t h, const float* x, const int32_t* eptr, const int32_t* src, const int32_t* dst,
                                const float* wig, const float* radial, const float* dout, const int32_t* sptr,
                                const int32_t* sperm, int32_t N, int64_t E, float* dradial, float* dx, void* stream);

/* Separable S2 activation on y [E, S_r, W]: out[:, l = 0] = silu(gate) (gate [E, W], row stride ldg), out[:, r > 0] =
 * from_red^T silu(to_red y) on the handle's reduced grid.  The backward recomputes the grid values: dy [E, S_r, W] and dgate
 * (row stride lddg) are written. */
int32_t adf_op_eq_s2act_fwd(adf_eqv2_t h, const float* y, const float* gate, int32_t ldg, int32_t W, int64_t E, float* out,
                            void* stream);
int32_t adf_op_eq_s2act_bwd(adf_eqv2_t h, const float* y, const float* gate, int32_t ldg, const float* dout, int32_t W,
                            int64_t E, float* dy, float* dgate, int32_t lddg, void* stream);

/* Attention weights from a_in [E, NH A] (row stride lda): LayerNorm over the A channels of a head (ln_w, ln_b [A]), smooth
 * leaky ReLU, dot with alpha_dot [NH, A], softmax over a target's edges (denominator + 1e-16) -> soft [E, NH]; alpha [E, NH]
 * = soft * mask (mask [E, NH]: 0 or 1 / keep; NULL: no dropout, alpha = soft). */
int32_t adf_op_eq_alpha_fwd(adf_eqv2_t h, const float* a_in, int32_t lda, const float* ln_w, const float* ln_b,
                            const float* alpha_dot, const int32_t* eptr, const float* mask, int32_t N, int64_t E, float* soft,
                            float* alpha, void* stream);
/* Its backward from dalpha [E, NH]: da_in (row stride ldda) is written; d_ln_w, d_ln_b [A] and d_alpha_dot [NH, A] are ADDED
 * into: per chunk of 256 edges one partial row (edges in list order), then the chunks in index order.  scratch: at least
 * 3 E NH + (3 ceil(E / 256) + 2) NH A floats; scratch_floats says what it holds (less: ADF_EINVAL).  d_ln_w, d_ln_b and
 * d_alpha_dot may be NULL together: the parameter pass is then not run (the geometric gradient, csrc/eqv2_geo.h). */
int32_t adf_op_eq_alpha_bwd(adf_eqv2_t h, const float* a_in, int32_t lda, const float* ln_w, const float* ln_b,
                            const float* alpha_dot, const int32_t* eptr, const float* mask, const float* soft,
                            const float* dalpha, int32_t N, int64_t E, float* da_in, int32_t ldda, float* d_ln_w,
                            float* d_ln_b, float* d_alpha_dot, float* scratch, int64_t scratch_floats, void* stream);

/* Rotate-out and aggregation: agg [N, S, NH V] = sum over a target's edges, in list order, of D^T[:, rows |m| <= mmax]
 * (truncation rescale * alpha[e, head] * z[e]); z [E, S_r, NH V], alpha [E, NH].  only_l >= 0: that degree alone is formed
 * (the force blocks read l = 1), the other rows of agg are zero; -1: all.  The edge-degree embedding is this entry with
 * NH = 1 and alpha = 1. */
int32_t adf_op_eq_rotate_out_fwd(adf_eqv2_t h, const float* z, const float* alpha, int32_t NH, int32_t V, const int32_t* eptr,
                                 const float* wig, int32_t only_l, int32_t N, float* agg, void* stream);
/* Its backward from dagg [N, S, NH V]: dz [E, S_r, NH V] and dalpha [E, NH] (a head's V channels and the coefficients in
 * index order) are written. */
int32_t adf_op_eq_rotate_out_bwd(adf_eqv2_t h, const float* z, const float* alpha, int32_t NH, int32_t V, const int32_t* dst,
                                 const float* wig, const float* dagg, int32_t only_l, int64_t E, float* dz, float* dalpha,
                                 void* stream);

#ifdef __cplusplus
}
#endif
