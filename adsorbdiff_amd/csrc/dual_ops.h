#pragma once
#include "../../include/adsorbdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Training on energy-gradient forces (csrc/dual_ops.hip, csrc/message_dual.hip; PaiNNGradForceTrainStep).
 * With F = -d(sum_b E_b)/d(pos) in the loss and v = dL/dF held constant, grad_theta of the force term is -grad_theta D,
 * D = d/d eps sum_b E_b(pos + eps v) at eps = 0: one tangent forward in which every activation a carries a_dot, and one
 * reverse pass through the joint (primal, tangent) graph.  These are the dual forms of the step's nonlinear operators
 * (the reference: torch.autograd with create_graph=True through models/painn/painn.py:318-340, 380-414):
 *     forward   (y, y_dot = J x_dot);    backward   x_bar = J^T y_bar + (d/dx [J x_dot])^T y_dot_bar,  x_dot_bar = J^T y_dot_bar
 * A DUAL OPERAND (suffix 2) holds its primal block followed by its tangent block of the same shape, so the linear layers in
 * between run as adf_op_linear_fwd / adf_op_linear_bwd over twice the rows; a strided operand's tangent block lies
 * rows * stride floats behind its primal block.  Exact f32, one launch per direction, no float atomics, fixed summation
 * order.  num_edges: the edge count adf_graph_build returned (the row count of the per-edge blocks).
 *
 * e_tan [num_edges, 4] = (u_dot, d_dot) of every edge row for the position tangent v [N,3]: with delta = v[src] - v[owner],
 * d_dot = u . delta and u_dot = (delta - u d_dot) / d; where the distance floor holds, d_dot = 0 and u_dot = delta / d. */
int32_t adf_op_edge_tangent(adf_painn_t h, const float* v, float* e_tan, int64_t num_edges, void* stream);
/* rbf2 [2 num_edges, num_rbf]: the radial basis of adf_op_rbf, then its tangent rbf'(d) d_dot. */
int32_t adf_op_rbf_dual(adf_painn_t h, const float* e_tan, float* rbf2, int64_t num_edges, void* stream);
/* y[m, :] += bias for the first M rows (row stride ldy) of a stacked product: its tangent rows take no bias. */
int32_t adf_op_dual_bias(float* y, int32_t ldy, const float* bias, int64_t M, int32_t N, void* stream);
/* ScaledSiLU on n elements per block: y_dot = f'(h) h_dot;  dh = dy f' + dy_dot f'' h_dot,  dh_dot = dy_dot f'. */
int32_t adf_op_ssilu_dual_fwd(const float* h2, float* y2, int64_t n, void* stream);
int32_t adf_op_ssilu_dual_bwd(const float* h2, const float* dy2, float* dh2, int64_t n, void* stream);
/* LayerNorm with adf_op_layernorm_fwd's corrected two-pass moments (stats [N,2] as there).  The backward ACCUMULATES into
 * dx2 and writes dw, db [H] (the tangent rows add to dw, not to db); scratch: 512 * 2 * H floats; H <= 1024. */
int32_t adf_op_layernorm_dual_fwd(const float* x2, const float* w, const float* b, float* y2, float* stats, int32_t N,
                                  int32_t H, void* stream);
int32_t adf_op_layernorm_dual_bwd(const float* x2, const float* w, const float* stats, const float* dy2, float* dx2, float* dw,
                                  float* db, int32_t N, int32_t H, float* scratch, void* stream);
/* adf_op_vdot_fwd / _bwd: dot = sum_k v1 v2 / sqrtC, nrm = sqrt(sum_k v2^2 + eps) of vv2 [2][N,3,2C]; nrm2 / dnrm2 with row
 * strides ldn / lddn; dv1_2 [2][N,3,C] (may be NULL): a direct gradient of v1. */
int32_t adf_op_vdot_dual_fwd(const float* vv2, float* dot2, float* nrm2, int32_t ldn, int64_t N, int32_t C, float eps,
                             void* stream);
int32_t adf_op_vdot_dual_bwd(const float* vv2, const float* nrm2, int32_t ldn, const float* ddot2, const float* dnrm2,
                             int32_t lddn, const float* dv1_2, float* dvv2, int64_t N, int32_t C, void* stream);
/* adf_op_update_out_fwd / _bwd on dual operands; every output is written. */
int32_t adf_op_update_out_dual_fwd(const float* x1_2, const float* vec1_2, const float* a2, const float* dot2, const float* vv2,
                                   float s, float* x2_2, float* vec2_2, int64_t N, int32_t H, void* stream);
int32_t adf_op_update_out_dual_bwd(const float* a2, const float* dot2, const float* vv2, float s, const float* dx2_2,
                                   const float* dvec2_2, float* da2, float* ddot2, float* dv1_2, float* dx1_2, float* dvec1_2,
                                   int64_t N, int32_t H, void* stream);
/* The message block (adf_op_message_fwd / _bwd: the plain path, rbfh2 / drbfh2 [2 num_edges, 3H] materialised) on the
 * handle's current graph.  Forward: one workgroup per target atom over its CSR segment, the primal sum and the four
 * one-factor-replaced tangent terms in one pass.  Backward: one workgroup per source atom over its own segment through the
 * reverse rows; writes dxh2, drbfh2 (at the segment's own rows, as adf_op_message_bwd), dvec2 (unless vec_is_zero: vec2 and
 * dvec2 may be NULL) and the residual path dx2. */
int32_t adf_op_message_dual_fwd(adf_painn_t h, const float* e_tan, const float* xh2, const float* vec2, const float* rbfh2,
                                const float* x2, float* x1_2, float* vec1_2, int32_t vec_is_zero, int64_t num_edges,
                                void* stream);
int32_t adf_op_message_dual_bwd(adf_painn_t h, const float* e_tan, const float* xh2, const float* vec2, const float* rbfh2,
                                const float* gx1_2, const float* gv1_2, float* dxh2, float* drbfh2, float* dvec2, float* dx2,
                                int32_t vec_is_zero, int64_t num_edges, void* stream);

#ifdef __cplusplus
}
#endif
