#pragma once
#include "../../include/adsorbdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Geometric gradient of the EquiformerV2 training graph (csrc/eqv2_geo.hip, adsorbdiff_amd/eqv2_train_step.py::
 * EqV2EnergyGradient): what the backward of the edge operators of csrc/eqv2_train.h / csrc/eqv2_s2ef_train.h leaves out because
 * there the Wigner rows wig [E, DR] and the distances dist [E] are inputs.  With these five entries they are functions of the
 * edge vectors, and forces = -dE/dpos of the energy the same graph reports, with the edge set held fixed.
 *
 * Stateless entries on caller-owned DEVICE float32 buffers; the handle is read for its dimensions and constant tables only.
 * Exact f32, no atomics of any kind; every output element is written by one thread in the one summation order written below,
 * so two calls on the same input give the same bits.  Layouts as in csrc/eqv2_train.h: wig / dwig [E, DR] hold the kept rows
 * |m| <= min(l, mmax) of D_l at d_off[l], row-major [2 min(l, mmax) + 1][2l + 1]; r(l, m) is the order-major reduced index of
 * a tensor [E, S_r, W] in the edges' frames.  adsorbdiff_amd/lib.py binds this text with the parser it uses for
 * include/adsorbdiff_hip.h. */

/* The Wigner term of adf_op_eq_rotate_in_fwd's backward: with out = radial * (D [x[src] | x[dst]]),
 * dwig[e, l, i, j] = dwig[e, l, i, j] + sum_c (dout[e, r(l, m_i), c] * radial[e, w(l, |m_i|), c]) * xcat[l^2 + j, c], xcat =
 * [x[src[e]] | x[dst[e]]], over the 2C channels c in index order, started from 0.  One wave per edge; the edge's two node
 * rows are staged once, 64 channels at a time. */
int32_t adf_op_eq_rotate_in_bwd_wig(adf_eqv2_t h, const float* x, const int32_t* src, const int32_t* dst, const float* radial,
                                    const float* dout, int64_t E, float* dwig, void* stream);

/* The Wigner term of adf_op_eq_rotate_out_fwd's backward: with agg[n] = sum_e D^T (rescale * alpha * z),
 * dwig[e, l, i, j] = dwig[e, l, i, j] + sum_ch (z[e, r(l, m_i), ch] * alpha[e, ch / V] * rescale_l) * dagg[dst[e], l^2 + j, ch]
 * over the NH V channels in index order, started from 0.  only_l >= 0: that degree's rows alone; -1: all. */
int32_t adf_op_eq_rotate_out_bwd_wig(adf_eqv2_t h, const float* z, const float* alpha, int32_t NH, int32_t V, const int32_t* dst,
                                     const float* dagg, int32_t only_l, int64_t E, float* dwig, void* stream);

/* The data gradient adf_op_eq_radial_gauss_bwd leaves out: ddist[e] = ddist[e] + sum_c dh0[e, c] T_c, c ascending from 0,
 * T_c = sum_k W0[c, k] g_k'(dist[e]) over the edge's window only, k ascending from 0; g_k' = g_k 2 coeff (d - mu_k)
 * (eq_gauss_dvalue, csrc/eqv2_gauss.h: the basis, its centres, coeff and the window are that header's).  W0 = net.0.weight
 * with row stride ldw (floats).  scratch: NB EC floats (the transposed Gaussian columns). */
int32_t adf_op_eq_radial_gauss_dgrad(adf_eqv2_t h, const float* dist, const float* W0, int32_t ldw, const float* dh0, int64_t E,
                                     float* ddist, float* scratch, int64_t scratch_floats, void* stream);

/* dvec [E, 3] = ddist n + (n x tau) / |vec|, n = vec / |vec|, tau_k = sum_l <dwig_l, wig_l K_k^l> (k = x, y, z; degrees and
 * the elements of a degree in index order per lane, then the 64 lanes by a fixed butterfly).  K_k^l are the constant
 * generators of D_l (D_l(exp(t [e_k])) = 1 + t K_k^l + ...; built from J_l by adf_eqv2_set_constants): a rotation of the lab
 * multiplies the edge's frame on the right, so the derivative needs the kept rows in wig only, and neither the frame's
 * angles nor their poles (an edge along +-y) enter.  The result is the gradient of any function of wig that does not depend on
 * the roll of the frame about the edge - the energy is one.  wig: the rows adf_eqv2_export_graph handed out. */
int32_t adf_op_eq_wigner_bwd(adf_eqv2_t h, const float* vec, const float* wig, const float* dwig, const float* ddist, int64_t E,
                             float* dvec, void* stream);

/* forces [N, 3] = -dE/dpos from dvec = dE/dvec: vec points target -> source image, so dE/dpos[dst] -= dvec and
 * dE/dpos[src] += dvec.  g = 0; first n's incoming edges eptr[n] .. eptr[n+1] in list order (g -= dvec), then its outgoing
 * edges in the order of sperm (g += dvec; sptr [N+1] / sperm [E]: the edge numbers sorted by source, ties in list order, as in
 * adf_op_eq_rotate_in_bwd; entries are clamped to [0, E)); forces[n] = -g.  An atom without edges gets exactly zero. */
int32_t adf_op_eq_edge_grad_to_atoms(const float* dvec, const int32_t* eptr, const int32_t* sptr, const int32_t* sperm, int32_t N,
                                     int64_t E, float* forces, void* stream);

#ifdef __cplusplus
}
#endif
