#pragma once
#include "../../include/adsorbdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Training operators of the EquiformerV2 S2EF force field (csrc/eqv2_s2ef_train.hip,
 * adsorbdiff_amd/eqv2_train_step.py::RadialMLPLive): the Gaussian part of a radial MLP's first layer, forward and weight
 * gradient, on the LIVE distance basis the inference forward evaluates.  g_k, the centres, coeff and the window rule are
 * csrc/eqv2_gauss.h's, the one definition eq_radial_live_kernel uses too; a term outside an edge's window (at most 58 of
 * the NB functions) is never formed, in either direction.  The handle is read for NB = num_distance_basis, EC =
 * edge_channels and max_radius only.  Stateless entries on caller-owned DEVICE float32 buffers, exact f32, no atomics of any
 * kind; every sum runs in the one order written below, so two calls on the same input give the same bits.  adsorbdiff_amd/
 * lib.py binds this text with the parser it uses for include/adsorbdiff_hip.h.  scratch_floats says what scratch holds
 * (less than the entry needs: ADF_EINVAL). */

/* dist [E] = |vec_e| (vec [E, 3]) as the kernels of the basis evaluate it: the distances of the two entries below. */
int32_t adf_op_eq_edge_dist(const float* vec, int64_t E, float* dist, void* stream);

/* h0 [E, EC] (dense rows) += the Gaussian part of the first layer: h0[e, c] = h0[e, c] + T, T = sum_k W0[c, k] g_k(dist[e])
 * over the edge's window only, k ascending, started from 0.  W0 = net.0.weight [EC, NB + 2 EC] with row stride ldw (floats);
 * the Gaussian columns come first.  scratch: NB EC floats (the transposed Gaussian columns, so that a wave reads a
 * column's EC weights as one row). */
int32_t adf_op_eq_radial_gauss_fwd(adf_eqv2_t h, const float* dist, const float* W0, int32_t ldw, int64_t E, float* h0,
                                   float* scratch, int64_t scratch_floats, void* stream);

/* Its weight gradient from dh0 [E, EC]; there is no data gradient (distances are inputs).  dW0[c, k] (row stride lddw) =
 * dW0[c, k] + (P_0 + P_1 + ... + P_7), added in that order, over the edges whose window holds k; the other columns of dW0,
 * those no edge's window reaches included, are not touched.  perm [E] int32: the edge numbers sorted by dist, ascending,
 * ties in list order (torch.sort(dist, stable=True)); the window's ends do not decrease with the distance, so the edges
 * of a column are one contiguous range [lo, hi) of perm, and P_w = the sum of g_k(dist[perm[i]]) dh0[perm[i], c] over
 * i = lo + w, lo + w + 8, ..., ascending, started from 0.  A perm that is not sorted gives other sums but reads and writes
 * nothing out of bounds (entries are clamped to [0, E)).  scratch: 4 E floats. */
int32_t adf_op_eq_radial_gauss_bwd(adf_eqv2_t h, const float* dist, const int32_t* perm, const float* dh0, int64_t E,
                                   float* dW0, int32_t lddw, float* scratch, int64_t scratch_floats, void* stream);

#ifdef __cplusplus
}
#endif
