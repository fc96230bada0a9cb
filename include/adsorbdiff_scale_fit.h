/*
 * adsorbdiff_scale_fit.h - the C ABI of the scale-factor fit (csrc/scale_fit.hip, api.hip).
 * A companion of adsorbdiff_hip.h with the same conventions (status codes, device pointers, `stream` = hipStream_t);
 * adsorbdiff_amd/lib.py binds its prototypes from this text exactly as it binds the main header's.
 *
 * Fitting the scale factors (modules/scaling/fit.py, scale_factor.py:106-172): a ScaleFactor observes
 * torch.mean(torch.var(x, dim=0)) of the node features it returns, batch by batch; the fit is sqrt(1 / (the atom-weighted
 * mean of those)).
 */
#ifndef ADSORBDIFF_SCALE_FIT_H
#define ADSORBDIFF_SCALE_FIT_H

#include "adsorbdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct adf_painn* adf_painn_t;

/* adf_op_column_variance: out[0] (device double) = the mean over the H columns of the unbiased variance over the N rows of
 * x (device float32 [N, H], rows contiguous).  Float64 throughout and two passes (column means, then the centred squares);
 * partial sums meet in a fixed order and there are no atomics, so two runs give the same bits.  Any H >= 1; rows are read
 * 16 bytes per lane when H % 4 == 0.  scratch: device memory of adf_op_column_variance_scratch(N, H) bytes (0 for N < 1 or
 * H < 1), 8-byte aligned, written here.  N < 2 (torch gives NaN there), H < 1 or a null pointer: ADF_EINVAL.  Enqueues four
 * launches on `stream`, no host synchronisation. */
int64_t adf_op_column_variance_scratch(int64_t N, int32_t H);
int32_t adf_op_column_variance(const float* x, int64_t N, int32_t H, double* out, void* scratch, void* stream);

/* The ordinary full forward of adf_painn_forward (every row computed: no subset, no incremental lists; the handle's
 * arithmetic, f16x3 or exact f32) that also observes: after update layer l has applied its scale multiplier, layer_var[l]
 * (device double [num_layers]) receives adf_op_column_variance of x.  upto in [0, num_layers): the layers after `upto` are
 * not run and their entries of layer_var are left unwritten, so observing layer l costs l + 1 layers.  f1 / f2: the heads'
 * outputs as in adf_painn_forward, or both NULL: the heads are skipped.  They must be NULL when upto < num_layers - 1; with
 * f1 given, a two-head handle needs f2 too.  A handle with an energy head is served the same way (the energy head is not
 * evaluated).  Like a call on another batch, it ends a static-atom promise (adf_graph_set_moving) and invalidates the graph
 * cache, the layer-0 records and the kept layer state; what adf_painn_forward returns afterwards is unchanged.  Batches
 * of fewer than 2 atoms: ADF_EINVAL.  Flags: adf_check_flags, as the forward. */
int32_t adf_painn_forward_observe(adf_painn_t h, const adf_batch* b, int32_t upto, double* layer_var, float* f1, float* f2,
                                  void* stream);

#ifdef __cplusplus
}
#endif
#endif
