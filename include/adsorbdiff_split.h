/*
 * adsorbdiff_split.h — the C ABI of "two half-batches, two streams" (csrc/stepper.hip sample_loop_split).
 * A companion of adsorbdiff_hip.h with the same conventions (status codes, device pointers, `stream` = hipStream_t);
 * adsorbdiff_amd/lib.py binds its prototypes from this text exactly as it binds the main header's.
 *
 * Systems of a batch never interact, so the two sides of a cut at a system boundary are two independent dependent chains
 * of kernels.  adf_sample_split runs view A (systems [0, cut)) on the caller's stream with the handle and view B (systems
 * [cut, B)) on a library-owned non-blocking stream with the handle's twin, forked by one event at entry and joined by one
 * event before it returns; the host enqueues step t of A, then step t of B.  Every result - positions, f1 / f2, state,
 * the per-system table - has the bits of adf_sample on the whole batch.
 */
#ifndef ADSORBDIFF_SPLIT_H
#define ADSORBDIFF_SPLIT_H

#include "adsorbdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct adf_painn* adf_painn_t;

/* A second handle that borrows `parent`'s weight images (fp32 weights, fp16 hi/lo and fragment arenas, rbf images, scale
 * factors, switches) through const pointers and owns everything a forward writes: workspaces, graph buffers, kept
 * per-layer state, row-maxima slots, counters, flags, profiler, and the second stream with its events.  A handle has at
 * most one twin.  adf_painn_set_weights on the parent re-points the twin in the same call; on a twin it is ADF_EINVAL.
 * adf_painn_destroy of a parent whose twin lives is ADF_EINVAL: destroy the twin first.  While a twin exists,
 * adf_profile_enable / adf_profile_read / adf_get_counters / adf_check_flags on the parent cover both handles: times,
 * group counts, k-steps and incremental-layer totals are sums (under overlap the category times add up to more than wall
 * time), edge and atom counts are sums when the last sampling run was split, flags are ORed. */
int32_t adf_painn_create_twin(adf_painn_t parent, adf_painn_t* out);

/* The switch (adf_tune::sample_split, read from ADF_SAMPLE_SPLIT at creation). */
int32_t adf_painn_set_split(adf_painn_t h, int32_t on);

/* Where to cut.  natoms [B] and edges [B] (may be NULL: no tie-break) are HOST arrays; nothing touches the device.
 * *cut in [1, B - 1] = systems of view A: the boundary where |atoms(A) - atoms(B)| is least; among equal differences the
 * one where |edges(A) - edges(B)| (per-system edge counts of a previous build) is least, then the lowest.  B < 2: *cut = 0
 * (no split). */
int32_t adf_split_choose_cut(const int32_t* natoms, const int64_t* edges, int32_t num_systems, int32_t* cut);

/* View B.  pos, cell, atomic_numbers, tags, fixed, f1, f2, the noise tables, the moving mask and the per-system table are
 * read through pointer offsets into the caller's arrays - nothing of them is copied.  What counts atoms or systems from
 * the start of its batch cannot be an offset pointer and is handed over re-based to view B's first atom / system (small
 * int32 device arrays the caller keeps alive for the call; the moving lists for as long as the static-atom promise). */
typedef struct {
    int32_t cut;                  /* systems of view A, from adf_split_choose_cut                                    */
    int32_t atoms_a;              /* atoms of view A                                                                 */
    int32_t n_out_a;              /* entries of out_idx that lie in view A (out_idx is ascending)                    */
    int32_t n_out_b;              /* n_out - n_out_a                                                                 */
    const int32_t* atom_offset;   /* [B - cut + 1] view B's prefix sum of natoms, starting at 0                      */
    const int32_t* batch;         /* [N - atoms_a] view B's system index, starting at 0                              */
    const int32_t* out_idx;       /* [n_out_b] view B's listed atoms minus atoms_a (NULL when out_idx is NULL)       */
    const int32_t* mov_idx;       /* adf_graph_set_moving's mov_idx entries of view B minus atoms_a (NULL: no promise) */
    const int32_t* mov_off;       /* [B - cut + 1] offsets into it, starting at 0                                    */
} adf_split_view;

/* adf_sample (same arguments and contracts; b, out_idx and every array describe the WHOLE batch) on two streams.
 * b->reps is the whole batch's image count and is used for both views.  state is combined on the device at the join;
 * the numeric flags of both handles are read together by adf_check_flags(h).  The one-stream loop runs instead - on `h`
 * alone, unchanged - when the switch is off, the batch has fewer than two systems, the handle is in exact-f32 arithmetic,
 * or the coupled early stop is on (early_stop_count > 0 without adf_painn_set_per_system_stop: every step then depends on
 * all systems).  Per-system early stop is eligible, with the polling of adf_sample.  Trajectory sinks, step hooks and the
 * translation-only samplers have no split form: call their own entries. */
int32_t adf_sample_split(adf_painn_t h, adf_painn_t twin, const adf_batch* b, const adf_split_view* view, float* pos,
                         const int32_t* tags, const int32_t* fixed, const adf_step_coef* coefs_dev, int32_t num_steps,
                         const float* z_tr_all, const float* z_rot_all, int32_t early_stop_count, int32_t poll_every,
                         int32_t* state, const int32_t* out_idx, int32_t n_out, float* f1, float* f2, void* stream);

/* Sampling runs of adf_sample_split on `h` that went through the split loop / that ran the one-stream loop instead. */
int32_t adf_split_stats(adf_painn_t h, int64_t* split_runs, int64_t* fallback_runs);

#ifdef __cplusplus
}
#endif
#endif
