/*
 * adsorbdiff_hip.h — C ABI of libadsorbdiff_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the denoising-diffusion sampling hot path of AdsorbDiff.
 * The reference has no FFI of its own (it is pure Python on top of PyTorch /
 * torch_scatter); each entry point below replaces the Python-level interface
 * named in its comment (paths relative to the reference tree).  The Python
 * binding that a maintainer adds is a ctypes stub — see INTEGRATION.md and
 * adsorbdiff_amd/lib.py.
 *
 * Conventions
 *   - every function returns an int32 status: ADF_OK, or an ADF_E* code; the
 *     message of the last failure on the calling thread is adf_last_error().
 *     ADF_EOOM is what the host shim turns into RuntimeError so that
 *     ml_diffuse's split-the-batch-and-retry contract keeps working
 *     (relaxation/ml_relaxation.py:146-165); ADF_ENONEIGHBOR becomes the
 *     ValueError of painn_denoising.py:370-375.
 *   - all array arguments are caller-owned DEVICE pointers, row-major, float32
 *     or int32 as named; `stream` is a hipStream_t passed as void*.
 *   - a handle is bound to the device that was current at adf_painn_create and
 *     is NOT thread-safe.  Work is enqueued on `stream`; nothing synchronises
 *     unless stated.
 *   - the operators of the EquiformerV2 training graph are declared beside
 *     their translation units and bound by adsorbdiff_amd/lib.py from that
 *     text: csrc/eqv2_train.h (edge side, forward and backward),
 *     csrc/eqv2_s2ef_train.h (the live Gaussian basis), csrc/eqv2_geo.h (the
 *     gradient with respect to the edge geometry: energy-gradient forces).
 *     So are the dual operators of the PaiNN step that trains on
 *     energy-gradient forces: csrc/dual_ops.h.
 */
#ifndef ADSORBDIFF_HIP_H
#define ADSORBDIFF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADF_OK 0
#define ADF_EINVAL 1      /* invalid argument / unsupported hyper-parameter        */
#define ADF_EOOM 2        /* device allocation failed                             */
#define ADF_ENONEIGHBOR 3 /* an image has no neighbours (painn_denoising.py:370)  */
#define ADF_EHIP 4        /* HIP runtime error                                    */
#define ADF_EOVERFLOW 5   /* candidate list of one centre exceeded its capacity   */
#define ADF_ENUMERIC 6    /* non-finite model output (see adf_painn_set_arithmetic) */

typedef struct adf_painn* adf_painn_t;

/* Hyper-parameters of the PaiNN denoiser: the constructor arguments of
 * adsorbdiff.models.painn.painn_denoising.PaiNN (painn_denoising.py:57-81)
 * that reach the arithmetic. */
typedef struct {
    int32_t hidden_channels;   /* H, multiple of 64                              */
    int32_t num_layers;
    int32_t num_rbf;           /* R, even, <= 128                                */
    int32_t num_elements;      /* rows of the atom embedding table               */
    int32_t max_neighbors;     /* K of the strict top-K neighbour cap, <= 128    */
    int32_t envelope_exponent; /* p of the polynomial envelope                   */
    int32_t num_heads;         /* 2 when so3_denoising else 1; 0: no force head (S2EF energy only) */
    float cutoff;              /* Angstrom                                       */
} adf_painn_hparams;

/* Order of the weight table handed to adf_painn_set_weights (all float32,
 * torch.nn.Linear layout [out, in]; names are the reference state_dict keys):
 *   0  atom_emb.embeddings.weight              [num_elements, H]
 *   1  radial_basis.rbf.offset                 [R]
 *   then per layer l (13 entries, base 2 + 13*l):
 *    +0  message_layers.l.x_layernorm.weight   [H]
 *    +1  message_layers.l.x_layernorm.bias     [H]
 *    +2  message_layers.l.x_proj.0.weight      [H, H]
 *    +3  message_layers.l.x_proj.0.bias        [H]
 *    +4  message_layers.l.x_proj.2.weight      [3H, H]
 *    +5  message_layers.l.x_proj.2.bias        [3H]
 *    +6  message_layers.l.rbf_proj.weight      [3H, R]
 *    +7  message_layers.l.rbf_proj.bias        [3H]
 *    +8  update_layers.l.vec_proj.weight       [2H, H]
 *    +9  update_layers.l.xvec_proj.0.weight    [H, 2H]
 *    +10 update_layers.l.xvec_proj.0.bias      [H]
 *    +11 update_layers.l.xvec_proj.2.weight    [3H, H]
 *    +12 update_layers.l.xvec_proj.2.bias      [3H]
 *   then per head h in {out_forces, out_forces2}, per block b in {0,1} (6 entries):
 *    +0 output_network.b.vec1_proj.weight  +1 vec2_proj.weight
 *    +2 update_net.0.weight  +3 update_net.0.bias  +4 update_net.2.weight  +5 update_net.2.bias
 */
#define ADF_WEIGHTS_PER_LAYER 13
#define ADF_WEIGHTS_PER_HEAD 12

/* Replaces constructing the model (painn_denoising.py:57-148).  Accepted: hidden_channels a multiple of 64 in
 * [128, 1024], num_rbf even in [2, 128], max_neighbors in [1, 128], num_layers in [1, 16], num_heads in [0, 2], any
 * envelope exponent; anything else is ADF_EINVAL.  A num_rbf that is no multiple of 8 does not fit the 16-byte pieces
 * of the f16 message kernel's rbf_proj image: such a handle runs the message block in its exact-f32 kernel in either
 * arithmetic (adf_painn_set_arithmetic then only switches the node products). */
int32_t adf_painn_create(const adf_painn_hparams* hp, adf_painn_t* out);
int32_t adf_painn_destroy(adf_painn_t h);

/* (Re)bind the weights.  Pointers are device pointers that stay owned by the
 * caller and must outlive their use; rbf_proj is re-packed into the library's
 * own layout.  scale_factors: HOST array [num_layers], the effective
 * upd_out_scalar_scale_l multipliers (1.0 when unfitted; scale_factor.py:166). */
int32_t adf_painn_set_weights(adf_painn_t h, int32_t n_weights, const void* const* weights,
                              const float* scale_factors, void* stream);

/* Describes one batch of independent adsorbate+slab systems (the fields of the
 * PyG Batch the reference's forward reads).  All device. */
typedef struct {
    int32_t num_systems;          /* B                                            */
    int32_t num_atoms;            /* N                                            */
    const float* pos;             /* [N,3]                                        */
    const float* cell;            /* [B,3,3]  rows = lattice vectors              */
    const int32_t* atomic_numbers;/* [N]                                          */
    const int32_t* batch;         /* [N] system index, non-decreasing             */
    const int32_t* atom_offset;   /* [B+1] prefix sum of natoms                   */
    int32_t reps[3];              /* periodic images per lattice direction (host) */
} adf_batch;

/* Replaces BaseModel.generate_graph + PaiNN.generate_graph_values
 * (models/base.py:33-123, painn_denoising.py:353-400): periodic radius graph,
 * strict top-K, symmetrisation.  The graph stays in the handle.  *num_edges
 * (HOST, may be NULL) forces a stream sync when non-NULL. */
int32_t adf_graph_build(adf_painn_t h, const adf_batch* b, void* stream, int64_t* num_edges);

/* Static-atom cache for repeated graph builds of the SAME batch in which only some atoms move
 * (sampling: the adsorbate; denoising_torch.py:353 only rewrites pos[tags == 2]).  moving: [N] int32
 * mask (1 = may move), mov_idx: indices of the moving atoms grouped by system, mov_off: [B+1] offsets
 * into mov_idx; all caller-owned device arrays that must stay valid until reset.  The next build
 * evaluates everything and caches each static centre's K nearest static candidates; later builds
 * only re-evaluate candidates that involve a moving atom — results are identical to a full build.
 * While the promise is in force adf_painn_forward also keeps the layer-0 gather records across calls: they depend
 * on the atomic numbers only (x0 = emb(Z), vec0 = 0), so the batch's atomic numbers and the weights must not change
 * either (adf_painn_set_weights invalidates).  Pass NULLs to switch the cache off (default).  Any call invalidates. */
int32_t adf_graph_set_moving(adf_painn_t h, const int32_t* moving, const int32_t* mov_idx, const int32_t* mov_off);

/* Arithmetic of the dense products: 0 = f16x3 (three fp16 matrix-core products per fp32 product, fp32 accumulate:
 * 2^-22 relative per product for activations inside the fp16 range, |a| <= 65504; default), 1 = exact f32 MFMA (the
 * reference's width, models/painn/README.md:12; ~2x slower).  A forward whose output is not finite reports
 * ADF_ENUMERIC through adf_check_flags; the host mirror then re-runs the forward / the sampling run in exact f32. */
int32_t adf_painn_set_arithmetic(adf_painn_t h, int32_t exact_f32);

/* Incremental layers (default on; ADF_INCREMENTAL=0 in the environment at creation = off).  While a static-atom promise
 * is in force (adf_graph_set_moving: same batch, only flagged atoms move) the handle keeps x / vec / gather records of
 * every layer and a forward recomputes a node row only if one of its inputs — its own row in the layer below, a
 * neighbour's, or its in-edge list / geometry, compared bit for bit with the previous build — changed since the row
 * was computed.  Every output is bit-identical to a full forward; the reference recomputes everything every step
 * (denoising_torch.py:498 -> painn_denoising.py:460-471).  Costs about 110 KB of HBM per atom (H=512, 6 layers).
 * The lengths of the recompute lists stay on the device: list-mode launches are sized for all N rows and every kernel
 * of a layer reads its row count from device memory; the host sees the counts one forward late (pinned double buffer
 * behind an event it polls without waiting) and uses them only to choose between the list and the all-rows form of a
 * layer - an incremental forward synchronises nothing (ADF_INC_SYNC=1 restores a synchronous 52-byte read-back).
 * Calling this (with either value) drops the kept state and zeroes the counters adf_get_counters reports. */
int32_t adf_painn_set_incremental(adf_painn_t h, int32_t on);

/* Kernel-selection switches.  Each chooses between kernels that compute the same thing (same K order per output element:
 * same bits); the non-default values select the independent form a test compares the default against, or a path that some
 * inputs run anyway.  adf_painn_create reads them from the
 * environment once and the handle keeps its own copy, so handles created under different environments coexist in one
 * process.  The stateless entries (adf_linear_forward, adf_op_*) share one copy read at their first use. */
typedef struct adf_tune {
    int32_t gemm_stream;      /* ADF_GEMM_STREAM: test hook.  0 = every f16x3 node product runs the LDS-staged form, the reference the
                               * bit-identity tests compare against; else 1 (default): the streamed form wherever a shape allows it */
    int32_t head_gate_fused; /* ADF_HEAD_GATE_FUSED: 0 = the heads' gate in a kernel of its own, else 1 (default) */
    int32_t lift_emit;        /* ADF_LIFT_EMIT: 0 = x_proj's row magnitudes are measured, else 1 (handed on by the producers) */
    int32_t graph_sys_csr;    /* ADF_GRAPH_SYS_CSR: 0 = global-memory count / fill / sort only, else 1 (default) */
    int32_t train_gemm16;     /* ADF_TRAIN_GEMM: "f32" = 0, the training products in exact f32, else 1 (stateless entries only) */
    int32_t wgrad_f32;        /* ADF_WGRAD: "f32" = 1, weight gradients in exact f32, else 0 (stateless entries only) */
    /* EquiformerV2 (adf_eqv2_create keeps the same copy) */
    int32_t eqv2_gemm_tile256;   /* ADF_EQV2_GEMM_TILE: 128 = 0, the 128-row tile for every shape, else 1 (256 rows from 8192 on) */
    int32_t eqv2_rotin_generic;  /* ADF_EQV2_ROTIN_GENERIC set (any value): 1, the run-time-mmax rotate-in kernel, else 0 */
    int32_t eqv2_rotout_generic; /* ADF_EQV2_ROTOUT_GENERIC set (any value): 1, the run-time-mmax rotate-out kernel, else 0 */
    /* Two half-batches on two streams (the section of that name below; same bits as the one-stream loop) */
    int32_t sample_split;     /* ADF_SAMPLE_SPLIT: 0 = adf_sample_split runs the one-stream loop, else 1 (default): its two views
                               * run on two streams (adf_painn_set_split overrides) */
} adf_tune;
/* Test hook: the selection the handle holds (the variants give the same bits, so outputs cannot show it). */
int32_t adf_painn_get_tune(adf_painn_t h, adf_tune* out);

/* Read the device-side error flags of the last graph build (candidate overflow,
 * empty image).  Synchronises the stream.  adf_painn_forward does not check
 * them itself so that a sampling loop stays free of host round trips. */
int32_t adf_check_flags(adf_painn_t h, void* stream);

/* Copy the handle's current graph out (parity tests).  Directed top-K stage in
 * the reference's candidate order: nbr_count[N], nbr_src[N*K], nbr_shift[N*K*3].
 * Symmetrised stage (grouped by target, order within a group unspecified):
 * edge_src/edge_dst [cap], edge_dist [cap], edge_vec [cap*3]; returns E in
 * *num_edges.  Any pointer may be NULL.  Synchronises the stream. */
int32_t adf_graph_export(adf_painn_t h, int32_t* nbr_count, int32_t* nbr_src, int32_t* nbr_shift,
                         int64_t edge_capacity, int32_t* edge_src, int32_t* edge_dst, float* edge_dist,
                         float* edge_vec, int64_t* num_edges, void* stream);

/* Replaces PaiNN.forward(data) (painn_denoising.py:402-481): graph build + 6
 * message/update layers + the two gated-equivariant heads.  f1,f2: [N,3]
 * (f2 may be NULL when num_heads == 1). */
int32_t adf_painn_forward(adf_painn_t h, const adf_batch* b, float* f1, float* f2, void* stream);

/* The same forward when the caller reads the outputs of a subset of atoms only — the sampler: the per-system score
 * is the mean over the adsorbate atoms (denoising_torch.py:263-268, 460-467), the slab rows of f1 / f2 are never
 * read.  out_idx: n_out ascending atom indices (device int32).  All layers but the last run in full; the last
 * layer's message targets, its update and the heads are evaluated for the listed atoms only.  Rows out_idx[*] of
 * f1 / f2 are bit-identical to adf_painn_forward's; the other rows are NOT written. */
int32_t adf_painn_forward_subset(adf_painn_t h, const adf_batch* b, const int32_t* out_idx, int32_t n_out, float* f1,
                                 float* f2, void* stream);

/* Unit-testable pieces of the forward on the handle's current graph
 * (PaiNNMessage.forward, painn_denoising.py:530-567, fused with the residual
 * of :443-445):  x_out = (x + dx)/sqrt2 [N,H],  vec_out = vec + dvec [N,3,H]. */
int32_t adf_painn_message_layer(adf_painn_t h, int32_t layer, int32_t num_atoms, const float* x,
                                const float* vec, float* x_out, float* vec_out, void* stream);
/* PaiNNUpdate.forward + residual + ScaleFactor (painn_denoising.py:447-451,601-623), in place. */
int32_t adf_painn_update_layer(adf_painn_t h, int32_t layer, int32_t num_atoms, float* x, float* vec,
                               void* stream);
/* Test hook for the row maxima that the f16x3 path takes from the kernels that write the rows (ADF_ROW_MAXIMA, on by
 * default) instead of measuring passes: the maxima of the last launch, combined over the producers' slots.
 * which = 0: max|x_out| per row [rows] and 1: max|vec_out| per row and component [3 rows] of the last message launch;
 * 2: max of every |v2| row [rows] of the last vec_proj launch (adf_painn_update_layer); 3: the |v2| rows themselves
 * [rows, H].  which = 4 switches capture on (capacity != 0) or off and returns nothing: while it is on, vec_proj leaves its
 * slots on the per-layer entry above too (otherwise only where the library reads them) and the library keeps a copy of the
 * magnitudes it combined from the slots; which = 5 / 6 return that copy: the magnitudes of the vec rows [3 rows] / of the
 * [x | |v2|] rows [rows] as the last layer of the last forward handed them to its products.
 * *rows (optional) receives the row count; out: device floats, `capacity` of them (NULL: only query rows).
 * ADF_EINVAL when no launch has emitted maxima. */
int32_t adf_painn_debug_row_maxima(adf_painn_t h, int32_t which, float* out, int64_t capacity, int32_t* rows,
                                   void* stream);

/* Stand-alone torch.nn.functional.linear (+ optional ScaledSiLU) on device pointers, A[M,K]
 * W[N,K] bias[N] C[M,N] contiguous; K % 32 == 0.  mode 0: exact-f32 MFMA (gemm.hip); mode 1:
 * f16x3 split MFMA (gemm16.hip).  Unit-test entry for the dense blocks of painn_denoising.py:531,
 * 603, 609, 689-693; synchronises in mode 1. */
int32_t adf_linear_forward(const float* A, const float* W, const float* bias, float* C, int32_t M, int32_t N,
                           int32_t K, int32_t act_ssilu, int32_t mode, void* stream);

/* Per-step schedule scalars, computed by the host with the reference's own
 * 0-dim tensor arithmetic (denoising_torch.py:237-293) so that the products
 * round exactly as there:
 *   dcom = coef_tr * s_tr                      (+ noise_tr  * z_tr   in SDE mode)
 *   drot = ((rot_pre * s_rot) * rot_dt) * rot_g2 (+ noise_rot * z_rot in SDE mode)
 * ODE: coef_tr = 0.5*g_tr^2*dt, rot_pre = 0.5.  SDE: coef_tr = g_tr^2*dt, rot_pre = 1,
 * noise_tr = g_tr*sqrt(dt), noise_rot = g_rot*sqrt(dt). */
typedef struct {
    float coef_tr;
    float rot_pre;
    float rot_dt;
    float rot_g2;
    float noise_tr;
    float noise_rot;
} adf_step_coef;

/* Replaces the initial random placement (denoising_torch.py:215-232).
 * noise: [B,3] uniform [0,1) drawn by the host from the CPU generator. */
int32_t adf_sde_init_placement(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags,
                               const float* noise, void* stream);

/* Replaces one iteration of Denoiser.reverse_sde_sampling_rot after the model
 * call (denoising_torch.py:263-353 incl. DiffTorchCalc :491-500): zero f2 on
 * fixed atoms, per-system adsorbate means, ODE/SDE update, COM wrap, rigid
 * rotation+translation of the adsorbate, cumulative early-stop counter.
 * z_tr,z_rot: [B,3] standard normals (SDE only, else NULL).  state: device
 * int32[8] = {cumulative converged-step count, frozen flag, all-converged flag
 * of the step in flight, steps applied, steps issued, -, -, -}; the caller
 * initialises it to {0,0,1,0,0,0,0,0}.  Once the count reaches `early_stop_count` (>0) that step and all
 * later ones leave pos untouched, which is the reference's `break`
 * (denoising_torch.py:312-320).  dcom,drot: optional [B,3] outputs. */
int32_t adf_sde_step(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags,
                     const int32_t* fixed, const float* f1, const float* f2, const adf_step_coef* coef,
                     const float* z_tr, const float* z_rot, int32_t early_stop_count, int32_t* state,
                     float* dcom, float* drot, void* stream);

/* Same step with the whole schedule in a DEVICE table coefs_dev[num_steps], indexed by state[4]
 * (steps issued).  Every step is then the identical launch sequence, so forward + step can be
 * captured once into a hipGraph and replayed (small batches are launch-bound). */
int32_t adf_sde_step_scheduled(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags,
                               const int32_t* fixed, const float* f1, const float* f2,
                               const adf_step_coef* coefs_dev, int32_t num_steps, const float* z_tr,
                               const float* z_rot, int32_t early_stop_count, int32_t* state, float* dcom,
                               float* drot, void* stream);

/* Counters of the last adf_painn_forward: algorithmic bytes of the message
 * kernel, dense FLOPs, padded/real edge rows (bench.py roofline). */
/* The whole reverse loop of Denoiser.reverse_sde_sampling_rot after the initial placement (denoising_torch.py:
 * 235-356) in one call: num_steps x (adf_painn_forward[_subset] + adf_sde_step_scheduled), enqueued on `stream`.
 * z_tr_all, z_rot_all: [num_steps][B][3] standard normals (SDE) or both NULL (ODE).  poll_every > 0 (and
 * early_stop_count > 0): every poll_every steps the frozen flag state[1] is read back (one stream synchronisation)
 * and the loop ends once it is set — the reference's `break`; 0 = never synchronise for that (steps after the stop
 * are no-ops on pos; incremental layers never synchronise: their list lengths stay on the device, ADF_INC_SYNC=1 restores the
 * per-forward read-back).  out_idx / n_out: optional subset of atoms whose model outputs are evaluated (see
 * adf_painn_forward_subset), NULL = all.  f1, f2: [N,3] work arrays (last step's outputs on return). */
int32_t adf_sample(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags, const int32_t* fixed,
                   const adf_step_coef* coefs_dev, int32_t num_steps, const float* z_tr_all, const float* z_rot_all,
                   int32_t early_stop_count, int32_t poll_every, int32_t* state, const int32_t* out_idx,
                   int32_t n_out, float* f1, float* f2, void* stream);

/* ---- translation-only samplers: Denoiser.reverse_sde_sampling (denoising_torch.py:96-196, probability-flow ODE) and
 * Denoiser.langevin_dynamics (:369-458, annealed Langevin).  Per step:
 *   score = mean of head 1 (f1) over the tag-2 atoms of each system (_get_ads_output, :460-467)
 *   dcom  = coef * score (+ noise * z)   with dcom_z := 0, then the COM wrap of adf_sde_step (:150-166, :421-435)
 *   pos  += dcom on the tag-2 atoms (set_positions, :52-56); slab atoms are never written.
 * ODE: coef = 0.5*g_tr^2*dt (adf_step_coef.coef_tr with ode), noise unused, z = NULL.
 * Langevin: coef = step_size = step_lr*(sigma/sigma_min)^2, noise = sqrt(2*step_size), z = [B,3] standard normals;
 * the table runs over num_steps * n_step_each inner steps.  Both scalars are f32 values computed by the host with the
 * reference's own tensor arithmetic. */
typedef struct {
    float coef;
    float noise;
} adf_tr_coef;

/* One translation step after a forward: either `coef` (host) or the DEVICE table coefs_dev[num_steps] indexed by
 * state[4], as adf_sde_step / adf_sde_step_scheduled.  state: the int32[8] protocol of adf_sde_step (early stop:
 * cumulative count of steps where every |dcom| <= 1e-3, reverse_sde_sampling :168-176; pass 0 for Langevin, which has
 * none).  f1 is the only model output read.  dcom: optional [B,3] output (the wrapped increment). */
int32_t adf_tr_step(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags, const float* f1,
                    const adf_tr_coef* coef, const adf_tr_coef* coefs_dev, int32_t num_steps, const float* z,
                    int32_t early_stop_count, int32_t* state, float* dcom, void* stream);
/* The whole loop after the initial placement in one call: num_steps x (forward + adf_tr_step), with the poll_every,
 * out_idx / n_out contracts of adf_sample.  The forward evaluates head 1 only (no out_forces2 products: neither sampler
 * reads head 2; its head-1 rows are bit-identical to adf_painn_forward's).  z_all: [num_steps][B][3] or NULL.  f1: [N,3]
 * work array.  adf_tr_sample_traj pushes a frame after every frame_every-th step (adf_sample_traj). */
int32_t adf_tr_sample(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags, const adf_tr_coef* coefs_dev,
                      int32_t num_steps, const float* z_all, int32_t early_stop_count, int32_t poll_every,
                      int32_t* state, const int32_t* out_idx, int32_t n_out, float* f1, void* stream);

typedef struct {
    int64_t num_edges;
    int64_t num_atoms;
    int64_t message_bytes_per_layer;  /* SURVEY.md §8d formula on the real E, N */
    int64_t dense_flops;              /* node + edge GEMM flops of one forward  */
    /* incremental layers, totals since adf_painn_set_incremental: node rows recomputed / rows a full forward would
     * have computed (layers x atoms), message-kernel launches made and the in-edges of the targets they evaluated */
    int64_t inc_rows, inc_rows_full, inc_msg_launches, inc_msg_edges;
} adf_counters;
int32_t adf_get_counters(adf_painn_t h, adf_counters* out, void* stream);

/* ---- Per-system early stop (opt-in; csrc/stepper.hip).  sys_state: [B,4] int32 DEVICE memory owned by the caller, row b =
 * {cvg_count, frozen, steps_applied, stop_step}, initialised to {0, 0, 0, -1}; NULL switches the mode off.  While it is set,
 * adf_sde_step[_scheduled], adf_tr_step, adf_sample[_traj] and adf_tr_sample[_traj] on this handle apply the reference's
 * loop (denoising_torch.py:312-320) to every system on its own, as if it were sampled alone:
 *   frozen: nothing is read of f1 / f2 and nothing written to its pos rows; its dcom / drot output rows are 0;
 *   else dcom / drot as always; if its wrapped |dcom| <= 1e-3: cvg_count += 1, and when cvg_count == early_stop_count
 *   the system freezes with stop_step = state[4], this step's update NOT applied (the reference's break);
 *   a system that did not freeze gets the update and steps_applied += 1.  early_stop_count == 0: nothing freezes.
 * The arithmetic is the coupled path's own (shared device functions): at B = 1 both give the same bits.
 * state[] in this mode: [0] frozen systems, [1] 1 iff all B are frozen (what the fused loops poll), [3] max steps_applied,
 * [4] steps issued.  One kernel per step (one wave per system) plus a one-thread launch that advances state[4].
 * A call whose batch does not have B systems returns ADF_EINVAL. */
int32_t adf_painn_set_per_system_stop(adf_painn_t h, int32_t* sys_state, int32_t B);

/* Optional HIP-event timing of the kernel groups of adf_painn_forward / adf_sde_step, recorded
 * on the launch stream.  Categories: 0 graph build, 1 message kernel (one launch per layer),
 * 2 node-side dense blocks (LayerNorm + GEMMs + update), 3 output heads, 4 stepper.
 * adf_profile_read synchronises, returns summed milliseconds and number of timed groups per
 * category (arrays of 5) and resets the log.  *message_ksteps (optional) = sum over all 32-edge
 * row blocks of all message launches of (k-window length actually contracted x 32-column blocks that ran: 6, or 4 in
 * the vec == 0 launches of the first layer); executed MFMA flops of the message kernel = message_ksteps * 32 * 32 * 2
 * (x 3 products in the f16x3 arithmetic). */
#define ADF_PROF_NCAT 5
int32_t adf_profile_enable(adf_painn_t h, int32_t on);
int32_t adf_profile_read(adf_painn_t h, float* ms, int64_t* count, int64_t* message_ksteps, void* stream);

/* On-box peaks for the roofline fractions: out_host3[0] = HBM stream copy GB/s (read + write bytes of a
 * 1 GiB -> 1 GiB copy), [1] = v_mfma_f32_32x32x16_f16 TFLOP/s, [2] = v_mfma_f32_32x32x2_f32 TFLOP/s, both from a
 * register-resident loop on every CU with non-zero operands.  Measurement aid of bench.py, not on the sampling path. */
int32_t adf_measure_peaks(float* out_host3, void* stream);

/* ---- per-step trajectory frames.  Replaces Denoiser.write's blocking per-step host copy
 * (relaxation/diffusers/denoising_torch.py:358-367, 469-477; relaxation/ase_utils.py:19-48): a frame = the [N,3] positions
 * after a reverse step.  adf_frames_push snapshots `src` into one of two device staging buffers on `stream` and copies it
 * into slot (index % slots) of a pinned host ring on the sink's own stream; frames are numbered in push order.  A host
 * writer thread takes them with adf_frames_wait (blocks up to timeout_ms; *host_ptr = NULL on time-out) and gives the slot
 * back with adf_frames_release; push blocks the enqueueing thread only while the slot it needs is still unreleased.
 * adf_sample_traj / adf_eqv2_sample_traj = adf_sample / adf_eqv2_sample that push a frame after every `frame_every`-th
 * applied step (and after the last one) without leaving the fused loop.  adf_frames_abort cancels a sink: a push that is
 * waiting for a slot (or any later push) returns ADF_EINVAL and every wait returns at once - the host writer calls it when
 * it stops early (I/O error), so that the sampler reports the failure instead of blocking on a full ring.  Not thread-safe
 * per sink except wait / release / pushed / abort against push. */
typedef struct adf_frames* adf_frames_t;
int32_t adf_frames_create(int32_t device, int64_t frame_floats, int32_t slots, adf_frames_t* out);
int32_t adf_frames_destroy(adf_frames_t f);
int32_t adf_frames_push(adf_frames_t f, const float* src, void* stream);
int32_t adf_frames_wait(adf_frames_t f, int64_t index, int32_t timeout_ms, const float** host_ptr);
int32_t adf_frames_release(adf_frames_t f, int64_t index);
int64_t adf_frames_pushed(adf_frames_t f);
int32_t adf_frames_abort(adf_frames_t f);
int32_t adf_sample_traj(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags, const int32_t* fixed,
                        const adf_step_coef* coefs_dev, int32_t num_steps, const float* z_tr_all, const float* z_rot_all,
                        int32_t early_stop_count, int32_t poll_every, int32_t* state, const int32_t* out_idx,
                        int32_t n_out, float* f1, float* f2, adf_frames_t sink, int32_t frame_every, void* stream);
int32_t adf_tr_sample_traj(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags,
                           const adf_tr_coef* coefs_dev, int32_t num_steps, const float* z_all, int32_t early_stop_count,
                           int32_t poll_every, int32_t* state, const int32_t* out_idx, int32_t n_out, float* f1,
                           adf_frames_t sink, int32_t frame_every, void* stream);

/* Hand-off to the relaxation stage: the lift rule of scripts/create_lmdbs/pred_traj_to_lmdb.py:81-90 applied to the
 * sampled final frames on the device (in place).  lifted: optional [B] output = shift applied per system. */
int32_t adf_lift_adsorbates(float* pos, const int32_t* tags, const int32_t* atom_offset, int32_t B, float min_gap,
                            float* lifted, void* stream);

/* Relaxation anomalies (replaces DetectTrajAnomaly, adsorbdiff/placement/flag_anomaly.py:6-154, evaluated per structure on
 * the host with five ASE NeighborList builds) for a whole batch of relaxations, first frame against last frame.
 *   dmin(i,j)   = min over lattice vectors T of |p_j + T - p_i|, T over all integer combinations along the periodic
 *                 directions, T = 0 excluded when i == j (an atom can bind its own image: the diagonal counts);
 *   conn_m(i,j) = dmin(i,j) < m * (R_i + R_j) + 2 * skin   (strict), R = radii[atomic number];
 *   adsorbate = tag 2, slab = tag != 2, frozen = tag 0; slab_ref = pos_slab_ref, or the initial positions when NULL.
 *   flags[b] = { dissociated:     conn_1 over the adsorbate atoms differs between initial and final in any entry,
 *                desorbed:        no (adsorbate, slab) pair has conn_desorption_mult in the final positions (a system
 *                                 without adsorbate atoms is desorbed),
 *                surface_changed: a slab pair with conn_1(final) and not conn_surface_mult(slab_ref), or with
 *                                 conn_1(slab_ref) and not conn_surface_mult(final),
 *                intercalated:    an (adsorbate, frozen) pair with conn_1 in the final positions }  - scripts/eval.py's order.
 * b->pos: the initial positions; pos_final [N,3]; pos_slab_ref [N,3] aligned with the batch (rows of tag 2 are ignored);
 * radii: device table [num_radii]; flags: [B,4] int32, 0 or 1.  Positions need not be wrapped into the cell: every
 * displacement is reduced to its nearest image first.  b->reps: images tried per direction after that reduction, sized by
 * the caller for the largest threshold of the batch (engine.cell_repeats; anomaly.hip states why that suffices); a
 * direction with reps 0 is not periodic.  An atomic number outside [0, num_radii) returns ADF_EINVAL, reported like
 * adf_graph_build reports one outside its table: the call synchronises `stream` to read the error word.  The flags are
 * ORs of per-pair evidence, combined with integer atomics: bit-reproducible. */
int32_t adf_flag_anomalies(const adf_batch* b, const float* pos_final, const float* pos_slab_ref, const int32_t* tags,
                           const float* radii, int32_t num_radii, float skin, float surface_mult, float desorption_mult,
                           int32_t* flags, void* stream);

/* Rank the relaxed sites (scripts/eval.py:566-579: the minimum relaxed energy per system among the sites without an
 * anomaly).  Sites of group g are energy[group_offset[g] .. group_offset[g+1]).  A site is valid when its four flags
 * (flags [S,4], NULL: no filter) are 0 and its energy is not NaN.  best[g]: index into `energy` of the valid site of
 * least energy, ties to the lowest index, -1 without a valid site; best_energy[g] (may be NULL): its energy, +inf
 * without one; n_valid[g] (may be NULL): valid sites.  One launch, fixed reduction order, no atomics. */
int32_t adf_select_best_sites(const float* energy, const int32_t* flags, const int32_t* group_offset, int32_t num_groups,
                              int32_t* best, float* best_energy, int32_t* n_valid, void* stream);

/* ---- Duplicate sites (csrc/unique.hip; adsorbdiff_amd/site_select.py).  An extension: the reference has no
 * counterpart (scripts/run_vasp_dft/write_vasp_inputs_nsite.py takes the best N sites per slab on the host).  Every array
 * is a device array, outputs are written with plain stores, there are no float atomics, nothing is read back and every
 * result is bit-reproducible.  Sites are systems of a batch: atoms atom_offset[s] .. atom_offset[s+1] of pos / tags /
 * atomic_numbers, cell [S,9] with rows = lattice vectors.  Sites of group g are group_offset[g] .. group_offset[g+1]: the
 * caller has brought them into contiguous groups.
 *
 * adf_site_pair_distances.  Group g with n sites owns out[pair_offset[g] .. pair_offset[g] + n n): a full symmetric
 * [n,n] matrix with a zero diagonal (a group whose matrix does not fit into out_len elements is left unwritten).
 *   d(a,b) = max(d_ads, d_slab).  The displacement of two positions is the IS2RS metric's (adf_eval_is2rs;
 *   scripts/eval.py:765-777 min_diff): fractional = (q - p) . inverse(cell of site a, a the earlier site of the pair), a
 *   float32 explicit inverse; % 1 twice; minus 1 where > 0.5; times the cell; its Euclidean norm.  In a strongly skewed
 *   cell this is the reference's convention and not the shortest lattice image.
 *   d_slab: the largest displacement over the atoms of tag != 2, atom k of a against atom k of b; 0 when include_slab == 0.
 *   d_ads, permutation_invariant == 0: the same over the atoms of tag 2.
 *   d_ads, permutation_invariant == 1: the symmetric per-element Hausdorff distance of the two adsorbates: the largest,
 *     over the adsorbate atoms of a, of the least displacement to an adsorbate atom of b of the same atomic number, and
 *     the same with a and b exchanged; the larger of the two.  A flipped N2 is at distance 0 from itself; the value equals
 *     the ordered one whenever that is below half the shortest same-element separation.
 *   An adsorbate without atoms has d_ads = 0.  d = +inf when the two sites differ in atom count or anywhere in the ordered
 *   tags or atomic numbers (so also in adsorbate size).  A non-finite coordinate gives NaN, which is within no tolerance.
 *   One wave per pair i < j, lanes over atoms, mirrored to (j, i). */
int32_t adf_site_pair_distances(const float* pos, const float* cell, const int32_t* tags, const int32_t* atomic_numbers,
                                const int32_t* atom_offset, const int32_t* group_offset, const int64_t* pair_offset,
                                int32_t num_atoms, int32_t num_sites, int32_t num_groups, int64_t out_len,
                                int32_t include_slab, int32_t permutation_invariant, float* out, void* stream);
/* Greedy clustering of each group on the matrices of adf_site_pair_distances (dist, dist_len elements).  A site is valid
 * when its four flags (flags [S,4], NULL: no filter) are 0 and its energy (energy [S], NULL: none) is not NaN.  An invalid
 * site gets rep = -1; it is never a representative and nothing is merged into it.  Valid sites are visited in the order
 * (energy ascending, position in the group); without energies in the order of position.  A visited site s joins the first
 * representative r, in visiting order, with dist(s,r) <= tol and, when energy_tol >= 0 and energies are given,
 * |E_s - E_r| <= energy_tol (the difference is taken in double); rep[s] = r, an index into the site arrays.  Without
 * such a representative s becomes one: rep[s] = s.  n_unique[g]: representatives of the group.  tol must be finite and
 * >= 0.  One workgroup per group, the sort inside it; a group may hold any number of sites. */
int32_t adf_unique_sites(const float* dist, const int32_t* group_offset, const int64_t* pair_offset, int32_t num_sites,
                         int32_t num_groups, int64_t dist_len, const float* energy, const int32_t* flags, float tol,
                         float energy_tol, int32_t* rep, int32_t* n_unique, void* stream);
/* The k valid sites of least energy per group, ascending, ties to the lower index (validity as adf_select_best_sites);
 * with rep (may be NULL) only representatives, rep[s] == s.  top [G,k]: indices into `energy`, -1 where the group has
 * fewer; top_energy [G,k]: their energies, +inf there.  Column 0 with rep == NULL is adf_select_best_sites' answer. */
int32_t adf_select_top_sites(const float* energy, const int32_t* flags, const int32_t* rep, const int32_t* group_offset,
                             int32_t num_groups, int32_t k, int32_t* top, float* top_energy, void* stream);

/* ---- Slab symmetry (csrc/symmetry.hip, csrc/unique.hip; adsorbdiff_amd/slab_symmetry.py).  An extension: the
 * reference has no counterpart (it leaves symmetry reduction to pymatgen's site finder, placement/adsorbate_slab_config.py:
 * 113-116); neither pymatgen nor spglib was run against this contract, it stands alone and is checked against
 * crystallography.  Slabs are bare: atoms atom_offset[b] .. atom_offset[b+1] of pos [N,3] float32 / atomic_numbers, cell
 * [B,9] float32 with rows = lattice vectors; rows 0 and 1 span the surface plane.  All arithmetic is double, outputs are
 * written with plain stores, there are no float atomics and two calls give the same bits.
 *
 * Operation: x -> R x + tau with the permutation perm it induces on the slab's atoms.  R n = n for the surface normal
 * n = cell[0] x cell[1] / |.| (rotations about n, mirrors containing n; nothing that turns the slab over), R maps the
 * in-plane lattice onto itself, tau lies in the plane.
 *   Point operations.  (1) Lagrange-reduce the in-plane basis A = [a b]: A_r = A U, U integer unimodular.  (2) Enumerate the
 *   2 x 2 integer matrices W_r with entries in {-1, 0, 1} and determinant +-1 (proper_only: +1).  (3) Accept W_r when the
 *   lengths of the images of a_r, b_r and a_r + b_r (the columns of A_r W_r and their sum) each differ from the originals
 *   by at most symprec.  (4) W = U W_r U^-1, integer.  (5) R = M [W 0; 0 1] M^-1, M = [a b n] as columns: the lattice goes
 *   exactly onto itself even where the float32 cell is symmetric only to rounding.  At most 12 per slab.
 *   Translations.  i0: the first atom of the rarest atomic number (ties to the smaller number).  For every atom j of that
 *   element the candidate is tau_j = x_j - R x_i0.
 *   Acceptance.  (W, j) is an operation when every atom i has an atom k of its atomic number with
 *   |reduce(R x_i + tau - x_k)| <= symprec and no k is taken twice; perm[i] = that k (the nearest, ties to the lower
 *   index).  reduce: the two in-plane fractional components through M^-1 minus their nearest integer (ties to even), the
 *   component along n as it is (no wrap along the normal), then the Euclidean norm of M times that.  Below half the
 *   shortest in-plane lattice height, area / max(|a|, |b|), that is the true nearest image in any cell; a symprec at or
 *   above it (or a cell whose first two rows span no finite area) is refused: ADF_EINVAL.  No convention quirk as in
 *   adf_site_pair_distances.
 *   Order.  Operation 0 is the identity, stored as R = I, tau = 0, perm = iota exactly; then the other accepted candidates
 *   in ascending (W00, W01, W10, W11, j).  A slab without atoms has no operation.
 *
 * adf_slab_symmetry_search verifies every candidate (slab, 12 point slots, atom j) - one flag word each in `scratch`, slots
 * without a point operation and atoms of another element are rejected - and counts: n_ops [2B] on the device, the counts
 * followed by the slabs' atom counts n_b, copied into n_ops_host [2B] (host memory) before it returns: the one read-back,
 * after which the caller sizes the outputs.
 * `scratch`: adf_slab_symmetry_scratch(num_atoms, num_slabs) bytes of device memory, handed on unchanged to
 * adf_slab_symmetry_emit with the same atom_offset / symprec.  That writes, for op_offset [B+1] = exclusive sum of n_ops
 * and perm_offset [B+1] (int64) = exclusive sum of n_ops[b] n_b: rot [K,9] and trans [K,3] double, W [K,4] int32 and perm
 * (perm_len int32; operation k of slab b owns perm[perm_offset[b] + k n_b ..+ n_b)). */
int64_t adf_slab_symmetry_scratch(int32_t num_atoms, int32_t num_slabs);
int32_t adf_slab_symmetry_search(const float* pos, const float* cell, const int32_t* atomic_numbers,
                                 const int32_t* atom_offset, int32_t num_atoms, int32_t num_slabs, double symprec,
                                 int32_t proper_only, void* scratch, int32_t* n_ops, int32_t* n_ops_host, void* stream);
int32_t adf_slab_symmetry_emit(const int32_t* atom_offset, int32_t num_atoms, int32_t num_slabs, double symprec,
                               const void* scratch, const int32_t* op_offset, const int64_t* perm_offset, int32_t num_ops,
                               int64_t perm_len, double* rot, double* trans, int32_t* W, int32_t* perm, void* stream);
/* adf_site_pair_distances up to a symmetry of the slab.  The arguments of adf_site_pair_distances, and per group g the
 * operations op_offset[g] .. op_offset[g+1] of rot / trans (num_ops of them) with their permutations at perm_offset[g]
 * (as adf_slab_symmetry_emit writes them; n_b = the group's entries / its operations).  For i < j
 *   d_sym(i,j) = min over the group's operations g of d(g . site_i, site_j),
 * d exactly adf_site_pair_distances' max(d_ads, d_slab) in its min_diff convention with the cell of the earlier site i.
 * g . site_i: every position is R x + tau, formed in double and rounded to float32 once; the k-th atom of tag != 2 of
 * site i is compared with the perm[k]-th atom of tag != 2 of site j; the adsorbate goes through the ordered or the
 * per-element Hausdorff rule.  Operation 0 of a group is the identity and is not applied, so a group with that one
 * operation gets the bits of adf_site_pair_distances.  The value goes to (i,j) and (j,i); best_op (int32, laid out as out)
 * gets the index within the group of the minimising operation at both, ties to the lowest index - its direction is always
 * "earlier site onto later site"; 0 on the diagonal and where d is +inf or NaN.  d = +inf also when the number of tag != 2
 * atoms of the sites differs from n_b, when a group has no operation, and when the atoms of tag 2 of a site are not one
 * contiguous block (place_adsorbates writes them after the slab).  Per operation d_ads is evaluated first and the slab part
 * is skipped when d_ads >= the best d so far: such an operation cannot win (an exact saving). */
int32_t adf_site_pair_distances_sym(const float* pos, const float* cell, const int32_t* tags, const int32_t* atomic_numbers,
                                    const int32_t* atom_offset, const int32_t* group_offset, const int64_t* pair_offset,
                                    int32_t num_atoms, int32_t num_sites, int32_t num_groups, int64_t out_len,
                                    int32_t include_slab, int32_t permutation_invariant, const int32_t* op_offset,
                                    const double* rot, const double* trans, const int32_t* perm, const int64_t* perm_offset,
                                    int32_t num_ops, int64_t perm_len, float* out, int32_t* best_op, void* stream);

/* ---- Adsorbate placement (csrc/placement.hip; adsorbdiff_amd/placement.py): the reference's
 * AdsorbateSlabConfig, placement/adsorbate_slab_config.py:99-439, 460-575 with adsorbate.py:122-169, modes "random"
 * [mode 0] and "random_site_heuristic_placement" [mode 1], for a whole batch of slabs.  This is a written contract, a
 * reading of those lines and of the ASE calls they make [Atoms.rotate, Atoms.wrap, get_center_of_mass]; ASE was not run
 * against it: parity with ASE is unpinned.  Inputs and outputs are float32 unless stated, all arithmetic is float64, no
 * float atomics, every output is bit-reproducible.
 *
 * Draw rows [double, 8 per row, uniforms in the open unit interval]: (r1, r2, selection key, u0, u1, u2, binding pick,
 * spare).  adf_place_draws fills row i from (seed, keys[i], index[i]) alone: Philox4x32-10 as adf_noise_draws, counters
 * (key lo, key hi, index, j), j = 2 for the first four words and j = 3 for the last four, u = (w + 0.5) 2^-32. */
int32_t adf_place_draws(int64_t seed, const int64_t* keys, const int32_t* index, int32_t n, double* out, void* stream);
/* P placements in one launch.  Placement p belongs to slab slab_of[p] of `slabs` [pos, cell, atomic_numbers, atom_offset;
 * reps unused], sits on site[p] [P,3] and reads u0, u1, u2 of draws row p [P,8].  Adsorbates are CSR over the slabs:
 * atoms ads_offset[b] .. ads_offset[b+1] of ads_pos / ads_Z.  radii [num_radii] and masses [num_masses] are indexed by
 * atomic number; pbc [B,3] int32: the periodic directions of each slab.  Per placement:
 *   Rotation.  A one-atom adsorbate is not rotated and reports zeros.  Otherwise zrot = 360 u0 degrees, phi = 2 pi u2,
 *     z = -1 + 2 u1 [mode 0] or cos[pi/9] + (1 - cos[pi/9]) u1 [mode 1], rotvec = (sqrt(1 - z^2) cos phi,
 *     sqrt(1 - z^2) sin phi, z).  First the counter-clockwise rotation by zrot about +z, then the Rodrigues rotation that
 *     takes +z to rotvec: axis z_hat x rotvec normalised, cos = z, sin = |z_hat x rotvec|; below 1e-7 the axis is
 *     x_hat x rotvec normalised [ASE's fallback as we read it].  Both about the centre C: the mass-weighted centre
 *     [masses of ads_Z] in mode 0, atom binding_idx[p] in mode 1.
 *   Translation so that C sits on the site.  Normal n = cell[0] x cell[1] normalised, its sign not fixed.
 *   Height.  Every slab atom is moved by (cell centre - site), cell centre = 0.5 (a + b + c), and wrapped into the cell along
 *     the periodic directions by ASE's rule, fractional f -> (f + 1e-7) mod 1 - 1e-7; the adsorbate is moved by the same
 *     vector.  Only this one image of each slab atom is looked at, as in the reference.  For each pair (adsorbate atom a,
 *     slab atom s of any tag): w = s - a, h = w . n, q = |w - h n|, D = radii[Z_a] + radii[Z_s] + interstitial_gap.  The
 *     pair counts when q <= D, with x_pair = h + sqrt(D^2 - q^2).  scaled_normal = max x_pair; without a counted pair it is
 *     0 and n_combos = 0 [the reference's "scary edge case": the adsorbate stays on the site].
 *     A deliberate reading: the reference solves each pair with fsolve started at 3 (R_a + R_s), which reaches the upper
 *     root whenever the slab atom lies less than that far above the adsorbate atom along n; this contract takes the
 *     upper root always.
 * Outputs: rows out_row[p] .. out_row[p] + n_a of out_pos [out_rows,3] receive rotated + translation + scaled_normal n,
 * in the slab's original frame [the caller points out_pos at the collated batch: out_row[p] is where the adsorbate of
 * system p begins]; scaled_normal double [P]; n_combos int32 [P]; rot_meta double [P,4] = (zrot, rotvec).
 * mode 1 needs binding_idx [P]; interstitial_gap must lie in [0, 5).  An atomic number outside either table, a
 * binding_idx outside its adsorbate or an offset out of range returns ADF_EINVAL, reported like adf_flag_anomalies
 * reports one: the call synchronises `stream` to read the error word. */
int32_t adf_place_adsorbates(const adf_batch* slabs, const int32_t* slab_of, const float* site, const double* draws,
                             const int32_t* ads_offset, const float* ads_pos, const int32_t* ads_Z, const float* radii,
                             int32_t num_radii, const float* masses, int32_t num_masses, float interstitial_gap,
                             int32_t mode, const int32_t* binding_idx, const int32_t* pbc, int32_t P,
                             const int32_t* out_row, int64_t out_rows, float* out_pos, double* scaled_normal,
                             int32_t* n_combos, double* rot_meta, void* stream);
/* Candidate sites [get_binding_sites, :144-164].  Slab b has triangles tri_offset[b] .. tri_offset[b+1] of tri [T,3,3]
 * and candidates cand_offset[b] .. cand_offset[b+1], per_tri[b] = ceil(2 num_sites / T_b) per triangle in triangle order
 * [equal counts per triangle, not area-uniform: the reference's scheme]; cand_slab[c] is the slab of candidate c.
 * Candidate c reads r1, r2 of draws row c: (1 - sqrt(r1)) v0 + sqrt(r1) (1 - r2) v1 + sqrt(r1) r2 v2.  keep[c] = 1 when
 * its fractional coordinates along a and b lie in [-1e-7, 1 - 1e-7), that is when ASE's wrap with pbc = (T, T, F) leaves
 * it where it is [the reference's isclose of unwrapped and wrapped]. */
int32_t adf_place_site_candidates(const float* tri, const int32_t* tri_offset, const int32_t* per_tri,
                                  const int32_t* cand_offset, const int32_t* cand_slab, const float* cell,
                                  const double* draws, int32_t B, int32_t num_candidates, float* cand, int32_t* keep,
                                  void* stream);
/* get_interstitial_distances / there_is_overlap [:511-575] per system of any adsorbate + slab batch: the system is
 * translated so that the mass centre of the adsorbate [tag 2] is on the cell centre, every atom is wrapped as above, and
 * out[b] = min over (surface atom s of tag 1, adsorbate atom a) of |p_a - p_s| - R_a - R_s [float32; +inf for a system
 * without such a pair].  Errors as adf_place_adsorbates. */
int32_t adf_interstitial_distances(const adf_batch* b, const int32_t* tags, const float* radii, int32_t num_radii,
                                   const float* masses, int32_t num_masses, const int32_t* pbc, float* out, void* stream);

/* ---- Heuristic adsorption sites (csrc/sites.hip; adsorbdiff_amd/placement.py: heuristic_sites, reduce_sites; DESIGN.md
 * 4k): the site list of the reference's mode "heuristic" [placement/adsorbate_slab_config.py:113-116, 185-194], which it
 * takes from pymatgen's AdsorbateSiteFinder.  pymatgen was not run against this: it is a written contract, parity with
 * pymatgen is unpinned, and it is checked against crystallographic known answers and a float64 oracle.  Inputs are float32,
 * all arithmetic is float64, there are no float atomics and two calls give the same bits.
 *
 * Frame of slab b: M = [a b n] as columns, a = cell[b][0], b = cell[b][1], n = a x b / |a x b| [sign as it comes]; a cell
 * whose first two rows span no finite area is refused.
 *   put inside:  f = M^-1 x, f_k -> (f_k + 1e-7) - floor(f_k + 1e-7) - 1e-7 for k = 0, 1 [the wrap rule of
 *     adf_place_adsorbates], the component along n kept, x = M f.  [With cell[2] parallel to n this is that rule on the
 *     cell's own fractional coordinates; with a tilted cell[2] it may pick another lattice image.]
 *   d(x, y) = |reduce(x - y)|, reduce as in the slab symmetry section: the two in-plane components of M^-1 (x - y) minus
 *     their nearest integer [ties to even], the normal component as it is, the norm of M times that.  In a strongly skewed
 *     cell this is not the shortest image [the caveat of adf_site_pair_distances and adf_slab_symmetry_search]: two
 *     sites closer than tol through another image are then both kept.
 *
 * adf_surface_site_candidates.  Slab b has atoms atom_offset[b] .. atom_offset[b+1] of pos [N,3] / tags [N] and triangles
 * tri_offset[b] .. tri_offset[b+1] of tri [T,3,3] [as adf_place_site_candidates takes them].  Its candidates, kind-major:
 *   ontop   n_top[b] of them: its atoms of tag 1, in atom order;
 *   bridge  3 T_b: per triangle, in table order, the midpoints 0.5 (v1 + v2), 0.5 (v0 + v2), 0.5 (v0 + v1) - every edge
 *           listed by the corner opposite to it;
 *   hollow  T_b: per triangle (v0 + v1 + v2) / 3.  The slot is INVALID [valid = 0; it stays in the layout] when the
 *           triangle is "obtuse": at some corner the cosine between the two normalised edge vectors leaving it is not
 *           >= 1e-5 [pymatgen's no_obtuse_hollow as we read it].  A right triangle therefore counts as obtuse - the
 *           four-fold hollow of fcc(100) appears as the bridge site of the diagonal, a quirk that is kept - and so does a
 *           triangle with an edge of no length [its cosine is NaN].
 * Every candidate is put inside and stored as float32.  seg_offset [3 B + 1] is WRITTEN here, on the device, from the tag-1
 * counts and the triangle counts: segment 3 b + kind holds rows seg_offset[3 b + kind] .. seg_offset[3 b + kind + 1] of
 * cand [capacity,3] / valid [capacity]; seg_offset[3 B] = sum_b n_top[b] + 4 T.  capacity: rows of the two tables,
 * N + 4 T always suffices [rows past seg_offset[3 B] are not written].  Offsets that are not ascending or leave their
 * arrays, and tables too small, return ADF_EINVAL: no candidate is written, seg_offset holds nothing of use, nothing is
 * read or written past an array, and the call synchronises `stream` to read the error word [as adf_place_adsorbates does]. */
int32_t adf_surface_site_candidates(const float* pos, const int32_t* tags, const int32_t* atom_offset, const float* cell,
                                    const float* tri, const int32_t* tri_offset, int32_t num_atoms, int32_t num_triangles,
                                    int32_t num_slabs, int32_t capacity, int32_t* seg_offset, float* cand, int32_t* valid,
                                    void* stream);
/* The reduction of any candidate table.  Segment g = rows seg_offset[g] .. seg_offset[g+1] of cand [C,3] belongs to slab
 * seg_slab[g] [NULL: slab g] of cell [B,9]; valid [C] may be NULL [all valid].  Per segment, greedy in candidate order: a
 * valid candidate c is kept if and only if no kept r < c of its segment has dist(c, r) <= tol.  Two passes:
 *   first   dist = d [the identity alone]: near-duplicates, the copies that tiling produces included.  first[c] = the
 *           index [into cand] of the kept candidate c fell to - the first kept one within tol -, c itself when kept;
 *   second  over the survivors of the first, dist(c, r) = d_sym(c, r) = min over the operations k of the slab of
 *           d(R_k x_c + tau_k, x_r), evaluated in exactly this form [the operation acts on the later candidate], the
 *           operations op_offset[b] .. op_offset[b+1] of rot [K,9] / trans [K,3] as adf_slab_symmetry_emit writes them.
 *           op_offset NULL: the identity alone, and the second pass keeps what the first kept.
 * rep[c]: the kept candidate of the second pass that first[c] fell to; first[c] = rep[c] = -1 for an invalid slot.
 * multiplicity[r], for a survivor of the second pass: the survivors of the first pass that fell to it, itself included -
 * its orbit size in the cell; 0 for every other row.  counts [G,2]: kept after the first pass, kept after both; 0 for an
 * empty segment or one with invalid slots only.  tol [A] must be finite and >= 0.  One workgroup per segment; candidates,
 * kept sites and operations may each be of any number.  A segment whose offsets are not ascending or leave [0, C], whose
 * slab is outside [0, B) or whose operations leave [0, K) is neither read nor written: ADF_EINVAL, reported as above. */
int32_t adf_reduce_sites(const float* cand, const int32_t* valid, const int32_t* seg_offset, const int32_t* seg_slab,
                         const float* cell, int32_t num_candidates, int32_t num_segments, int32_t num_slabs,
                         const int32_t* op_offset, const double* rot, const double* trans, int32_t num_ops, double tol,
                         int32_t* first, int32_t* rep, int32_t* multiplicity, int32_t* counts, void* stream);

/* ---- Surface triangles (csrc/triangulate.hip; adsorbdiff_amd/placement.py: surface_triangles_device): the
 * triangle tables that adf_place_site_candidates and adf_surface_site_candidates take, made on the device for a whole
 * batch - the reference's tiling and pruning [placement/adsorbate_slab_config.py:117-142, 479-508], which it and
 * placement.surface_triangles leave to scipy.spatial.Delaunay on the host.  For points in general position the Delaunay
 * triangulation is unique: there the table equals scipy's as a set, and that is pinned [tests/golden/surface_triangles.npz].
 * Inputs are float32, all arithmetic is float64, there are no float atomics, two calls give the same bits, and a slab's
 * rows depend neither on its batch-mates nor on its place in the batch.
 *
 * Slab b has atoms atom_offset[b] .. atom_offset[b+1] of pos [N,3] / tags [N] and the cell cell[b] [9, rows a, b, c].
 *   Tiling.  v0, v1: the first two rows v of the cell with |v_x| >= 0.0005 or |v_y| >= 0.05 [custom_tile_atoms' test
 *     round(v[0], 3) != 0 or round(v[1], 1) != 0 - placement.tiling_vectors - which it equals wherever the two components
 *     are not within 1e-6 of 0.0005 / 0.05].  The n_top atoms of tag 1, in atom order, are copied to 9 tiles in the order
 *     of surface_triangles: tile 0 is (0, 0), tiles 1 .. 8 are (i, j) for i in (-1, 0, 1), j in (-1, 0, 1) without (0, 0).
 *     Tiled point tile * n_top + ordinal is (p + i v0) + j v1 in float64 [the products are exact]; rounded once to float32
 *     it is a row of tri, equal bit for bit to the host path's .astype(float32).
 *   Triangles.  Of the Delaunay triangulation of the x, y of all 9 n_top points [the float64 values], those with at least
 *     one vertex in tile 0.  A triangle is (a, b, c), a its least tiled index, a -> b -> c counter-clockwise in x, y; a
 *     slab's rows are sorted ascending by (a, b, c).
 *   Co-circular points.  A point whose distance to a triangle's circumcentre differs from the radius by at most circle_tol
 *     [A] lies on the circle.  The points on one empty circle form one convex polygon, which is split as a fan from its
 *     canonical vertex: the one of least x, values of x within circle_tol of the least counting as equal and the least y
 *     [then the least index] deciding among those.  Every vertex of the polygon arrives at the same fan: the rectangles of
 *     an fcc(100) or fcc(110) surface are all split along parallel diagonals.  [With more than one point strictly inside
 *     the band circle_tol / 10 .. 10 circle_tol of a circle the rule may be applied differently from two sides; 1e-4 A is
 *     ten float32 roundings of a coordinate above, and far below any interatomic distance.]
 * Outputs, written on the device: tri_offset [B+1] - slab b owns rows tri_offset[b] .. tri_offset[b+1] -, tri
 * [capacity,3,3] the vertices and tri_index [capacity,3] their tiled indices.  capacity >= 18 N always suffices [a planar
 * triangulation of n points has fewer than 2 n triangles, n = 9 n_top]; rows past tri_offset[B] are not written.
 * ADF_EINVAL - reported as adf_surface_site_candidates reports one: the call synchronises `stream` to read an error word -
 * for a slab without an atom of tag 1, a cell with fewer than two such rows, tiled points that are all collinear [or
 * coincide, or whose tiling vectors are parallel in x, y so that the tiles do not surround tile 0], atom offsets that are
 * not ascending or leave [0, N], more triangles than capacity, and a circle_tol that is negative or not finite.  On an error
 * tri and tri_index are not written, tri_offset holds zeros, and nothing is read or written past an array.  n_top may be
 * any number; n_top = 1 gives the triangulation of the lattice itself. */
int32_t adf_surface_triangles(const float* pos, const int32_t* tags, const int32_t* atom_offset, const float* cell,
                              int32_t num_atoms, int32_t num_slabs, double circle_tol, int32_t capacity,
                              int32_t* tri_offset, float* tri, int32_t* tri_index, void* stream);

/* ---- Surface tags (csrc/voronoi.hip; adsorbdiff_amd/surface_tags.py): the tags that every entry point above
 * starts from - 1 for a surface atom, 0 for the rest -, made on the device for a whole batch: the reference's
 * tag_surface_atoms [placement/slab.py:284-482: find_surface_atoms_by_height, find_surface_atoms_with_voronoi_given_height,
 * calculate_coordination_of_bulk_atoms], whose coordination numbers are pymatgen's VoronoiNN(tol=0.1).get_cn(use_weights=
 * True), a qhull call per atom.  pymatgen was not run against it; the geometry is pinned to qhull [scipy.spatial.Voronoi on
 * the same points, tests/golden/voronoi_cn.npz].  Inputs are float32, ALL arithmetic is float64, there are no float atomics,
 * two calls give the same bits, and a system's rows depend neither on its batch-mates nor on its place in the batch.
 *
 * adf_voronoi_coordination.  System b has atoms atom_offset[b] .. atom_offset[b+1] of pos [N,3], the cell cell[b] [9, rows
 * a, b, c] and is periodic along row k where pbc[b][k] != 0.  select [N]: the atoms to evaluate [!= 0], NULL: all.
 *   Images.  With V = a . (b x c), the plane spacing along row k is |V| / |product of the other two rows|, and the repeats
 *     along a periodic row are r_k = ceil(cutoff / spacing_k) of that system alone [0 along a row that is not periodic].
 *     Image (i_a, i_b, i_c), |i_k| <= r_k, has the index ((i_a + r_a) (2 r_b + 1) + (i_b + r_b)) (2 r_c + 1) + (i_c + r_c)
 *     and the shift (i_a a + i_b b) + i_c c.  The points of atom i are d = (p_j + shift) - p_i over every atom j of its
 *     system and every image, with 1e-16 < |d|^2 and |d| <= cutoff [13.0 A is pymatgen's; the first excludes the atom
 *     itself].  They are the CANDIDATES, ordered by (|d|^2, atom index j, image index).
 *   Facet j.  On the bisector plane of (i, j) - the points x with x . d_j = |d_j|^2 / 2 - start from the square of half-width
 *     1e4 A about d_j / 2 with sides along u = normalised(n x e), v = n x u [n = d_j / |d_j|, e = x when |n_x| < 0.9, else
 *     y], and clip it in candidate order by every other candidate k [Sutherland-Hodgman; a vertex with
 *     s = x . d_k - |d_k|^2 / 2 <= 0 is kept, an edge whose ends differ in that gets the point at t = s_a / (s_a - s_b)].
 *     What is left, if it has three vertices or more, is the facet; omega_j is the solid angle it subtends at the atom, the
 *     absolute value of the sum over the fan (v_0, v_m, v_m+1) of Van Oosterom and Strackee's
 *     2 atan2(a . (b x c), |a||b||c| + (a . b)|c| + (a . c)|b| + (b . c)|a|); omega_j = 0 without a facet.
 *   Outputs per evaluated atom.  omega_max = max_j omega_j; w_j = omega_j / omega_max; nn = the number of j with
 *     w_j > weight_tol; cn = the sum of those w_j in candidate order [get_cn(use_weights=True) with tol = weight_tol].
 *   Open cells.  flags bit 0 is set when a vertex of a facet lies farther than `far` [100 A] from the atom - a cell its
 *     candidates do not close, pymatgen's "pathological" RuntimeError - and for an atom without a candidate.  Then cn and
 *     omega_max are NaN and nn is 0.
 *   Security radius.  A candidate farther than twice the largest vertex distance R of the cell built so far cannot cut it,
 *     and a clip that does not cut leaves the vertices as they are, bit for bit.  The kernel builds the cell from the K
 *     nearest candidates [K = 64, doubled while candidate K exists and is not farther than 2 R]: the outputs are those of
 *     clipping by all candidates.
 *   Capacities, never silently exceeded: 1024 candidates per atom, 32 vertices per facet while it is clipped, 2^24 (atom,
 *     image) pairs looked at per atom.  ADF_EOVERFLOW otherwise; the message names the first such atom.
 * ADF_EINVAL: atom offsets that are not ascending or leave [0, N]; a system with a periodic row whose cell is singular or
 * not finite; cutoff, weight_tol or far that are not finite or not positive.  Errors are reported as
 * adf_surface_site_candidates reports them: the call synchronises `stream` to read an error word.  On an error no output is
 * written and nothing is read or written past an array.  Rows of atoms that are not selected are never written. */
int32_t adf_voronoi_coordination(const float* pos, const float* cell, const int32_t* pbc, const int32_t* atom_offset,
                                 int32_t num_atoms, int32_t num_systems, const int32_t* select, double cutoff,
                                 double weight_tol, double far, double* cn, double* omega_max, int32_t* nn, int32_t* flags,
                                 void* stream);
/* table [B,119]: per system and atomic number the least cn over that element's atoms, in atom order, +inf where the system
 * has none [calculate_coordination_of_bulk_atoms, reduced to the minimum that the comparison uses; every atom is
 * evaluated, not one per symmetry class].  cn / flags [N] as adf_voronoi_coordination wrote them for all atoms.  ADF_EINVAL:
 * a flagged atom [a bulk is periodic in three directions and its cells close], a cn that is NaN, an atomic number outside
 * [0, 118], offsets as above; the table is then not written.  Fixed order, no atomics. */
int32_t adf_bulk_coordination_min(const double* cn, const int32_t* flags, const int32_t* atomic_numbers,
                                  const int32_t* atom_offset, int32_t num_atoms, int32_t num_systems, double* table,
                                  void* stream);
/* adf_tag_surface_atoms.  Every atom of system b is a slab atom [tags of the caller are not read].  Per system, in order:
 *   1. f_i = p_i . (a x b) / (c . (a x b)): the fractional coordinate along row c; where that row is periodic f -> f - floor(f),
 *      twice [ASE's get_scaled_positions].
 *   2. Height rule [slab.py:350-382]: tag 1 iff not (f_i < max_i f - height / |c|); height = 2.0 A there.
 *   3. Coordination rule [slab.py:385-437], only with bulk_cn_min [B,119; adf_bulk_coordination_min of the slabs' bulks,
 *      one row per slab]: f_com = sum(m_i f_i) / sum(m_i) in atom order, m = masses[Z_i] [119 doubles]; every atom of tag 0
 *      with not (f_i < f_com) is evaluated as adf_voronoi_coordination evaluates it and becomes tag 1 when its cell is open
 *      or cn < bulk_cn_min[b][Z_i] - cn_tol.
 * Two deviations from the reference.  It takes the centre-of-mass test on pymatgen's unwrapped fractional coordinates:
 * here the one wrapped f serves both rules [they differ only for atoms outside the cell along c].  It compares
 * round(cn, 5) < min: with float32 positions a fully coordinated fcc atom comes out at 11.999995, on that knife; here the
 * comparison is cn < min - cn_tol, cn_tol = 1e-3 by default [>= 0].
 * Outputs: tags [N] 0 / 1; cn [N] and flags [N] of the evaluated atoms, NaN and 0 for the others.  ADF_EINVAL besides
 * adf_voronoi_coordination's: a singular or non-finite cell [any system], height or cn_tol negative or not finite, a mass
 * sum that is not positive, an atomic number outside [0, 118], and - with bulk_cn_min - an atom whose element is absent
 * [+inf or NaN] from its slab's row.  ADF_EOVERFLOW as above.  On an error no output is written. */
int32_t adf_tag_surface_atoms(const float* pos, const float* cell, const int32_t* pbc, const int32_t* atomic_numbers,
                              const int32_t* atom_offset, int32_t num_atoms, int32_t num_systems, const double* masses,
                              const double* bulk_cn_min, double height, double cutoff, double weight_tol, double far,
                              double cn_tol, int32_t* tags, double* cn, int32_t* flags, void* stream);

/* Multi-GPU exchange of the sharded sampler: systems are independent, every rank samples its shard
 * with no data-path collective, and ONE all-gather of the sampled adsorbate sites ends a pass.  Replaces the reference's
 * per-rank .npz + barrier + rank-0 merge (trainers/sde_denoising_trainer.py:862-909).  RCCL is loaded lazily (dlopen).
 *   adf_comm_unique_id   rank 0 draws a 128-byte id (ncclGetUniqueId) and hands it to the other ranks out of band
 *                        (adsorbdiff_amd/sampler.py broadcasts it through torch.distributed);
 *   adf_comm_create      collective over all ranks: one communicator per rank on the current device;
 *   adf_allgather_sites  out[r*bytes_per_rank ..] = rank r's `local`; device pointers, enqueued on `stream`;
 *                        every rank passes the same (padded) bytes_per_rank. */
#define ADF_COMM_ID_BYTES 128
typedef struct adf_comm* adf_comm_t;
int32_t adf_comm_unique_id(uint8_t* out128);
int32_t adf_comm_create(const uint8_t* id128, int32_t rank, int32_t world, adf_comm_t* out);
int32_t adf_comm_destroy(adf_comm_t comm);
int32_t adf_allgather_sites(adf_comm_t comm, const void* local, int64_t bytes_per_rank, void* out, void* stream);

/* ---- Training step (score matching; SURVEY.md 8f-1, BASELINE config 5).  Device ops that adsorbdiff_amd/train_step.py
 * strings together into forward-with-saved-activations, loss and backward of the PaiNN denoiser; they replace
 * torch.autograd through models/painn/painn_denoising.py + DenoisingTrainer._compute_loss
 * (trainers/sde_denoising_trainer.py:675-728) and torch.optim.AdamW + clip_grad_norm_ + the EMA update
 * (trainers/base_trainer.py:787-820).  Exact f32.  All pointers are device pointers; ld* are row strides in floats;
 * "acc" flags select accumulate-into instead of overwrite.  The graph ops use the handle's current graph. */
int32_t adf_op_linear_fwd(const float* A, int32_t lda, const float* W, const float* bias, float* C, int32_t ldc, int64_t M,
                          int32_t N, int32_t K, void* stream);
int64_t adf_op_linear_bwd_scratch(int64_t M, int32_t N, int32_t K); /* floats of scratch adf_op_linear_bwd needs */
int32_t adf_op_linear_bwd(const float* A, int32_t lda, const float* W, const float* dC, int32_t ldc, float* dA, int32_t ldda,
                          int32_t acc_dA, float* dW, float* db, int32_t acc_dW, int64_t M, int32_t N, int32_t K,
                          float* scratch, void* stream);
int32_t adf_op_ssilu_fwd(const float* h, float* y, int64_t n, void* stream);
int32_t adf_op_ssilu_bwd(const float* h, const float* dy, float* dh, int64_t n, void* stream);
int32_t adf_op_layernorm_fwd(const float* x, const float* w, const float* b, float* y, float* stats, int32_t N, int32_t H,
                             void* stream);
/* dx is accumulated into; dw, db [H] are written; scratch: 512 * 2 * H floats. */
int32_t adf_op_layernorm_bwd(const float* x, const float* w, const float* stats, const float* dy, float* dx, float* dw,
                             float* db, int32_t N, int32_t H, float* scratch, void* stream);
int32_t adf_op_embed_fwd(adf_painn_t h, const int32_t* Z, int32_t N, float* x, void* stream);
int32_t adf_op_embed_bwd(const float* dx, const int32_t* Z, float* demb, int32_t N, int32_t H, void* stream);
int32_t adf_op_rbf(adf_painn_t h, float* rbf, void* stream);
int32_t adf_op_message_fwd(adf_painn_t h, const float* xh, const float* vec, const float* rbfh, const float* x, float* x1,
                           float* vec1, int32_t vec_is_zero, void* stream);
/* The same forward through the sampler's fused message kernel (no [E,3H] operand: the radial-basis projection runs inside the
 * kernel on the matrix cores, painn_denoising.py:530-567); the layer's rbf_proj images are rebuilt from the bound weight
 * tensors first (the optimizer updates them in place).  Outputs agree with adf_op_message_fwd to ~1e-6 relative. */
int32_t adf_op_message_fwd_fused(adf_painn_t h, int32_t layer, const float* xh, const float* vec, const float* x, float* x1,
                                 float* vec1, int32_t vec_is_zero, void* stream);
int32_t adf_op_message_bwd(adf_painn_t h, const float* xh, const float* vec, const float* rbfh, const float* gx1,
                           const float* gv1, float* dxh, float* drbfh, float* dvec, float* dx, int32_t vec_is_zero,
                           void* stream);
/* The same backward with rbfh REGENERATED inside the kernel on the matrix cores (message_bwd.hip; autograd through
 * painn_denoising.py:530-567): no [E,3H] operand is kept from the forward or recomputed by a dense product.  drbfh is written
 * ([num_edges + 1, 3H]: one spare row that the kernel's padded edge rows write) with its 3H columns in the kernel's own
 * order; adf_op_message_bwd_perm fills perm[c'] = the column of rbf_proj's output
 * that kernel-order column c' holds (host array of 3H entries), so that the weight-gradient product of rbf_proj can run on it
 * and its rows be permuted back.  Needs the f16x3 arithmetic and equally spaced Gaussian centres
 * (adf_op_message_bwd_fused_supported returns 1) and the layer's rbf_proj images of this step (adf_op_message_fwd_fused
 * builds them).  Gradients agree with adf_op_message_bwd to ~1e-6 relative. */
int32_t adf_op_message_bwd_fused_supported(adf_painn_t h);
int32_t adf_op_message_bwd_perm(adf_painn_t h, int32_t* perm_host, int32_t n);
int32_t adf_op_message_bwd_fused(adf_painn_t h, int32_t layer, const float* xh, const float* vec, const float* gx1,
                                 const float* gv1, float* dxh, float* drbfh_lane_order, int64_t num_edges, float* dvec,
                                 float* dx, int32_t vec_is_zero, float* dbias_rows, void* stream);
/* The default since round 5: d(rbfh) never reaches memory.  adf_op_message_bwd_fused is called with drbfh_lane_order = NULL and
 * dbias_rows = [N, 3H] (it then writes, per atom, the column sums of the atom's d(rbfh) rows - the bias gradient of rbf_proj is
 * their sum over the atoms - and leaves the packed gradient records of the layer in the handle); adf_op_rbf_wgrad_fused then
 * ACCUMULATES dW [3H, R] of the layer's rbf_proj (reference row order), forming d(rbfh) again from those records, xh / vec
 * of the owning atom and the edge geometry while it stages the product (three-term bf16 split, six products, as
 * adf_op_linear_bwd's weight-gradient kernel).  edge_owner [num_edges] = the atom whose CSR segment holds an edge row
 * (adf_op_edge_owner, once per graph); rbf_image: adf_op_rbf_image; scratch: adf_op_rbf_wgrad_fused_scratch(h) floats.
 * Replaces autograd's dW = d(rbfh)^T edge_rbf for models/painn/painn_denoising.py:530-567 (PaiNNMessage.rbf_proj). */
int32_t adf_op_edge_owner(adf_painn_t h, int32_t* edge_owner, int64_t num_edges, void* stream);
/* the radial basis [num_edges, num_rbf] (adf_op_rbf) as the three bf16 terms of the product in the kernel's own layout, once per
 * step (it does not depend on the layer); `image`: adf_op_rbf_image_bytes(num_edges) bytes */
int64_t adf_op_rbf_image_bytes(int64_t num_edges);
int32_t adf_op_rbf_image(adf_painn_t h, const float* rbf, int64_t num_edges, void* image, void* stream);
int64_t adf_op_rbf_wgrad_fused_scratch(adf_painn_t h);
int32_t adf_op_rbf_wgrad_fused(adf_painn_t h, const float* xh, const float* vec, const void* rbf_image, const int32_t* edge_owner,
                               int64_t num_edges, float* dW, float* scratch, int32_t vec_is_zero, void* stream);
int32_t adf_op_vdot_fwd(const float* vv, float* dot, float* nrm, int32_t ldn, int64_t N, int32_t C, float eps, void* stream);
int32_t adf_op_vdot_bwd(const float* vv, const float* nrm, int32_t ldn, const float* ddot, const float* dnrm, int32_t lddn,
                        const float* dv1, float* dvv, int64_t N, int32_t C, void* stream);
int32_t adf_op_update_out_fwd(const float* x1, const float* vec1, const float* a, const float* dot, const float* vv, float s,
                              float* x2, float* vec2, int64_t N, int32_t H, void* stream);
int32_t adf_op_update_out_bwd(const float* a, const float* dot, const float* vv, float s, const float* dx2,
                              const float* dvec2, float* da, float* ddot, float* dv1, float* dx1, float* dvec1, int64_t N,
                              int32_t H, void* stream);
int32_t adf_op_vnorm_fwd(const float* t1, float* nrm, int32_t ldn, int64_t N, int32_t C, void* stream);
int32_t adf_op_vnorm_bwd(const float* t1, const float* nrm, int32_t ldn, const float* dnrm, int32_t lddn, float* dt1,
                         int64_t N, int32_t C, void* stream);
int32_t adf_op_gate_fwd(const float* o, const float* t2, float* xs, int32_t ldx, float* vout, int64_t N, int32_t C,
                        void* stream);
int32_t adf_op_gate_bwd(const float* o, const float* t2, const float* dxs, int32_t lddx, const float* dvout, float* d_o,
                        float* dt2, int64_t N, int32_t C, void* stream);
int32_t adf_op_copy_rows(const float* src, int32_t lds_, float* dst, int32_t ldd, int64_t M, int32_t C, int32_t accumulate,
                         void* stream);
int32_t adf_op_score_loss(const float* f1, const float* f2, const int32_t* tags, const int32_t* atom_offset,
                          const float* tr_sigma, const float* rot_sigma, const float* tr_score, const float* rot_score,
                          const float* rot_norm, float* loss, float* df1, float* df2, int32_t B, float* scratch, void* stream);
/* The same objective without so3_denoising (sde_denoising_trainer.py:675-701, the one-head model the translation-only
 * samplers run): L = mean_{b,k} (mean_ads(f1) / sigma - s)^2 sigma^2 with the z component of the prediction zeroed;
 * loss [3] = (L, L, 0); df1 [N,3] is written for all rows (zero off the adsorbate).  One wave per system, sums in a fixed
 * order; scratch: B floats. */
int32_t adf_op_score_loss_tr(const float* f1, const int32_t* tags, const int32_t* atom_offset, const float* tr_sigma,
                             const float* tr_score, float* loss, float* df1, int32_t B, float* scratch, void* stream);

/* ---- Forward noising of a training batch on the device (csrc/noising.hip; adsorbdiff_amd/noising.py DeviceNoiser).
 * Counter-based draws: row b of out (double [B,8]) depends on (seed, step, keys[b]) alone.  Philox4x32-10 with key
 * (seed lo, seed hi) and counters (key lo, key hi, step, j), j = 0, 1; a word w becomes u = (w + 0.5) 2^-32; the words of
 * j = 0 are (u_t, u_om, a0, a1), of j = 1 (a2, a3, a4, a5); Box-Muller in double on (a0,a1), (a2,a3), (a4,a5):
 * r = sqrt(-2 ln a_2p), n_2p = r cos(2 pi a_2p+1), n_2p+1 = r sin(2 pi a_2p+1).  Row = (u_t, n0..n5, u_om): n0..2 the COM
 * noise, n3..5 the rotation axis before normalisation. */
int32_t adf_noise_draws(int64_t seed, int32_t step, const int64_t* keys, int32_t B, double* out, void* stream);
/* The sampler's draws, keyed like the rows above: a system's rows depend on (seed, keys[b], site[b]) alone, so it is
 * sampled the same alone, in any batch, in any order and on any shard.  Philox4x32-10, key (seed lo, seed hi), counters
 * (key lo, key hi, t, 4 + 2 site + j), j = 0, 1 (last words 0..3 belong to adf_noise_draws and adf_place_draws).  site: the
 * number of the placement within its slab (NULL = 0), outside [0, 2^30) is ADF_EINVAL (read back once, synchronises).
 * Step row t in [0, T): words w0..w7 of j = 0, 1; Box-Muller in double on (w0,w1), (w2,w3), (w4,w5) as adf_noise_draws;
 * z_a[t,b] = float(n0, n1, n2), z_b[t,b] = float(n3, n4, n5).  Placement row: t = 0xFFFFFFFF, j = 0,
 * place[b,k] = (w_k >> 8) 2^-24, k = 0..2: in [0, 1), exact in float32.  Any of place [B,3], z_a, z_b [T,B,3] may be NULL.
 * Use: adf_sample with noise: z_tr_all = z_a, z_rot_all = z_b; Langevin: z_all = z_a. */
int32_t adf_sampler_draws(int64_t seed, const int64_t* keys, const int32_t* site, int32_t B, int32_t T, float* place,
                          float* z_a, float* z_b, void* stream);
/* tr_so3_schedule (sde_denoising_trainer.py:67-135 with pbc_correction :45-64 and rot_utils.py:18-98, 226-253) given one row
 * of draws per system: t = float(u_t), both sigmas in float32, the COM noise wrapped to its minimum image (fractional
 * solve in double), rot_update = axis / |axis| * omega(u_om) and its score by the table look-ups of rot_utils.py in
 * double (nearest eps row, np.interp), the quaternion rotation about the adsorbate's centre, the COM shift and the +1 A
 * lift.  The adsorbate is every atom of tag 2 in [atom_offset[b], atom_offset[b+1]).  pos_out [N,3] is a copy of pos with
 * the adsorbate rows replaced (pos_out != pos); tr_sigma, rot_sigma, rot_norm [B]; tr_score, rot_score, noise_vec [B,3];
 * rot_norm is exp_score_norm of the system's eps row (rot_utils.py:256-264), what the loss divides by.  Tables: device
 * double, omegas [n_omega], cdf and score [n_eps, n_omega], exp_score_norm [n_eps].  One wave per system, no atomics. */
int32_t adf_noise_tr_so3(const float* pos, const float* cell, const int32_t* tags, const int32_t* atom_offset, int32_t B,
                         int32_t N, const double* draws, float ads_std_low, float ads_std_high, float rot_std_low,
                         float rot_std_high, const double* omegas, const double* cdf, const double* score,
                         const double* exp_score_norm, int32_t n_eps, int32_t n_omega, float* pos_out, float* tr_sigma,
                         float* rot_sigma, float* tr_score, float* rot_score, float* noise_vec, float* rot_norm,
                         void* stream);
/* ads_COM_gaussian_schedule (sde_denoising_trainer.py:138-177) from (u_t, n0, n1) of the same rows: the noised centre is
 * wrapped into the cell as the samplers wrap it (float32 solve with cell, modulo 1 twice, back with cell . f; the COLUMNS
 * of cell act as lattice vectors), lifted by 1 A, and every adsorbate atom is set to it. */
int32_t adf_noise_com(const float* pos, const float* cell, const int32_t* tags, const int32_t* atom_offset, int32_t B,
                      int32_t N, const double* draws, float ads_std_low, float ads_std_high, float* pos_out,
                      float* tr_sigma, float* tr_score, float* noise_vec, void* stream);
/* rot_utils.score_norm (rot_utils.py:256-264) alone: out[b] = table[eps_index(rot_sigma[b])], table = exp_score_norm
 * [n_eps] on the device; for batches that arrive already noised. */
int32_t adf_igso3_score_norm(const float* rot_sigma, const double* table, int32_t n_eps, int32_t B, float* out, void* stream);
/* S2EF objective of the force field: OCPTrainer._compute_loss (trainers/ocp_trainer.py:308-356) with DDPLoss
 * (modules/loss.py:48-102) over nn.L1Loss for the energy ("mae") and L2MAELoss for the forces ("l2mae")
 * (utils/utils.py:1219-1260, 1319-1331); E_pred [B] / F_pred [N,3] are normalised predictions, E_tgt / F_tgt in target units:
 *     loss[1] = c_E W / B_glob  sum_b |E_pred[b] - (E_tgt[b] - mean_E) / std_E|
 *     loss[2] = c_F W / M_glob  sum_{i in S} ||F_pred[i] - (F_tgt[i] - mean_F) / std_F||_2,   loss[0] = loss[1] + loss[2]
 * S: the atoms with fixed == 0 when free_only (base_trainer.py:382-390), else all atoms; fixed == NULL: no atom is fixed.
 * counts: device {B_glob, M_glob, W} (int64; the all-reduced counts of a multi-rank step) or NULL: this call's own counts
 * and W = 1.  F_pred == NULL (a model without a force head): the energy term alone, dF untouched.  dE [B], dF [N,3]: the
 * gradient with respect to the predictions; zero at a zero residual (torch's subgradient of abs / norm) and outside S.
 * M_glob == 0 (no atom in S on any rank, or a supplied zero): the force term is 0 * W / 0 = NaN, as the reference's
 * loss * world_size / num_samples is, so loss[0] and loss[2] are NaN (a trainer skips such a step) and dF is NaN or zero.
 * metrics [2]: energy MAE and force MAE per component over the atoms with fixed == 0, both in target units
 * (_compute_metrics after denorm, ocp_trainer.py:358-402).  One wave per system, the systems combined in ascending order,
 * no float atomics: run-to-run identical, and a system's dE / dF rows depend on its own rows and the two divisors only.
 * scratch: adf_op_s2ef_loss_scratch(B) floats. */
int32_t adf_op_s2ef_loss(const float* E_pred, const float* F_pred, const float* E_tgt, const float* F_tgt,
                         const int32_t* fixed, const int32_t* atom_offset, int32_t B, int32_t free_only, float mean_E,
                         float std_E, float mean_F, float std_F, float c_E, float c_F, const int64_t* counts, float* loss,
                         float* dE, float* dF, float* metrics, float* scratch, void* stream);
int64_t adf_op_s2ef_loss_scratch(int32_t B);
/* energy[b] = sum over the system's atoms of (y[a] . w + bias), y [N, H2] the activated hidden layer of out_energy
 * (models/painn/painn.py:412-414): the fixed-order per-system sum of adf_painn_forward_energy. */
int32_t adf_op_energy_sum(const float* y, int32_t H2, const float* w, const float* bias, const int32_t* atom_offset,
                          float* energy, int32_t B, void* stream);
/* Backward of out_energy.2 (H2 -> 1), the per-system sum and the ScaledSiLU before it (painn.py:412-414) in one pass over
 * the stored pre-activation he0 [N, H2]:
 *     dhe0[n,c] = dE[sys(n)] w2[c] SSiLU'(he0[n,c]),   dW2[c] (+)= sum_n dE[sys(n)] SSiLU(he0[n,c]),   db2 (+)= sum_n dE[sys(n)]
 * atom_sys [N]: the atoms' system index.  dE == NULL: dE = 1 (the values adf_painn_forward_energy_gradient's own seed kernel
 * writes, from the same expression; that call does not go through this entry).  dW2 == db2 ==
 * NULL: data gradient only.  A workgroup owns 64 rows x 64 columns and writes one partial row; a second launch adds the
 * partial rows in a fixed order (16 contiguous groups of chunks, each ascending, then the groups): no float atomics.  scratch: adf_op_energy_head_bwd_scratch(N, H2) floats. */
int32_t adf_op_energy_head_bwd(const float* he0, const float* w2, const float* dE, const int32_t* atom_sys, float* dhe0,
                               float* dW2, float* db2, int32_t accumulate, int64_t N, int32_t H2, float* scratch,
                               void* stream);
int64_t adf_op_energy_head_bwd_scratch(int64_t N, int32_t H2);
int32_t adf_op_sqnorm_accumulate(const float* g, int64_t n, float* out, void* stream);
int32_t adf_op_adamw_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* sqnorm,
                          float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                          float ema_decay, void* stream);

/* ---- Reproducible optimizer step and embedding backward (csrc/optimizer.hip): no float atomics, every sum
 * in an order that depends on the data and on the chunk length L alone.
 * Tables (device memory, written by the host as int64 words): one row of 8 words per tensor
 *   { p, g, m, v, ema (pointers; g or ema may be 0), numel, weight-decay flag, 0 }
 * and one row of 2 words per chunk { tensor, offset }: every tensor is cut into chunks of L elements, the last one short.
 * State block (40 bytes): int64 applied, int64 skipped, int32 apply, float clip, bc1, bc2, ema_decay, sqnorm.
 * The chunk length L: */
int64_t adf_op_optimizer_chunk(void);
/* Squared gradient norm over all chunks (partials: nchunks floats, one ordinary store each; then one workgroup adds them in
 * index order in double) and the step's decision: apply = isfinite(sqnorm); if set, applied += 1, bc_k = 1 - beta_k^applied
 * in double, clip = min(1, max_norm / (sqrt(sqnorm) + 1e-6)) (max_norm <= 0: 1), ema_decay = min(ema_decay,
 * (1 + n) / (10 + n)) with n = ema_updates0 + applied (ema_updates0 < 0: ema_decay as given); else skipped += 1. */
int32_t adf_op_grad_sqnorm_multi(const void* tensors, const void* chunks, int32_t nchunks, float* partials, void* state,
                                 float max_norm, double beta1, double beta2, float ema_decay, int64_t ema_updates0,
                                 void* stream);
/* AdamW + clip + EMA over all chunks in one launch, reading apply / clip / bc1 / bc2 / ema_decay from the state block; the
 * element arithmetic is the one behind the per-tensor step above.  Tensors without a gradient are skipped. */
int32_t adf_op_adamw_multi(const void* tensors, const void* chunks, int32_t nchunks, const void* state, float lr, float beta1,
                           float beta2, float eps, float weight_decay, void* stream);
/* demb[Z[n]-1, :] += dx[n, :] (demb: [rows, H]) in segments of 64 atoms: per segment one partial row per element present
 * (atoms in index order), then per element the segments in index order.  Rows of absent elements are not written; Z outside
 * 1..rows contributes nothing.  scratch: the number of floats the _scratch entry returns. */
int32_t adf_op_embed_bwd_ordered(const float* dx, const int32_t* Z, float* demb, int32_t N, int32_t H, int32_t rows,
                                 float* scratch, void* stream);
int64_t adf_op_embed_bwd_ordered_scratch(int64_t N, int32_t H, int32_t rows);

/* ---- Evaluation metrics (csrc/evaluate.hip): modules/evaluator.py for the tasks "s2ef", "is2rs", "is2re", and the
 * per-batch loss of BaseTrainer.validate (trainers/base_trainer.py:712-785), accumulated on the device.
 * Accumulator: caller-owned device memory, double total[ADF_EVAL_SLOTS] and int64_t numel[ADF_EVAL_SLOTS], indexed by the
 * enum below (the reference's {"total", "numel"} of a metric; "metric" = total / numel is the reader's).  Every entry
 * ADDS into it and the caller zeroes it, so a pass over many batches needs no device-to-host read.  One accumulator per
 * Evaluator: "s2ef" and "is2re" both write ADF_EVAL_ENERGY_MAE.
 * One wave per system writes the system's partial sums in a fixed lane order, one thread adds the systems in ascending order
 * and adds into the accumulator; no float atomics, run-to-run bit-identical.  Every per-element term is formed in float32
 * with separately rounded operations, as the reference's float32 tensors form it; every sum is carried in float64.
 * scratch: adf_eval_scratch(B) doubles. */
enum {
    ADF_EVAL_ENERGY_MAE = 0,
    ADF_EVAL_FORCESX_MAE = 1,
    ADF_EVAL_FORCESY_MAE = 2,
    ADF_EVAL_FORCESZ_MAE = 3,
    ADF_EVAL_FORCES_MAE = 4,
    ADF_EVAL_FORCES_COSINE_SIMILARITY = 5,
    ADF_EVAL_FORCES_MAGNITUDE_ERROR = 6,
    ADF_EVAL_ENERGY_FORCES_WITHIN_THRESHOLD = 7,
    ADF_EVAL_POSITIONS_AVERAGE_DISTANCE_WITHIN_THRESHOLD = 8,
    ADF_EVAL_POSITIONS_MAE = 9,
    ADF_EVAL_POSITIONS_MSE = 10,
    ADF_EVAL_ENERGY_MSE = 11,
    ADF_EVAL_ENERGY_WITHIN_THRESHOLD = 12,
    ADF_EVAL_LOSS = 13,
    ADF_EVAL_SLOTS = 14
};
int64_t adf_eval_scratch(int32_t B);
/* Evaluator.task_metrics["s2ef"] as OCPTrainer._compute_metrics feeds it (trainers/ocp_trainer.py:358-402): E_pred [B] /
 * F_pred [N,3] are normalised predictions and are denormalised here (x * std + mean), E_tgt / F_tgt are in target units; the
 * force metrics run over the atoms with fixed == 0 when free_only (fixed == NULL: no atom is fixed), else over all atoms.
 * With M atoms in scope: energy_mae (numel B), forcesx/y/z_mae (M), forces_mae (3M), forces_cosine_similarity (M; per-atom
 * torch.cosine_similarity with eps 1e-8, 0 for an all-zero row), forces_magnitude_error (M; | ||p|| - ||t|| |) and
 * energy_forces_within_threshold (B; total = systems with |dE| < 0.02 and every in-scope |dF component| < 0.03).
 * Departure: a system with no atom in scope makes the reference raise (.max() of an empty slice); here its force maximum
 * counts as 0.  N: rows of F_pred / F_tgt / fixed; atom_offset is clamped to it. */
int32_t adf_eval_s2ef(const float* E_pred, const float* F_pred, const float* E_tgt, const float* F_tgt,
                      const int32_t* fixed, const int32_t* atom_offset, int32_t B, int32_t N, int32_t free_only,
                      float mean_E, float std_E, float mean_F, float std_F, double* total, int64_t* numel, double* scratch,
                      void* stream);
/* Evaluator.task_metrics["is2rs"] over the atoms with fixed == 0 (the split == "val" block of run_relaxations,
 * trainers/ocp_trainer.py:607-642): positions_mae and positions_mse of the plain difference (numel 3M, no minimum image, as
 * the reference) and average_distance_within_threshold: per system the mean over its free atoms of the minimum-image
 * distance (evaluator.py min_diff: fractional = d . inv(cell), % 1.0 twice, > 0.5 -> -1, back through cell [B,3,3], rows =
 * lattice vectors, all three directions periodic), total = thresholds [T] (device, float64: numpy.arange(0.01, 0.5, 0.001)
 * built on the host) that the mean lies strictly below, numel = B * T.  A system without free atoms has a NaN mean and
 * counts for none.  N: rows of pos_pred / pos_tgt / fixed; atom_offset is clamped to it. */
int32_t adf_eval_is2rs(const float* pos_pred, const float* pos_tgt, const float* cell, const int32_t* fixed,
                       const int32_t* atom_offset, int32_t B, int32_t N, const double* thresholds, int32_t T,
                       double* total, int64_t* numel, double* scratch, void* stream);
/* Evaluator.task_metrics["is2re"]: energy_mae, energy_mse and energy_within_threshold (|dE| < 0.02), numel B each. */
int32_t adf_eval_is2re(const float* E_pred, const float* E_tgt, int32_t B, double* total, int64_t* numel, void* stream);
/* Evaluator.update with a plain number: total[slot] += value[0] (a device float), numel[slot] += 1. */
int32_t adf_eval_add(const float* value, int32_t slot, double* total, int64_t* numel, void* stream);

/* ---- EquiformerV2 denoiser (BASELINE config 4).  Replaces
 * EquiformerV2S_OC20_DenoisingPos.forward(data) (models/equiformer_v2/equiformer_v2_denoising.py:185-318) for the
 * configuration the repository ships (configs/denoising/eqv2_so3.yml): one resolution, layer_norm_sh, SiLU attention
 * with re-normalised alpha, separable S2 activation, grid MLP feed-forward, per-block atom edge embeddings, Gaussian
 * distance expansion with 600 functions (equiformer_v2_oc20.py:251-264), FOR_denoising = two force blocks. */
typedef struct adf_eqv2* adf_eqv2_t;
typedef struct {
    int32_t lmax, mmax;              /* lmax_list[0] (1..6), mmax_list[0] (<= lmax)                        */
    int32_t num_layers;
    int32_t sphere_channels;         /* C                                                               */
    int32_t attn_hidden_channels;
    int32_t num_heads, attn_alpha_channels, attn_value_channels;
    int32_t ffn_hidden_channels;
    int32_t grid_resolution;         /* res: the S2 grid has res x res points                           */
    int32_t edge_channels;
    int32_t num_distance_basis;      /* 600 in the reference, whatever the constructor argument says    */
    int32_t max_num_elements;
    int32_t max_neighbors;           /* K of the strict top-K cap                                       */
    float max_radius;                /* cutoff, Angstrom                                                */
    float avg_degree;                /* rescale of the edge-degree embedding (_AVG_DEGREE)              */
} adf_eqv2_hparams;

int32_t adf_eqv2_create(const adf_eqv2_hparams* hp, adf_eqv2_t* out);
int32_t adf_eqv2_destroy(adf_eqv2_t h);

/* Constant tables the reference takes from e3nn / Jd.pt (so3.py:509-531,566-613; wigner.py:8), HOST float32 arrays
 * computed by adsorbdiff_amd/so3_math.py:  jd = J_l row-major, l = 0..lmax concatenated;  to_red / from_red
 * [res*res, S_r] with the |m| <= mmax coefficients in m-major order;  to_full / from_full [res*res, (lmax+1)^2]. */
int32_t adf_eqv2_set_constants(adf_eqv2_t h, const float* jd, const float* to_red, const float* from_red,
                               const float* to_full, const float* from_full);

/* Bind the weights: caller-owned DEVICE float32 tensors in torch layout, reference state_dict names:
 *   0 atom_radii [101]  1 sphere_embedding.weight  2,3 edge_degree_embedding.{source,target}_embedding.weight
 *   4..13 edge_degree_embedding.rad_func  (RAD = net.0.weight, net.0.bias, net.1.weight, net.1.bias, net.3.weight,
 *         net.3.bias, net.4.weight, net.4.bias, net.6.weight, net.6.bias)
 *   then per block i:  norm_1 (NORM = affine_weight, norm_l0.weight, norm_l0.bias), ga (ATTN), norm_2 (NORM),
 *         ffn (so3_linear_1.weight, .bias, scalar_mlp.0.weight, .bias, grid_mlp.0.weight, grid_mlp.2.weight,
 *         grid_mlp.4.weight, so3_linear_2.weight, .bias)
 *   then norm (NORM), force_block (ATTN), force_block2 (ATTN)
 *   ATTN = alpha_dot, source_embedding.weight, target_embedding.weight, so2_conv_1.fc_m0.weight, .bias,
 *          so2_conv_1.so2_m_conv.{0..mmax-1}.fc.weight, so2_conv_1.rad_func (RAD), alpha_norm.weight, .bias,
 *          so2_conv_2.fc_m0.weight, .bias, so2_conv_2.so2_m_conv.{0..mmax-1}.fc.weight, proj.weight, proj.bias */
int32_t adf_eqv2_set_weights(adf_eqv2_t h, int32_t n_weights, const void* const* weights, void* stream);

/* 0 = f16x3 split products on the f16 matrix cores where the shapes allow (default), 1 = exact f32 everywhere. */
int32_t adf_eqv2_set_arithmetic(adf_eqv2_t h, int32_t exact_f32);

/* The conditional model (energy_encoding "scalar", equiformer_v2_denoising.py:130-133,258-264): energy_embedding =
 * nn.Linear(1, C), DEVICE float32 w [C] (weight [C,1]) and b [C], copied.  Every forward then adds to the l = 0 row of
 * the node embedding, before the edge-degree embedding, the term fp16(fp16(e) * fp16(w) + fp16(b)) of the atom's
 * system energy e - the reference's layer run in fp16 (node_wise_y.half(), as under its --amp).  w = b = NULL: the
 * unconditional model (default); one of them NULL: ADF_EINVAL. */
int32_t adf_eqv2_set_energy_embedding(adf_eqv2_t h, const float* w, const float* b, void* stream);
/* The per-system energies e of the conditional model: DEVICE float32 [num_systems], copied; a forward on a batch of
 * another system count returns ADF_EINVAL.  energy = NULL: e = 0 for every system (the reference's sampling mode;
 * the default).  energy != NULL with num_systems < 1: ADF_EINVAL.  Either call drops the incremental blocks' kept
 * state; the term table is built once by the next forward (one tiny launch), not per step of adf_eqv2_sample. */
int32_t adf_eqv2_set_system_energy(adf_eqv2_t h, const float* energy, int32_t num_systems, void* stream);

/* Use this edge list (source, target, vector target -> source image; target non-decreasing; DEVICE arrays, copied)
 * instead of building one, until adf_eqv2_set_edges(h, 0, ...) — parity tests against reference runs whose pick among
 * exactly tied K-th neighbours is implementation-defined. */
int32_t adf_eqv2_set_edges(adf_eqv2_t h, int64_t num_edges, const int32_t* src, const int32_t* dst, const float* vec,
                           int32_t max_in_degree, void* stream);
/* Static-atom cache of the neighbour search, as adf_graph_set_moving. */
int32_t adf_eqv2_set_moving(adf_eqv2_t h, const int32_t* moving, const int32_t* mov_idx, const int32_t* mov_off);

/* The forward: graph (models/base.py:33-123, NOT symmetrised), edge frames + Wigner rows, embeddings, num_layers
 * transformer blocks, final norm, two force blocks.  f1, f2: [N,3] = the l = 1 coefficients (m = -1, 0, 1) of the two
 * force blocks (equiformer_v2_denoising.py:307-318).  x_blocks (optional, may be NULL): [num_layers + 1][N][S][C]
 * node embeddings after the edge-degree embedding and after every block (parity tests). */
int32_t adf_eqv2_forward(adf_eqv2_t h, const adf_batch* b, float* f1, float* f2, float* x_blocks, void* stream);
/* The sampler's forward (cf. adf_painn_forward_subset): only the force blocks read the last node embedding, and the
 * update reads the adsorbate rows of f1 / f2 alone (denoising_torch.py:263-268, 460-467) - the force blocks run for the
 * listed target atoms only (n_out ascending indices, device int32), on a compacted copy of their incoming edges.  Rows
 * out_idx[*] of f1 / f2 are bit-identical to adf_eqv2_forward's; the other rows are NOT written. */
int32_t adf_eqv2_forward_subset(adf_eqv2_t h, const adf_batch* b, const int32_t* out_idx, int32_t n_out, float* f1,
                                float* f2, void* stream);
int32_t adf_eqv2_check_flags(adf_eqv2_t h, void* stream);

/* Reverse-diffusion stepper on an EquiformerV2 handle: same contracts as adf_sde_init_placement,
 * adf_sde_step_scheduled and adf_sample above. */
/* Incremental blocks (off until switched on; the host mirror switches it on for a sampling run, denoising_pos_params
 * ["incremental_layers"], default True).  While a static-atom promise is in force (adf_eqv2_set_moving: same batch, only
 * flagged atoms move) the handle keeps the embedding and every transformer block's output; a forward compares every
 * target's incoming edge list (sources and vectors, bit for bit) with the previous forward's and block i recomputes only
 * the targets within i + 1 hops of a changed one - on a compacted copy of their edges, as adf_eqv2_forward_subset does for
 * the force blocks.  Every output is bit-identical to a full forward; the reference recomputes every row at every step
 * (denoising_torch.py:498 -> equiformer_v2_denoising.py:232-318).  Costs (num_layers + 2) x S x C x 4 bytes per atom
 * (250 KB at config 4) and one 4 x num_layers-byte read-back (a stream synchronisation) per forward, which sizes the
 * launches.  Calling this (with either value) drops the kept state and zeroes the inc_* counters. */
int32_t adf_eqv2_set_incremental(adf_eqv2_t h, int32_t on);

int32_t adf_eqv2_init_placement(adf_eqv2_t h, const adf_batch* b, float* pos, const int32_t* tags, const float* noise,
                                void* stream);
int32_t adf_eqv2_sde_step(adf_eqv2_t h, const adf_batch* b, float* pos, const int32_t* tags, const int32_t* fixed,
                          const float* f1, const float* f2, const adf_step_coef* coef, const adf_step_coef* coefs_dev,
                          int32_t num_steps, const float* z_tr, const float* z_rot, int32_t early_stop_count,
                          int32_t* state, float* dcom, float* drot, void* stream);
int32_t adf_eqv2_sample(adf_eqv2_t h, const adf_batch* b, float* pos, const int32_t* tags, const int32_t* fixed,
                        const adf_step_coef* coefs_dev, int32_t num_steps, const float* z_tr_all, const float* z_rot_all,
                        int32_t early_stop_count, int32_t poll_every, int32_t* state, const int32_t* out_idx, int32_t n_out,
                        float* f1, float* f2, void* stream);
int32_t adf_eqv2_sample_traj(adf_eqv2_t h, const adf_batch* b, float* pos, const int32_t* tags, const int32_t* fixed,
                             const adf_step_coef* coefs_dev, int32_t num_steps, const float* z_tr_all, const float* z_rot_all,
                             int32_t early_stop_count, int32_t poll_every, int32_t* state, const int32_t* out_idx, int32_t n_out,
                             float* f1, float* f2, adf_frames_t sink, int32_t frame_every, void* stream);

/* Translation-only samplers on an EquiformerV2 handle: same contracts as adf_tr_step / adf_tr_sample[_traj]; the fused
 * loop runs force_block only (no force_block2, a whole SO(2) attention block, equiformer_v2_denoising.py:307-318). */
int32_t adf_eqv2_tr_step(adf_eqv2_t h, const adf_batch* b, float* pos, const int32_t* tags, const float* f1,
                         const adf_tr_coef* coef, const adf_tr_coef* coefs_dev, int32_t num_steps, const float* z,
                         int32_t early_stop_count, int32_t* state, float* dcom, void* stream);
int32_t adf_eqv2_tr_sample(adf_eqv2_t h, const adf_batch* b, float* pos, const int32_t* tags,
                           const adf_tr_coef* coefs_dev, int32_t num_steps, const float* z_all, int32_t early_stop_count,
                           int32_t poll_every, int32_t* state, const int32_t* out_idx, int32_t n_out, float* f1,
                           void* stream);
int32_t adf_eqv2_tr_sample_traj(adf_eqv2_t h, const adf_batch* b, float* pos, const int32_t* tags,
                                const adf_tr_coef* coefs_dev, int32_t num_steps, const float* z_all,
                                int32_t early_stop_count, int32_t poll_every, int32_t* state, const int32_t* out_idx,
                                int32_t n_out, float* f1, adf_frames_t sink, int32_t frame_every, void* stream);

/* adf_painn_set_per_system_stop on an EquiformerV2 handle: adf_eqv2_sde_step, adf_eqv2_tr_step and the fused loops. */
int32_t adf_eqv2_set_per_system_stop(adf_eqv2_t h, int32_t* sys_state, int32_t B);

/* Stand-alone torch.nn.functional.linear (+ optional SiLU, act = 2) through this path's dense-product kernels (unit tests
 * and micro-benchmarks of so2_ops.py:12-79,158-238 / so3.py:694-745 shapes).  A [M,K], W [N,K], bias [N] or NULL, C [M,N],
 * device pointers.  mode 0: exact f32; 1: f16x3 split with per-row power-of-two lifts (fp32 rows split in the kernel;
 * K % 32 == 0, N % 4 == 0); 2: the same product on rows pre-split into fp16 hi / lo images; 3: as 2 with the weights
 * streamed from their MFMA-fragment image (the sampler's first SO(2) convolution; N % 32 == 0, N >= 128, K % 64 == 0;
 * bit-identical to 2).  repeat > 1 re-runs the product kernel alone.  Synchronises. */
int32_t adf_eqv2_linear_forward(const float* A, const float* W, const float* bias, float* C, int64_t M, int32_t N, int32_t K,
                                int32_t act, int32_t mode, int32_t repeat, void* stream);

/* Work of the last forward and HIP-event time per kernel group (bench.py roofline).  Categories: 0 graph + Wigner,
 * 1 radial MLPs, 2 rotate in / out, 3 SO(2) convolution products, 4 S2 activation, 5 attention weights, 6 node-side
 * norms / SO(3) linears, 7 feed-forward grid MLP, 8 stepper. */
#define ADF_EQV2_PROF_NCAT 9
typedef struct {
    int64_t num_edges, num_atoms;
    int64_t dense_flops;       /* 2 x multiply-adds of every dense product of the REFERENCE's forward (f32-equivalent work) */
    int64_t conv_flops;        /* 2 x multiply-adds the SO(2)-convolution kernels of the last forward executed (force blocks:
                                * l = 1 columns only; subset forward / incremental blocks: the listed targets' edges only,
                                * estimated) */
    int64_t inc_rows, inc_rows_full;  /* incremental blocks, totals since adf_eqv2_set_incremental: block rows recomputed /
                                       * block rows full forwards would have computed (blocks x atoms) */
    int64_t forwards_total, conv_flops_total;  /* forwards since adf_eqv2_profile_enable(1) and conv_flops summed over them
                                                * (on the last forward's edge count) */
} adf_eqv2_counters;
int32_t adf_eqv2_get_counters(adf_eqv2_t h, adf_eqv2_counters* out, void* stream);
int32_t adf_eqv2_profile_enable(adf_eqv2_t h, int32_t on);
int32_t adf_eqv2_profile_read(adf_eqv2_t h, float* ms, int64_t* count, void* stream);

/* ---- EquiformerV2 S2EF force field (models/equiformer_v2/equiformer_v2_oc20.py:415-562, class EquiformerV2_OC20): the
 * denoiser's handle and forward with (1) no atomic radii - edge distances enter the Gaussian basis as they are, so the
 * basis is live on every edge and no radial function is tabulated per element pair; (2) one force block; (3) an energy
 * head.  Atomic numbers are valid in [0, max_num_elements).
 *
 * adf_eqv2_set_weights_s2ef binds the S2EF table: the table of adf_eqv2_set_weights WITHOUT entry 0 (atom_radii) and
 * WITHOUT the trailing force_block2 (ATTN) entries; everything else in the same order.  It also tabulates, per radial
 * function, the element-embedding part of the first layer, b0 + W_s semb[Z_s] + W_t temb[Z_t], per element pair
 * ([max_num_elements^2, edge_channels]); every forward then evaluates per edge only the window of Gaussians that do not
 * underflow (at most 58 of the 600), fused with the LayerNorm + SiLU that follows.  adf_eqv2_set_weights on the same
 * handle switches back to the denoiser. */
int32_t adf_eqv2_set_weights_s2ef(adf_eqv2_t h, int32_t n_weights, const void* const* weights, void* stream);

/* The energy head.  With use_grid_mlp and use_sep_s2_act only the gating scalars reach the l = 0 output of energy_block
 * (transformer_block.py:473-530), so per atom e = w2 . SiLU(W1 x[:, 0, :] + b1) + b2.  DEVICE float32 tensors, read by
 * pointer on every forward (the first is also split into its fp16 hi/lo image here: bind again after changing it):
 *   0 energy_block.scalar_mlp.0.weight [F, C]  1 energy_block.scalar_mlp.0.bias [F]
 *   2 row 0 of energy_block.so3_linear_2.weight[0] [F]  3 energy_block.so3_linear_2.bias [1]
 * energy_lin_ref: [max_num_elements] device table added per atom (use_energy_lin_ref), or NULL. */
int32_t adf_eqv2_set_energy_head(adf_eqv2_t h, int32_t n_weights, const void* const* w, float avg_num_nodes,
                                 const float* energy_lin_ref, void* stream);

/* S2EF forward: energy [B] = (sum_i e_i) / avg_num_nodes (+ energy_lin_ref[Z_i] atom by atom), forces [N,3] = the l = 1
 * coefficients of force_block (NULL: the force block is not evaluated), x_blocks as adf_eqv2_forward (may be NULL).  The
 * per-system sum runs in a fixed order (one workgroup per system, no atomics): a system's energy is bit-identical
 * whatever batch it sits in.  adf_eqv2_forward on an S2EF handle needs f2 = NULL. */
int32_t adf_eqv2_forward_energy(adf_eqv2_t h, const adf_batch* b, float* energy, float* forces, float* x_blocks,
                                void* stream);

/* Unit-test hook: the S2EF model's first radial layer + LayerNorm + SiLU of radial function `which` (0 edge-degree
 * embedding, 1..num_layers the blocks, num_layers + 1 the force block) on a caller's edges: src / dst [E] index Z,
 * vec [E,3], out [E, edge_channels]; device pointers.  Synchronises. */
int32_t adf_eqv2_radial_first_layer(adf_eqv2_t h, int32_t which, int64_t num_edges, const int32_t* src, const int32_t* dst,
                                    const float* vec, const int32_t* Z, float* out, void* stream);

/* ---- S2EF PaiNN (models/painn/painn.py:52-432): the denoiser's handle with one force head (num_heads = 1, or 0 for
 * regress_forces=False) plus the energy head out_energy = Linear(H, H/2), ScaledSiLU, Linear(H/2, 1), summed per system.
 * adf_painn_set_weights keeps its table; the energy head is bound separately, in this order:
 *   0 out_energy.0.weight [H/2, H]  1 out_energy.0.bias [H/2]  2 out_energy.2.weight [1, H/2]  3 out_energy.2.bias [1]
 * The tensors are read by pointer on every forward (bind again after they move); the first one is also split into the
 * fp16 hi/lo image of the f16x3 arithmetic here, so bind again after changing it. */
int32_t adf_painn_set_energy_head(adf_painn_t h, int32_t n_weights, const void* const* w, void* stream);

/* Floor of the edge distances (edges at or below it get it): 1e-3 by default (painn_denoising.py:366-367, so the
 * denoiser's graphs are unchanged), 1e-6 for the S2EF model (painn.py:334-335).  The radius graph drops pairs closer
 * than 0.01 A before (d^2 > 1e-4, utils/utils.py:536-540), so neither floor is reached by an edge of a valid graph. */
int32_t adf_painn_set_distance_floor(adf_painn_t h, float floor);

/* S2EF forward: energy [B] and forces [N,3] (forces may be NULL when num_heads == 0).  The per-system sum runs in a fixed
 * order (one workgroup per system, no atomics): a system's energy is bit-identical whatever batch it sits in. */
int32_t adf_painn_forward_energy(adf_painn_t h, const adf_batch* b, float* energy, float* forces, void* stream);

/* Forces as the gradient of the energy: energy [B] and forces [N,3] = -dE/dpos with E = sum of the per-system energies and the
 * edge set held fixed.  Replaces, for the S2EF PaiNN,
 *     pos.requires_grad_(True); out = model(data); forces = -torch.autograd.grad(out["energy"].sum(), pos)[0]
 * on the reference module (models/painn/painn.py:318-340, 380-414).  It is NOT the reference's direct_forces=False branch
 * (painn.py:421-429), which differentiates the sum of the last node embedding x instead of the energy.  Works with
 * num_heads == 0 (a model without a force head); the force head, if any, is not evaluated.  One call does the whole
 * evaluation on `stream` without host synchronisation once the workspaces have grown: graph build, a forward that keeps
 * 21 H floats per atom and layer, the data-gradient backward (no weight-gradient product; the transposed weight images are
 * built once per adf_painn_set_weights / adf_painn_set_energy_head), the edge-geometry gradient of every message block and
 * its reduction onto the atoms.  No float atomics: the result is run-to-run identical and a system's energy and forces do
 * not depend on the batch it sits in.  The energy comes from the same per-system sum as adf_painn_forward_energy's but from
 * an unfused ScaledSiLU, so the two may differ in the last bits.  Errors as adf_painn_forward_energy; ADF_EOOM when the
 * workspace cannot be allocated (split the batch).  Flags: adf_check_flags. */
int32_t adf_painn_forward_energy_gradient(adf_painn_t h, const adf_batch* b, float* energy, float* forces, void* stream);

/* Bytes of library-owned device memory adf_painn_forward_energy_gradient holds for a batch of num_atoms atoms: activations,
 * per-edge partial gradients (sized for either arithmetic), reverse-edge index and the images of the transposed weights. */
int32_t adf_painn_energy_gradient_workspace(adf_painn_t h, int64_t num_atoms, int64_t* bytes);

/* ---- Batched L-BFGS of ml_relax (relaxation/optimizers/lbfgs_torch.py:22-213), model-agnostic.  All state lives on the
 * device in fp64: s / y rings [memory, 3N], rho, alpha, r0, f0, q / z.  Dot products run over the whole flattened batch
 * (as in the reference: the systems of one batch are coupled) with fixed-order reductions and no atomics, so a relaxation
 * is bit-reproducible run to run.  ADF_EOOM when the history does not fit (ml_relax then splits the batch). */
typedef struct adf_lbfgs* adf_lbfgs_t;
int32_t adf_lbfgs_create(int64_t num_atoms, int32_t num_systems, int32_t memory, double maxstep, double damping,
                         double alpha, int32_t early_stop_batch, adf_lbfgs_t* out);
int32_t adf_lbfgs_destroy(adf_lbfgs_t h);
/* a new run on the same batch shape: the history is forgotten and r0, f0 and the update mask are zeroed (enqueued on
 * `stream`), as in a fresh handle */
int32_t adf_lbfgs_reset(adf_lbfgs_t h, void* stream);
/* check_convergence (:70-88): max_force[b] = max over system b of |f_atom| in fp64 (max_force f64 [B], may be NULL);
 * the update mask of system b is max_force[b] >= fmax and is kept for the next step; *all_converged (device int32, may
 * be NULL) = no mask set.  forces: f32 [N,3] with the constraint already applied. */
int32_t adf_lbfgs_converge(adf_lbfgs_t h, const int32_t* atom_offset, const float* forces, double fmax,
                           double* max_force, int32_t* all_converged, void* stream);
/* LBFGS.step (:134-189), for iteration = 0, 1, 2, ... in order from a fresh or reset handle (anything else: ADF_EINVAL):
 * history append (iteration > 0, deque of maxlen memory), the batch-global two-loop recursion over
 * loopmax = min(memory, iteration) entries, determine_step, the skip of a step whose max |dr| over the batch is below 1e-7
 * (decided on the device; r0 / f0 then stay) and pos += f32(dr) where the last converge's mask is set (everywhere with
 * early_stop_batch).  pos: f32 [N,3] in / out.  Enqueues 3 + 2 loopmax launches, no host synchronisation.  In per-system
 * mode (adf_lbfgs_set_per_system) the step is the one described there, in one launch. */
int32_t adf_lbfgs_step(adf_lbfgs_t h, const int32_t* atom_offset, float* pos, const float* forces, int64_t iteration,
                       void* stream);
/* the update mask of the last converge, int32 [B] device */
int32_t adf_lbfgs_get_mask(adf_lbfgs_t h, int32_t* out, void* stream);
/* the search direction z of the last step (the two-loop recursion's result, before determine_step), f64 [3N] device; a
 * device-to-device copy on `stream`.  Both modes; in per-system mode the rows of a system whose mask was clear are those of
 * its own last step (undefined before it).  ADF_EINVAL on a null argument or a handle that has not stepped since create /
 * reset. */
int32_t adf_lbfgs_get_direction(adf_lbfgs_t h, double* z_out, void* stream);
/* max |dr| over the batch of the last step (below 1e-7: the step was skipped), device f64 scalar.  Maxima here propagate
 * NaN as the reference's reductions do: a NaN force clears its system's mask and does not make the step skip. */
int32_t adf_lbfgs_last_step_max(adf_lbfgs_t h, double* out, void* stream);
/* Per-system mode (on != 0) or the coupled recursion above (0, the default).  Valid on a handle that has not stepped since
 * create / reset (ADF_EINVAL afterwards) and not together with early_stop_batch (ADF_EINVAL: it moves converged systems
 * while others run, so a system alone and in a batch would differ by design); allocates rho / alpha [B, memory] and the
 * step counters.  In this mode every system b keeps its own step counter t_b (0 at create / reset), its slice of the
 * rings, its own rho and alpha, and adf_lbfgs_step does, in ONE launch with one workgroup per system:
 *   mask of the last converge clear: nothing - no history append, r0 / f0 / pos untouched, t_b unchanged;
 *   mask set, t = t_b: if t > 0 append s = r - r0, y = -(f - f0), rho = 1 / dot(y, s) (deque of maxlen memory); the
 *   two-loop recursion over loopmax = min(memory, t) entries with every dot product over this system's 3 n_b entries
 *   only; determine_step; the step is skipped when the largest |dr| of THIS system is below 1e-7 (the maximum propagates
 *   NaN, so a NaN does not skip; pos, r0 and f0 then stay); otherwise pos += f32(dr), r0 = r, f0 = f; t_b += 1 either way.
 * That is the step LBFGS.step (:134-189) takes for iteration t_b when the system is alone in its batch.  The summation
 * order of a dot product depends on the system's atom count alone (a 256-strided sum per thread, then a fixed tree), so a
 * system's relaxation has the same bits alone, in any batch and on any shard.  adf_lbfgs_step keeps its iteration check
 * (0, 1, 2, ... from a fresh or reset handle), adf_lbfgs_reset zeroes the counters too, and adf_lbfgs_last_step_max is the
 * NaN-propagating maximum over the systems that attempted a step (0 when none did). */
int32_t adf_lbfgs_set_per_system(adf_lbfgs_t h, int32_t on);
/* Per-system mode only (ADF_EINVAL otherwise): steps_taken[b] = t_b (int32 [B], device) and last_absmax[b] = the largest
 * |dr| of system b in the last adf_lbfgs_step (f64 [B], device; below 1e-7: that system skipped; -1: its mask was clear
 * and it attempted nothing).  Either output may be NULL. */
int32_t adf_lbfgs_get_step_state(adf_lbfgs_t h, int32_t* steps_taken, double* last_absmax, void* stream);

/* ---- The active set: the systems whose update mask is set, so that a relaxation can leave the converged ones out of the
 * model forward (LBFGS.set_drop_converged).  That mode rests on two properties of the force model, not on anything in
 * these entries: a system's energy and force rows do not depend on the batch it is evaluated in, and the forward is
 * deterministic run to run; then the rows kept from a system's last forward are the bits a new forward would return.  A
 * model without them gets a different relaxation, not a wrong-by-construction one: every system is still relaxed until its
 * own convergence.  All arrays are on the device; B is the handle's system count.
 *
 * adf_lbfgs_active_build, from the mask the last adf_lbfgs_converge left in the handle (ADF_EINVAL before any converge
 * since create / reset, and for a NULL argument): act_sys [B] = the ids of the systems whose mask is set, ascending,
 * padded with -1; act_offset [B + 1] = the exclusive prefix sum of those systems' atom counts, entries past B_act equal
 * N_act; info [4] = {B_act, N_act, changed, 0}.  changed = 1 when the list differs from the one the previous build on this
 * handle wrote; the first build after create / reset always reports 1 (the handle keeps the previous mask, adf_lbfgs_reset
 * forgets it).  One launch of one workgroup: an integer scan that walks B in chunks of the workgroup size with a carried
 * prefix, in a fixed order, no atomics. */
int32_t adf_lbfgs_active_build(adf_lbfgs_t h, const int32_t* atom_offset, int32_t* act_sys, int32_t* act_offset,
                               int32_t* info, void* stream);
/* One array of a gather: rows of row_bytes bytes (a positive multiple of 4; src and dst 4-byte aligned), one row per atom
 * (per_system = 0) or per system (per_system != 0). */
typedef struct adf_active_field {
    const void* src;
    void* dst;
    int32_t row_bytes;
    int32_t per_system;
} adf_active_field;
#define ADF_ACTIVE_MAX_FIELDS 16
/* Gather, no handle.  For the k-th active system s = act_sys[k] (k < info[0], read on the device; the grid is sized by
 * num_systems and workgroups past B_act exit): rows [atom_offset[s], atom_offset[s+1]) of every per-atom field go to rows
 * [act_offset[k], act_offset[k+1]) of its dst, row s of every per-system field goes to row k.  batch_out (int64, one per
 * compact atom, value k) and natoms_out (int64, one per compact system) are written when not NULL.  ONE launch copies all
 * fields (at most ADF_ACTIVE_MAX_FIELDS) as contiguous dword ranges.  num_atoms is the atom count of the full batch (it
 * sizes the grid only).  ADF_EINVAL: a NULL list or field pointer, a row_bytes that is not a positive multiple of 4, a
 * misaligned pointer, more fields than the maximum, nothing to write. */
int32_t adf_active_gather(const int32_t* atom_offset, const int32_t* act_sys, const int32_t* act_offset,
                          const int32_t* info, int32_t num_systems, int64_t num_atoms, const adf_active_field* fields,
                          int32_t num_fields, int64_t* batch_out, int64_t* natoms_out, void* stream);
/* Scatter, the inverse for the outputs of a compact forward.  forces_c f32 [N_act, 3] go to the rows of the active systems
 * in forces_raw and in forces_con (both f32 [N, 3]); a row of forces_con is +0 where fixed (int32 [N]) != 0 and the raw row
 * otherwise.  energy_c [B_act] rows of energy_row_bytes bytes (a positive multiple of 4) go to rows act_sys[k] of energy.
 * Rows of systems outside the list are not written.  One launch, plain vector stores.  energy_c / energy may both be NULL
 * (forces only). */
int32_t adf_active_scatter(const int32_t* atom_offset, const int32_t* act_sys, const int32_t* act_offset,
                           const int32_t* info, int32_t num_systems, int64_t num_atoms, const float* forces_c,
                           const void* energy_c, int32_t energy_row_bytes, const int32_t* fixed, float* forces_raw,
                           float* forces_con, void* energy, void* stream);

/* ---- Two half-batches, two streams (csrc/stepper.hip sample_loop_split).
 *
 * Systems of a batch never interact, so the two sides of a cut at a system boundary are two independent dependent chains
 * of kernels.  adf_sample_split runs view A (systems [0, cut)) on the caller's stream with the handle and view B (systems
 * [cut, B)) on a library-owned non-blocking stream with the handle's twin, forked by one event at entry and joined by one
 * event before it returns; the host enqueues step t of A, then step t of B.  Every result - positions, f1 / f2, state,
 * the per-system table - has the bits of adf_sample on the whole batch.
 */

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

/* ---- Scale-factor fit (csrc/scale_fit.hip, api.hip).
 *
 * Fitting the scale factors (modules/scaling/fit.py, scale_factor.py:106-172): a ScaleFactor observes
 * torch.mean(torch.var(x, dim=0)) of the node features it returns, batch by batch; the fit is sqrt(1 / (the atom-weighted
 * mean of those)).
 */

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

/* ---- Slab cutting (csrc/slabcut.hip, adsorbdiff_amd/slabs.py).
 *
 * The reference's compute_slabs (placement/slab.py:485-552: pymatgen's SlabGenerator, StructureMatcher and
 * SpacegroupAnalyzer per Miller index) and get_symmetrically_distinct_miller_indices for a batch of bulks.  Neither
 * pymatgen nor spglib was run against it: parity with pymatgen unpinned; what follows is the contract.  The bulk's cell is
 * taken as given (no standardize_bulk).  All arithmetic is double; a bulk's results do not depend on the batch it is in,
 * and two runs give the same bits (no float atomics).
 *
 * A batch of B bulks: pos double [N,3] (Cartesian), cell double [B,9] (rows = lattice vectors, right-handed),
 * atomic_numbers int32 [N], atom_offset int32 [B+1]; periodic in all three directions.
 *
 * Per (bulk, Miller index h), h divided by its gcd:
 *  1. Oriented cell.  (u1, u2): a basis of the integer lattice {u : h.u = 0} from the extended Euclid algorithm,
 *     Lagrange-Gauss reduced in the Cartesian metric.  u1 is the shortest vector of that lattice; among vectors whose
 *     squared lengths differ by no more than 1e-9 L^2 (L: the cell's longest edge) the lexicographically greatest integer
 *     triple.  u2 is, among the vectors v that complete u1 to a basis with u1 x u2 = h (so that the Cartesian cross product
 *     points along the plane normal n, the direction of h in the reciprocal basis), the shortest one with
 *     u1.v <= 1e-9 |u1|^2.  Hence |u1| <= |u2| and u1.u2 <= 0 (within that tolerance), right-handed.  Where the two shortest
 *     vectors form an obtuse pair of the other hand, u2 is therefore not the second shortest vector but that minus u1.
 *     u3: the integer vector with h.u3 = 1 whose component in the plane is shortest; ties (1e-9 L^2 on the squared
 *     length) to the lexicographically greatest triple.  (u1, u2, u3) is unimodular; the height of the cell along n is
 *     d = d_hkl.
 *  2. Thickness.  n_slab = ceil(min_slab_size / d) oriented cells of slab, n_vac = ceil(min_vacuum_size / d) of vacuum.
 *     Output frame: cell[0] along +x, cell[1] in the xy plane, cell[2] = (0, 0, (n_slab + n_vac) d) - perpendicular, where
 *     pymatgen keeps the oblique u3: a stated deviation, equivalent for every consumer behind the vacuum.  The slab is
 *     centred at half that height: (lowest atom + highest atom) / 2 lies there.
 *  3. Terminations.  The heights of the oriented cell's atoms modulo d, sorted; every periodic gap above `tol` gives a cut
 *     plane at its midpoint, `shift` = that height in [0, d); a plane within 1e-9 A of d is the plane at 0.  No gap above tol: one cut, in the largest gap (ties within
 *     1e-9 A to the lowest height).  A cut's slab holds the n_slab oriented cells above the plane.
 *  4. Primitive in-plane cell.  The in-plane translations that map the oriented cell's atoms onto themselves (species equal,
 *     positions within symprec, modulo (u1, u2, u3) - for a slab of whole oriented cells these are the translations that map
 *     the slab onto itself) generate with u1, u2 a finer lattice.  Its basis (p1, p2): p1 the shortest vector, ties
 *     (1e-9 L^2) to the greatest component along u1, then the greatest across it; p2 by the rule of u2.  One atom per
 *     translation class is kept, the one of the lowest index in the bulk.  Without such translations (p1, p2) = (u1, u2).
 *     Translations that do not close to a group at this symprec refuse the bulk.
 *  5. Duplicate terminations.  Two cuts are the same slab when some (x, y) -> R (x, y) + tau, z kept relative to the slabs'
 *     mid-planes, takes every atom of one onto an atom of its species of the other within symprec, modulo (p1, p2).  R: the
 *     point operations of the lattice (p1, p2) - integer 2 x 2 matrices W (entries -2 .. 2, determinant +-1) in that basis
 *     under which |p1|, |p2| and |p1 + p2| keep their lengths within symprec, as adf_slab_symmetry_search finds them.  tau:
 *     whatever takes the first atom of the rarest species onto an atom of its species at its height.  Atoms closer than
 *     2 symprec to each other are not told apart.  The cut with the smaller shift is kept.
 *  6. Top and bottom.  A kept slab is invertible when the test of 5 maps it onto itself after z -> -z about its mid-plane
 *     (any operation with R_zz = -1).  Every kept slab is emitted with top = 1; a non-invertible one again with top = 0:
 *     turned by 180 degrees about x through its centre, cell[2] restored to +z, cell[1] negated and, where that leaves
 *     cell[0].cell[1] > 0, lowered by cell[0] (the rule of u2 once more: the cell stays right-handed and obtuse), centred and
 *     wrapped.  Flipped slabs are not compared with other terminations.
 *  7. Order.  Pairs in the caller's order.  Within a pair the top = 1 slabs by ascending shift, then the top = 0 slabs in the
 *     same order.  Atoms: wrapped to fractional in-plane coordinates in [-1e-6, 1 - 1e-6); atom a precedes atom b when it is
 *     lower by more than symprec; else (same layer) when its first fractional coordinate is smaller by more than 1e-6; else
 *     when its second is; the position of an atom is the number of atoms that precede it.
 */

/* Distinct Miller indices.  The point group of each bulk: the integer matrices W with entries in {-1, 0, 1} whose rows
 * a'_i = sum_j W_ij a_j keep the lengths of the three edges and the three face diagonals within symprec, and under which
 * f -> f W + t maps the atoms onto themselves (species equal, within symprec) for some t.  The search is complete for
 * conventional and reduced cells; for other cells it can only miss operations, which splits classes: duplicate slabs later,
 * never a wrong one.  The classes: gcd-reduced h with |h|, |k|, |l| <= max_miller under h -> W h and h -> -h; the
 * representative is the lexicographically greatest member inside the box; representatives come in descending order.
 *
 * adf_distinct_millers_count: found (device) and found_host (host) int32 [3 B]: per bulk the number of indices, the order
 * of the group, error bits.  One launch, one read-back.  max_miller outside 1 .. 4, symprec not finite and positive:
 * ADF_EINVAL; a bulk with a singular, left-handed or non-finite cell: ADF_EINVAL, the message names the bulk, its atoms are
 * not read.  scratch: adf_distinct_millers_scratch(N, B) bytes, 256-byte aligned, kept for the fill.
 * adf_distinct_millers_fill: millers int32 [capacity, 3]; bulk b's indices from miller_offset[b] (int32 [B+1], the
 * exclusive scan of the counts).  capacity below the total: ADF_EOVERFLOW, nothing written. */
int64_t adf_distinct_millers_scratch(int32_t num_atoms, int32_t num_bulks);
int32_t adf_distinct_millers_count(const double* pos, const double* cell, const int32_t* atomic_numbers,
                                   const int32_t* atom_offset, int32_t num_atoms, int32_t num_bulks, int32_t max_miller,
                                   double symprec, void* scratch, int32_t* found, int32_t* found_host, void* stream);
int32_t adf_distinct_millers_fill(const void* scratch, const int32_t* found, const int32_t* found_host,
                                  const int32_t* miller_offset, int32_t num_atoms, int32_t num_bulks, int32_t max_miller,
                                  int32_t capacity, int32_t* millers, void* stream);

/* Slabs: count, then fill.  P pairs: pair_bulk int32 [P], pair_miller int32 [P,3]; pair p works in the scratch segment
 * pair_atom_offset[p] .. pair_atom_offset[p+1] (int64 [P+1]), at least its bulk's atoms long; segment_atoms: the last
 * offset.  scratch: adf_slab_cut_scratch(segment_atoms, P) bytes, 256-byte aligned, kept for the fill.
 *
 * adf_slab_cut_count: counts (device) and counts_host (host) int32 [3 P]: slabs of the pair, atoms of each of them, error
 * bits.  One launch, one read-back.  A size or tolerance that is not finite and positive: ADF_EINVAL.  h = (0,0,0), a
 * singular, left-handed or non-finite cell, a bulk without atoms, a slab beyond 2^20 atoms, translations that do not close:
 * ADF_EINVAL, the message names the bulk; the bulk's atoms are not read and its segment is not written.
 *
 * adf_slab_cut_fill: pair p's slabs are rows pair_slab_offset[p] .. of the per-slab outputs, its atoms rows
 * pair_out_offset[p] .. (int32 [P+1], int64 [P+1]: the exclusive scans of the counts and of slabs x atoms).  pos64 double
 * [atom_capacity, 3], pos32 float [atom_capacity, 3] (pos64 rounded once), atomic_numbers int32 [atom_capacity]; cell double
 * [slab_capacity, 9], millers int32 [slab_capacity, 3] (gcd-reduced), shift double, top / bulk_index / natoms int32
 * [slab_capacity].  Offsets that are not the count pass's, or that pass a capacity: ADF_EOVERFLOW, the message names the
 * bulk, nothing is written.  Two launches (the check, the fill) and one read-back. */
int64_t adf_slab_cut_scratch(int64_t segment_atoms, int32_t num_pairs);
int32_t adf_slab_cut_count(const double* pos, const double* cell, const int32_t* atomic_numbers, const int32_t* atom_offset,
                           int32_t num_atoms, int32_t num_bulks, const int32_t* pair_bulk, const int32_t* pair_miller,
                           const int64_t* pair_atom_offset, int32_t num_pairs, int64_t segment_atoms, double min_slab_size,
                           double min_vacuum_size, double tol, double symprec, void* scratch, int32_t* counts,
                           int32_t* counts_host, void* stream);
int32_t adf_slab_cut_fill(const void* scratch, const int32_t* pair_bulk, const int64_t* pair_atom_offset,
                          const int32_t* pair_slab_offset, const int64_t* pair_out_offset, int32_t num_pairs,
                          int64_t segment_atoms, double symprec, int32_t slab_capacity, int64_t atom_capacity, double* pos64,
                          float* pos32, int32_t* atomic_numbers, double* cell, int32_t* millers, double* shift, int32_t* top,
                          int32_t* bulk_index, int32_t* natoms, void* stream);

const char* adf_last_error(void);
const char* adf_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ADSORBDIFF_HIP_H */
