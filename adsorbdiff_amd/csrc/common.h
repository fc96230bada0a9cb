// Internal declarations shared by the HIP translation units of libadsorbdiff_hip.so.
// gfx950 (MI355X) only: 64-wide wavefronts, f32 MFMA 32x32x2, 160 KiB LDS per CU.
#pragma once
#include "base.h"
#include "switches.h"
#include "arith.h"
#include "lanes.h"

#define ADF_GROUP_NODES 32      // target nodes per message-kernel work item
#define ADF_SLICE_CH 64         // channels per message-kernel slice (x3 parts = 192 MFMA columns)
#define ADF_MAX_CAND 1024       // in-cutoff candidates per centre held in LDS by the top-K kernel
#define ADF_MAX_K 128
#define ADF_NFLAGS 8
#define ADF_MAX_INDEG 1024
#define ADF_MAX_LAYERS 16      // incoming edges per target the per-target sorter handles (graph.hip)

// fp16 hi/lo split of one nn.Linear weight (gemm16.hip), library-owned
struct adf_w16 {
    void* hi;
    void* lo;
    float* inv_scale;  // device scalar: 1 / (power-of-two scale applied before the split)
    float* bias_perm;  // row-permuted bias of the fused 3H-wide layers (else null)
    void* frag;        // fragment-ordered image of hi / lo (adf_pack_frag, gemm16.hip): the B operands of v_mfma_f32_32x32x16_f16
                       // as the lanes load them, for the kernels that stream weights straight into registers (null: none)
};
// operands of the fused GEMM epilogues (gemm16.hip)
struct adf_epi {
    const float* vec_in;  // EPI 1: vec [N,3,H] (P_i = vec_i * xb)
    float* rec;           // EPI 1: gather records
    float* x;             // EPI 2
    float* vec;           // EPI 2
    const float* dot;     // EPI 2
    const float* vv;      // EPI 2: v1 [N,3,H] (written by EPI 3)
    float* v1;            // EPI 3: v1 out [N,3,H]
    float* dotw;          // EPI 3: dot out [N,H]
    float* cat;           // EPI 3: |v2| [N,H] ; EPI 4: norm [M,N]
    float scale;          // EPI 2: ScaleFactor
    int H;
    int vec_is_zero;      // EPI 1
    const float* A2;      // any EPI: second source of the A operand for columns [K1, K) (same row stride), K1 % 32 == 0
    int K1;               // 0 = single source
    const int32_t* row_map;  // EPI 1: record row of tile row n is row_map[n] (compact rows of an incremental layer); null = n
    // any EPI: per-row magnitudes max|a| of the A rows (indexed like the rows are loaded: atom*3 + component for EPI 3/4).
    // Each row is lifted by its own power of two before the fp16 hi/lo split and the lift is divided out in the epilogue
    // (an unlifted element below ~0.1 loses its a_lo term to the matrix core's subnormal flush).  null = no lift.
    const float* rmag;
    unsigned int* out_mag;   // EPI 0: receives max|c| of every output row (atomicMax on float bits; zeroed by the launcher)
    // any EPI: the row count lives on the device (an incremental layer's recompute list, incremental.hip): rows =
    // min(M, *m_dev); the launch is sized for M.  null = M.
    const int32_t* m_dev;
    int accumulate;          // EPI 0: C += A W^T (+ bias) instead of C = (the training step's accumulated data gradients)
    const float* gate;       // EPI 0 (heads): multiply output row r, column c by gate[(r / 3) * gate_ld + c]  (null: no gate)
    int gate_ld;
    // Partial row maxima (see adf_painn::rmx_part): a producer writes, with plain stores, the maximum over the columns it owns
    // into a slot of its own, [part][part_stride]; adf_launch_rowmax_combine takes the maximum over the parts.
    float* catpart;          // EPI 3: max |v2| of row n over the 32 channels of group g -> catpart[g * part_stride + n]
    long long part_stride;
};
// scratch for the row magnitudes a launcher measures itself (adf_launch_rowmag) when the caller has none to hand over
struct adf_lift {
    float* buf;
    long long cap;   // rows
};
struct adf_layer_weights {
    const float *ln_w, *ln_b, *xp0_w, *xp0_b, *xp2_w, *xp2_b, *rbf_w, *rbf_b;
    const float *vp_w, *xv0_w, *xv0_b, *xv2_w, *xv2_b;
    adf_w16 xp0_16, xp2_16, vp_16, xv0_16, xv2_16;
};
struct adf_block_weights {
    const float *vec1_w, *vec2_w, *un0_w, *un0_b, *un2_w, *un2_b;
    adf_w16 vec1_16, vec2_16, un0_16, un2_16;
};

struct adf_painn {
    adf_painn_hparams hp;
    int device;
    bool weights_set;
    const float* emb;
    const float* rbf_offset;
    adf_layer_weights layer[16];
    adf_block_weights head[2][2];
    float scale[16];
    // message-kernel image of rbf_proj: [layer][slice][R][192] and bias [layer][slice][192]
    float* rbf_pack;
    float* rbf_bias_pack;
    // f16 hi/lo image of (rbf_proj * scale): [layer][slice][hi|lo][192][R] halves; bias * scale; 1/scale per layer
    void* rbf_pack16;
    float* rbf_bias_pack16;
    float* rbf_scales;
    // fp16 hi/lo images of every GEMM weight (one arena) + their scales; gemm_f32 selects the exact path
    unsigned char* w16_arena;
    size_t w16_bytes;
    float* w16_scales;
    float* w16_bias_perm;  // [L][2][3H] row-permuted biases of x_proj.2 / xvec_proj.2
    unsigned int* w16_scratch;
    unsigned char* wfrag_arena;   // fragment images of every split weight (adf_w16::frag), same size as w16_arena
    bool gemm_f32;
    bool msg_f32;
    bool msg_f32_only;   // num_rbf % 8 != 0: the message block always runs its exact-f32 kernel (adf_painn_create)
    // The environment switches as adf_painn_create read them (switches.h); a twin holds its parent's.  gemm_f32, msg_f32,
    // lift_on, inc_on start from it and change with their setters; sw.tune.sample_split with adf_painn_set_split.
    adf_switches sw;
    // per-row power-of-two lifts of the f16x3 products' A operands (default on; ADF_LIFT=0 = the unlifted split of rounds 1-2)
    bool lift_on;
    adf_lift lift;       // [3 capN] magnitudes a launcher measures itself
    float *mag_a, *mag_b;  // [capN] magnitudes handed from a producer (LayerNorm, a product's epilogue) to the next product
    float* mag_v3;         // [3 capN] magnitudes of the vec rows entering the heads (measured once, used by both heads)
    bool mag_v3_valid;
    // Row maxima from the producers (sw.row_maxima: ADF_ROW_MAXIMA, default 1): the message kernel and vec_proj's
    // epilogue emit partial maxima of the rows they write and the layers' measuring passes go.  No atomics, no memsets:
    // every slot has one writer and every row's slots are all written.
    float* rmx_part;       // [H/64 + H/32 + 3 H/64][part_stride]: xpart | catpart | vpart, then dbg_mag [4][part_stride]
    float *xpart, *catpart, *vpart;   // xpart[slice][row], catpart[group][row], vpart[slice][3 row + axis]
    int64_t part_stride;   // capN rounded up to 32 rows: a 128-B line of a slot array has one writing workgroup
    // the rows whose xpart / vpart slots are current: written by the last message launch and not touched since
    const float *part_x, *part_vec;
    int part_n;
    const int32_t* part_dev;
    int dbg_msg_rows, dbg_cat_rows;   // adf_painn_debug_row_maxima: rows of the last emitting message / vec_proj launch
    // adf_painn_debug_row_maxima(which = 4) switches capture on: vec_proj then emits its slots on the public per-layer entry too
    // (nobody reads them there but the hook), and update_layer keeps a copy of the magnitudes it combined for its two
    // products: dbg_mag[0 .. 3 rows) of the vec rows, dbg_mag[3 part_stride ..] of the [x | |v2|] rows
    bool dbg_capture;
    float* dbg_mag;
    int dbg_comb_rows;

    // ---- grow-only workspaces
    int64_t capN, capB, capE;
    int32_t* nbr_cnt;    // [N]
    int32_t* nbr_src;    // [N*K]
    int32_t* nbr_shift;  // [N*K]  index into the lexicographic shift table
    int32_t* deg;        // [N+1] in-degree per target atom (symmetrised graph)
    int32_t* nptr;       // [N+1] exclusive scan = CSR row pointer over targets
    int32_t* cursor;     // [N]   fill cursors
    int32_t* img_cnt;    // [B]   directed edges per image (empty-image check)
    int32_t* sys_slow;   // [B]   1 = the system does not fit the per-system LDS kernels of the CSR build (graph.hip)
    void* scan_tmp;      // hipcub scan workspace
    size_t scan_tmp_bytes;
    // static-atom cache of the top-K kernel (adf_graph_set_moving)
    const int32_t* moving;   // caller-owned [N] mask, null = every atom may move (no cache)
    const int32_t* mov_idx;  // caller-owned: indices of the moving atoms grouped by system
    const int32_t* mov_off;  // caller-owned [B+1]
    float* cache_d2;         // [capN*K]
    int32_t* cache_cid;      // [capN*K]
    int32_t* cache_cnt;      // [capN]
    bool cache_valid;
    int32_t* e_src;      // [capE] source atom of every edge, grouped by target, sorted by distance
    float4* e_geom;      // [capE] (ux,uy,uz,d): unit vector target->source, distance
    // device int32[8], STICKY (only adf_check_flags / adf_graph_build(num_edges) / adf_graph_set_moving clear them):
    // {0 candidate overflow, 1 empty image, 2 edge overflow, 3 in-degree beyond the sorter, 4 atomic number out of
    //  range, 5 non-finite or fp16-range-exceeding activation (gemm16.hip), 6 an edge row without its reverse row
    //  (energy_grad.hip), 7 unused}
    int32_t* flags;
    float *x, *vecA, *vecB, *y, *xh, *vv, *cat, *dot;  // node buffers
    float* rec;          // [(N+1)][H/32][160] gather records of the message kernel (message.hip)
    bool rbf_uniform;    // Gaussian centres are k/(R-1): the message kernel may use its recurrence (ADF_MSG_RBF=direct: never)
    // Layer-0 gather records depend on the atomic numbers only (x0 = emb(Z), vec0 = 0).  While a static-atom
    // promise is in force (adf_graph_set_moving: same batch, only flagged atoms move) they are computed once.
    float* rec0;
    int64_t rec0_cap, rec0_N;
    bool rec0_valid;
    // ---- incremental layers (api.hip forward_incremental, incremental.hip): per-layer node state kept across the
    // forwards of one static-atom promise; a forward recomputes only rows whose inputs changed since they were computed
    bool inc_on;                       // adf_painn_set_incremental / ADF_INCREMENTAL (default on)
    bool inc_valid;                    // the kept state belongs to the current batch, weights and arithmetic
    int64_t inc_capN, inc_N;
    int inc_layers;
    float* incX[ADF_MAX_LAYERS + 1];   // x entering layer l (l = L: entering the heads)   [capN, H]
    float* incV[ADF_MAX_LAYERS + 1];   // vec likewise, l >= 1 (vec entering layer 0 is zero)  [capN, 3, H]
    float* incR[ADF_MAX_LAYERS];       // gather records of layer l  [(capN+1), H/32, 160]
    int32_t *prev_nptr, *prev_src;     // CSR of the previous build (swapped with nptr / e_src / e_geom per build)
    float4* prev_geom;
    unsigned char *inc_c0, *inc_chg;   // [capN] in-edges changed; [2][capN] layer input changed (ping-pong)
    unsigned char *inc_pend, *inc_need, *inc_tf;  // [L][capN] row has unapplied changes / is needed / is recomputed now
    int32_t* inc_list;                 // [L][capN] compacted recompute lists (ascending)
    int32_t* inc_cnt;                  // device [2L+1]: list lengths, in-edges of the listed rows, all edges
    // The list lengths never gate a launch: list-mode kernels are sized for all N rows and read their row count from
    // inc_cnt on the device (rows_dev below).  The host sees the counts one forward late, through a pinned double buffer
    // and an event it polls without waiting, and uses them only to choose between the list and the all-rows form of a
    // layer and for the statistics.  ADF_INC_SYNC=1 (sw.inc_sync): read them back synchronously instead (exact launch sizes).
    int32_t* inc_cnt_host;             // pinned [2][2L+1]
    void* inc_ev[2];                   // hipEvent_t after the copy into inc_cnt_host[slot]
    bool inc_ev_live[2];
    int inc_slot;
    int32_t inc_seen[2 * ADF_MAX_LAYERS + 1];  // the latest counts the host has seen
    bool inc_seen_valid;
    unsigned char inc_pend_whole[2][ADF_MAX_LAYERS];  // per slot: which layers of that forward ran in the all-rows form
    int32_t inc_pend_N[2];
    int32_t inc_pend_Nseen;            // the atom count inc_seen belongs to
    const int32_t* rows_dev;           // device row count of the launches being enqueued (a list-mode layer), else null
    void* inc_tmp; size_t inc_tmp_bytes;  // hipcub select workspace
    unsigned long long inc_rows, inc_rows_full, inc_edges, inc_launches;  // totals since adf_painn_set_incremental
    unsigned long long build_serial, inc_serial;  // graph builds made / the build the kept state belongs to
    float *sub_x, *sub_vec, *sub_f;  // compact rows of adf_painn_forward_subset: [capS,H], [capS,3,H], [capS,3]
    int64_t capS;
    float* sys;          // [B*16] per-system scratch of the stepper
    int32_t* ps_state = nullptr; int32_t ps_B = 0;   // per-system early stop (adf_painn_set_per_system_stop): caller's [B,4]
    // ---- S2EF energy head out_energy = Linear(H, H/2), ScaledSiLU, Linear(H/2, 1) (adf_painn_set_energy_head)
    const float *oe0_w, *oe0_b, *oe2_w, *oe2_b;
    adf_w16 oe0_16;
    unsigned char* oe0_buf;   // hi / lo planes + inverse scale + split scratch of out_energy.0.weight
    bool energy_set;
    const float* x_last;      // node features entering the heads of the last full forward (h->x or the kept incX[L])
    float dist_floor;         // edge distances at or below it are set to it (adf_painn_set_distance_floor, default 1e-3)
    void* grad;               // energy_grad.hip: transposed weight images and workspaces of adf_painn_forward_energy_gradient
    // last graph
    int64_t lastN, lastB;
    int32_t last_reps[3];
    int num_cus;
    // ---- optional HIP-event profiling of the forward (bench.py roofline); see api.hip
    adf_prof prof;
    unsigned long long* kcount;           // device counter: executed k-steps of the message kernel
    // ---- two half-batches on two streams (api.hip adf_sample_split, stepper.hip sample_loop_split)
    adf_painn* twin;                      // a parent: its twin (adf_painn_create_twin), else null
    adf_painn* parent;                    // a twin: the handle whose weight images it reads (never freed here)
    bool split_last;                      // parent: its caches and graph belong to view A of a split run
    int32_t split_cut; int64_t split_N;   // ... of this cut of a batch of this many atoms
    unsigned long long split_runs, split_fallbacks;
    unsigned long long moving_serial, inc_set_serial;     // calls of adf_graph_set_moving / adf_painn_set_incremental
    unsigned long long seen_moving_serial, seen_inc_serial;   // twin: the parent's calls it has followed
    void* split_stream;                   // twin: hipStream_t of view B (non-blocking)
    void* split_ev[2];                    // twin: hipEvent_t fork, join
    int32_t* split_state;                 // twin: device int32[16]: view B's state[8], the caller's state at the fork [8]
    int32_t* split_hist; int64_t split_hist_cap;   // twin: device [2][cap] all-converged flag of every step of A and of B
    // ---- owners of the device buffers above, one per set that lives and dies together
    adf_pool m_life;   // creation to destruction: rbf_pack*, flags, kcount, the w16_* and wfrag arenas, oe0_buf
    adf_pool m_ws;     // the workspaces sized by capN / capB / capE, prev_* and rmx_part included
    adf_pool m_inc;    // incremental layers: incX / incV / incR, inc_*
    adf_pool m_sub;    // sub_x / sub_vec / sub_f
    adf_pool m_rec0;   // rec0
    // ---- adf_painn_forward_observe: scratch of the column-variance operator (scale_fit.hip), grown on demand
    void* obs_scratch = nullptr;
    int64_t obs_bytes = 0;
    adf_pool m_obs;    // obs_scratch
};

enum { ADF_PROF_GRAPH = 0, ADF_PROF_MESSAGE = 1, ADF_PROF_NODE = 2, ADF_PROF_HEADS = 3, ADF_PROF_STEPPER = 4 };
static inline void adf_prof_begin(adf_painn* h, int cat, hipStream_t s) { h->prof.begin(cat, s); }
static inline void adf_prof_end(adf_painn* h, hipStream_t s) { h->prof.end(s); }

// ---- kernels' host launchers (each enqueues on `s`, returns ADF_*)
int32_t adf_launch_gemm(const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc,
                        int M, int N, int K, int act_ssilu, hipStream_t s);
// Callers without a handle (adf_linear_forward, the adf_op_* / tr_* operators of train.hip) take the kernel selection from
// adf_switches_process().tune (switches.h) and the CU count of the current device from adf_current_num_cus().
int adf_current_num_cus();
// C = act(A W^T + bias) with EPI 0's operands in *ep (null: the plain product): A2 / K1, rmag (the A rows' magnitudes are
// already known: written by the producer of A - LayerNorm, a previous product's out_mag), out_mag (emit the output rows'
// magnitudes; zeroed here), m_dev, accumulate, gate / gate_ld.  lf: measure the A rows' magnitudes into lf->buf first (row
// lifts, see adf_epi::rmag) unless ep->rmag has them.  num_cus: of the device the launch goes to (tile choice).
int32_t adf_launch_gemm16(const float* A, int lda, const adf_w16* W, const float* bias, float* C, int ldc, int M,
                          int N, int K, int act_ssilu, const adf_epi* ep, hipStream_t s, const adf_lift* lf,
                          const adf_tune& tune, int num_cus);
// m_dev / m_mul: rows = min(M, *m_dev * m_mul) when the count lives on the device (m_mul = 3: [N,3,K] vector rows)
int32_t adf_launch_rowmag(const float* A, int lda, int K1, const float* A2, int K2, long long M, float* mag, hipStream_t s,
                          const int32_t* m_dev = nullptr, int m_mul = 1);
// mag[r] = max over p < nparts of part[p * stride + r], r < M (partial row maxima written by the rows' producers)
int32_t adf_launch_rowmax_combine(const float* part, long long stride, int nparts, long long M, float* mag, hipStream_t s,
                                  const int32_t* m_dev = nullptr, int m_mul = 1);
int32_t adf_split_weight(const float* w, long long n, adf_w16* out, unsigned int* scratch_bits, hipStream_t s,
                         int perm_H = 0, int K = 0, const float* bias = nullptr, int parts = 3);
int32_t adf_launch_gemm16_vecnorm(const float* A, int lda, const adf_w16* W, float* nrm, int M, int N, int K,
                                  hipStream_t s, const adf_tune& tune, const adf_lift* lf = nullptr,
                                  const float* premag = nullptr);
int32_t adf_launch_gemm16_fused(const float* A, int lda, const adf_w16* W, int M, int H, int K, int epi,
                                const adf_epi* ep, hipStream_t s, const adf_tune& tune, const adf_lift* lf = nullptr);
// C = act(A . W^T + b): f16x3 split MFMA by default, exact-f32 MFMA when h->gemm_f32 (ADF_GEMM=f32)
static inline int32_t adf_linear(const adf_painn* h, const float* A, int lda, const float* W, const adf_w16* W16,
                                 const float* bias, float* C, int ldc, int M, int N, int K, int act, hipStream_t s,
                                 const float* premag = nullptr, float* out_mag = nullptr) {
    if (h->gemm_f32) return adf_launch_gemm(A, lda, W, K, bias, C, ldc, M, N, K, act, s);
    adf_epi ep = {};
    ep.m_dev = h->rows_dev;
    if (h->lift_on) { ep.rmag = premag; ep.out_mag = reinterpret_cast<unsigned int*>(out_mag); }
    return adf_launch_gemm16(A, lda, W16, bias, C, ldc, M, N, K, act, &ep, s, h->lift_on ? &h->lift : nullptr, h->sw.tune,
                             h->num_cus);
}
// gemm16.hip: fragment image of a split weight [N, K]
int32_t adf_pack_frag(const adf_w16* w, int N, int K, void* out, hipStream_t s);
int32_t adf_graph_build_impl(adf_painn* h, const adf_batch* b, hipStream_t s);
// api.hip: energy[b] = sum over the system's atoms of (y[a] . w + bias), fixed order (adf_energy_sum_kernel)
int32_t adf_energy_sum(const float* y, int H2, const float* w, const float* bias, const int32_t* atom_offset, float* energy,
                       int num_systems, hipStream_t s);
// energy_grad.hip: state of adf_painn_forward_energy_gradient (invalidate: the bound weights changed)
void adf_grad_invalidate(adf_painn* h);
void adf_grad_free(adf_painn* h);
// message_geo.hip: per-edge-row (dE/dd, dE/du) of a message block, see the kernel comment
bool adf_message_geo_supported(const adf_painn* h);
int32_t adf_message_geo(adf_painn* h, int layer, const float* xh, const float* vec, bool vec_is_zero, float4* part,
                        long long ecap, bool accumulate, hipStream_t s);
// incremental.hip
size_t adf_inc_temp_bytes(int64_t n);
int32_t adf_inc_compare(adf_painn* h, int N, hipStream_t s);  // inc_c0 from (nptr, e_src, e_geom) vs prev_*
int32_t adf_inc_need_from_list(adf_painn* h, int N, int L, const int32_t* out_idx, int n_out, hipStream_t s);
int32_t adf_inc_plan_layer(adf_painn* h, int l, int N, bool first, bool have_need, hipStream_t s);
// n_dev: rows = min(n, *n_dev) (the list length stays on the device)
int32_t adf_inc_scatter_rows(const float* src, const int32_t* idx, int n, int width, float* dst, hipStream_t s,
                             const int32_t* n_dev = nullptr);
int32_t adf_inc_gather_rows(const float* src, const int32_t* idx, int n, int width, float* dst, hipStream_t s);
size_t adf_scan_temp_bytes(int64_t n);
int32_t adf_message_impl(adf_painn* h, int layer, int N, const float* x, const float* xh, const float* vec,
                         float* x_out, float* vec_out, bool vec_is_zero, hipStream_t s,
                         const int32_t* tlist = nullptr, int n_targets = 0, const float* rec = nullptr,
                         const int32_t* n_targets_dev = nullptr,   // n_targets_dev: the list length lives on the device
                         float* xpart = nullptr, float* vpart = nullptr, long long part_stride = 0);  // MsgParams::xpart
int32_t adf_pack_rbf(adf_painn* h, hipStream_t s);
int32_t adf_pack_rbf_layer(adf_painn* h, int l, hipStream_t s);
int32_t adf_pack_records(adf_painn* h, int N, const float* xh, const float* vec, bool vec_is_zero, hipStream_t s,
                         float* rec = nullptr);
int32_t adf_nodewise_embed(adf_painn* h, const int32_t* Z, int N, float* x, hipStream_t s);
int32_t adf_nodewise_layernorm(const float* x, const float* w, const float* b, float* y, int N, int H, hipStream_t s,
                               float* out_mag = nullptr, const int32_t* n_dev = nullptr);  // out_mag: max|y| per row
int32_t adf_nodewise_update_prep(const float* vv, const float* x, float* cat, float* dot, int N, int H, hipStream_t s);
int32_t adf_nodewise_update_apply(const float* h3, const float* dot, const float* vv, float* x, float* vec,
                                  float scale, int N, int H, hipStream_t s);
int32_t adf_head_forward(adf_painn* h, int head, int N, const float* x, const float* vec, float* out, hipStream_t s);
int32_t adf_stepper_init(const adf_batch* b, float* pos, const int32_t* tags, const float* noise,
                         hipStream_t s);
// sys: [16 B] floats of per-system scratch
int32_t adf_stepper_step(float* sys, const adf_batch* b, float* pos, const int32_t* tags, const int32_t* fixed,
                         const float* f1, const float* f2, const adf_step_coef* coef, const adf_step_coef* coefs_dev,
                         int num_steps, const float* z_tr, const float* z_rot, int32_t early_stop_count,
                         int32_t* state, float* dcom, float* drot, hipStream_t s, int32_t* sys_state = nullptr,
                         int32_t* hist_t = nullptr);   // hist_t (coupled rule): receives this step's all-converged flag
// translation-only samplers (reverse_sde_sampling / langevin_dynamics): head-1 mean, dcom = coef * score (+ noise * z),
// wrap, pos += dcom on the adsorbate; same state[] protocol as adf_stepper_step
int32_t adf_stepper_tr_step(float* sys, const adf_batch* b, float* pos, const int32_t* tags, const float* f1,
                            const adf_tr_coef* coef, const adf_tr_coef* coefs_dev, int num_steps, const float* z,
                            int32_t early_stop_count, int32_t* state, float* dcom, hipStream_t s,
                            int32_t* sys_state = nullptr);   // sys_state: the per-system rule (stepper.hip)

// ---- the stepper entries and the fused sampling loop of both score models (stepper.hip).  The model side: api.hip
// (PaiNN) and eqv2_api.hip (EquiformerV2) fill one in for a handle.
struct adf_model {
    void* h;
    int32_t (*check)(void* h, const adf_batch* b);               // the handle's batch check
    int32_t (*grow)(void* h, const adf_batch* b, float** sys);   // grow-only workspaces; *sys = per-system scratch [16 B]
    // forward of all atoms (out_idx null) or of the out_idx rows; f2 null: head 1 alone (translation samplers)
    int32_t (*forward)(void* h, const adf_batch* b, const int32_t* out_idx, int32_t n_out, float* f1, float* f2,
                       hipStream_t s);
    void (*prof)(void* h, bool begin, hipStream_t s);            // time the step under the model's stepper category
    // per-system early stop (adf_*_set_per_system_stop): the caller's [sys_B, 4] int32 table, null = the coupled rule
    int32_t* sys_state;
    int32_t sys_B;
};
// the switch itself: validates and stores into the handle's two fields
int32_t adf_model_set_per_system_stop(int32_t** slot, int32_t* slot_B, int32_t* sys_state, int32_t B);
int32_t adf_frames_push_impl(adf_frames* f, const float* src, hipStream_t s);
// the entries of include/adsorbdiff_hip.h on the handle of `m` (same arguments and contracts)
int32_t adf_model_init_placement(const adf_model& m, const adf_batch* b, float* pos, const int32_t* tags,
                                 const float* noise, hipStream_t s);
int32_t adf_model_sde_step(const adf_model& m, const adf_batch* b, float* pos, const int32_t* tags, const int32_t* fixed,
                           const float* f1, const float* f2, const adf_step_coef* coef, const adf_step_coef* coefs_dev,
                           int32_t num_steps, const float* z_tr, const float* z_rot, int32_t early_stop_count,
                           int32_t* state, float* dcom, float* drot, hipStream_t s, int32_t* hist_t = nullptr);
int32_t adf_model_tr_step(const adf_model& m, const adf_batch* b, float* pos, const int32_t* tags, const float* f1,
                          const adf_tr_coef* coef, const adf_tr_coef* coefs_dev, int32_t num_steps, const float* z,
                          int32_t early_stop_count, int32_t* state, float* dcom, hipStream_t s);
// sink null: adf_[eqv2_]sample, else adf_[eqv2_]sample_traj
int32_t adf_model_sample(const adf_model& m, const adf_batch* b, float* pos, const int32_t* tags, const int32_t* fixed,
                         const adf_step_coef* coefs_dev, int32_t num_steps, const float* z_tr_all, const float* z_rot_all,
                         int32_t early_stop_count, int32_t poll_every, int32_t* state, const int32_t* out_idx,
                         int32_t n_out, float* f1, float* f2, adf_frames* sink, int32_t frame_every, hipStream_t s);
int32_t adf_model_tr_sample(const adf_model& m, const adf_batch* b, float* pos, const int32_t* tags,
                            const adf_tr_coef* coefs_dev, int32_t num_steps, const float* z_all, int32_t early_stop_count,
                            int32_t poll_every, int32_t* state, const int32_t* out_idx, int32_t n_out, float* f1,
                            adf_frames* sink, int32_t frame_every, hipStream_t s);

// ---- two half-batches on two streams (stepper.hip).  One view of a split run: what differs between the two sides.
// Every array is the caller's, offset to the view's first atom / system; nothing is copied.
struct adf_split_side {
    const adf_batch* b;        // the view's batch descriptor (whole-batch reps)
    float* pos;
    const int32_t* tags;
    const int32_t* fixed;
    const int32_t* out_idx;    // re-based to the view's first atom (null: all atoms)
    int32_t n_out;
    float* f1;
    float* f2;
    int32_t* state;            // the view's own state[8]
    int32_t* hist;             // [num_steps] all-converged flag per step (coupled rule), else null
    int32_t sys0;              // the view's first system in the whole batch: its rows of the noise tables
    hipStream_t s;
};
// fork / join: events of the pair; state_init: the caller's state at the fork [8]
int32_t adf_model_sample_split(const adf_model& mA, const adf_model& mB, adf_split_side A, adf_split_side B,
                               const adf_step_coef* coefs_dev, int32_t num_steps, const float* z_tr_all,
                               const float* z_rot_all, int32_t total_systems, int32_t early_stop_count, int32_t poll_every,
                               int32_t* state_init, hipEvent_t fork, hipEvent_t join);
