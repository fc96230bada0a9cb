// C ABI of libadsorbdiff_hip.so: handle life-cycle, grow-only workspaces, and the launch
// sequence of one PaiNN denoiser forward (reference: painn_denoising.py:402-481).
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "common.h"

static thread_local char g_err[512] = "";

void adf_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* adf_last_error(void) { return g_err; }
extern "C" const char* adf_version(void) { return "adsorbdiff_hip 0.5.0 (gfx950)"; }

int adf_current_num_cus() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return n;
}

extern "C" int32_t adf_profile_enable(adf_painn_t h, int32_t on) {
    if (!h) { adf_set_error("null handle"); return ADF_EINVAL; }
    h->prof.enable(on != 0);
    ADF_HIP_CHECK(hipMemset(h->kcount, 0, 8 * sizeof(unsigned long long)));
    if (h->twin) return adf_profile_enable(h->twin, on);
    return ADF_OK;
}

extern "C" int32_t adf_profile_read(adf_painn_t h, float* ms, int64_t* count, int64_t* message_ksteps, void* stream) {
    if (!h || !ms || !count) { adf_set_error("null argument"); return ADF_EINVAL; }
    ADF_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    if (message_ksteps) {
        unsigned long long k[8];
        ADF_HIP_CHECK(hipMemcpy(k, h->kcount, sizeof(k), hipMemcpyDeviceToHost));
        ADF_HIP_CHECK(hipMemset(h->kcount, 0, sizeof(k)));
        *message_ksteps = (int64_t)k[0];
    }
    ADF_TRY(h->prof.read(ms, count, ADF_PROF_NCAT));
    if (h->twin) {   // the pair's profile: sums over both handles (the join has put B's work in front of `stream`'s end)
        float ms2[ADF_PROF_NCAT];
        int64_t count2[ADF_PROF_NCAT], k2 = 0;
        ADF_TRY(adf_profile_read(h->twin, ms2, count2, message_ksteps ? &k2 : nullptr, h->twin->split_stream));
        for (int c = 0; c < ADF_PROF_NCAT; ++c) { ms[c] += ms2[c]; count[c] += count2[c]; }
        if (message_ksteps) *message_ksteps += k2;
    }
    return ADF_OK;
}

extern "C" int32_t adf_painn_create(const adf_painn_hparams* hp, adf_painn_t* out) {
    if (!hp || !out) { adf_set_error("null argument"); return ADF_EINVAL; }
    if (hp->hidden_channels % ADF_SLICE_CH != 0 || hp->hidden_channels < 128 || hp->hidden_channels > 1024) {
        adf_set_error("hidden_channels=%d must be a multiple of %d in [128,1024]", hp->hidden_channels, ADF_SLICE_CH);
        return ADF_EINVAL;
    }
    if (hp->num_rbf % 2 != 0 || hp->num_rbf > 128 || hp->num_rbf < 2) {
        adf_set_error("num_rbf=%d must be even and <= 128", hp->num_rbf);
        return ADF_EINVAL;
    }
    if (hp->max_neighbors < 1 || hp->max_neighbors > ADF_MAX_K) {
        adf_set_error("max_neighbors=%d must be in [1,%d]", hp->max_neighbors, ADF_MAX_K);
        return ADF_EINVAL;
    }
    if (hp->num_layers < 1 || hp->num_layers > 16 || hp->num_heads < 0 || hp->num_heads > 2) {
        adf_set_error("num_layers must be in [1,16], num_heads in [0,2]");
        return ADF_EINVAL;
    }
    adf_painn* h = new (std::nothrow) adf_painn();
    if (!h) { adf_set_error("host allocation failed"); return ADF_EOOM; }
    h->hp = *hp;
    hipDeviceProp_t prop;
    if (hipGetDevice(&h->device) != hipSuccess || hipGetDeviceProperties(&prop, h->device) != hipSuccess) {
        adf_set_error("no usable HIP device: %s", hipGetErrorString(hipGetLastError()));
        adf_painn_destroy(h);
        return ADF_EHIP;
    }
    h->num_cus = prop.multiProcessorCount;
    h->dist_floor = 1.0e-3f;
    h->sw = adf_switches_from_env();
    h->inc_on = h->sw.incremental != 0;   // incremental layers: on unless ADF_INCREMENTAL=0 (adf_painn_set_incremental overrides)
    const int H = hp->hidden_channels, R = hp->num_rbf, L = hp->num_layers;
    adf_pool& m = h->m_life;
    int32_t st = m.alloc(&h->rbf_pack, (size_t)L * (H / ADF_SLICE_CH) * R * 192);
    if (st == ADF_OK) st = m.alloc(&h->rbf_bias_pack, (size_t)L * (H / ADF_SLICE_CH) * 192);
    if (st == ADF_OK) st = m.alloc(&h->rbf_pack16, (size_t)L * (H / ADF_SLICE_CH) * R * 192 * 2 * sizeof(uint16_t));
    if (st == ADF_OK) st = m.alloc(&h->rbf_bias_pack16, (size_t)L * (H / ADF_SLICE_CH) * 192);
    if (st == ADF_OK) st = m.alloc(&h->rbf_scales, 16);
    if (st == ADF_OK) st = m.alloc(&h->flags, ADF_NFLAGS);
    if (st == ADF_OK && hipMemset(h->flags, 0, sizeof(int32_t) * ADF_NFLAGS) != hipSuccess) st = ADF_EHIP;
    {   // fp16 hi/lo arena: per layer 9 H^2 + 2 (H*2H) ... computed exactly below
        const size_t HH = (size_t)H * H;
        const size_t per_layer = HH + 3 * HH + 2 * HH + 2 * HH + 3 * HH;                 // xp0 xp2 vp xv0 xv2
        const size_t per_head = HH + HH / 2 + 2 * HH + HH + HH / 4 + HH / 2;              // b0: vec1 vec2 un0 un2 ; b1: vec1 un0
        const size_t elems = (size_t)L * per_layer + (size_t)hp->num_heads * per_head;
        h->w16_bytes = elems * 2 * sizeof(uint16_t) + 4096;
        if (st == ADF_OK) st = m.alloc(&h->w16_arena, h->w16_bytes);
        if (st == ADF_OK) st = m.alloc(&h->w16_scales, 256);
        if (st == ADF_OK) st = m.alloc(&h->w16_bias_perm, (size_t)L * 2 * 3 * H);
        if (st == ADF_OK) st = m.alloc(&h->w16_scratch, 1);
        if (st == ADF_OK) st = m.alloc(&h->wfrag_arena, h->w16_bytes);
        h->gemm_f32 = h->sw.gemm_f32 != 0;
        h->lift_on = h->sw.lift != 0;
        h->msg_f32 = h->sw.msg_f32 != 0;
        // The f16 message kernel stages its rbf_proj image in 16-byte pieces of 8 basis functions per column: a basis that
        // is no multiple of 8 runs the exact-f32 message kernel (even R, contracted two deep) whatever the arithmetic of
        // the node products.  message_bwd.hip / message_geo.hip carry the same predicate.
        h->msg_f32_only = hp->num_rbf % 8 != 0;
        h->msg_f32 = h->msg_f32 || h->msg_f32_only;
    }
    if (st == ADF_OK) st = m.alloc(&h->kcount, 8);
    if (st == ADF_OK && hipMemset(h->kcount, 0, 8 * sizeof(unsigned long long)) != hipSuccess) st = ADF_EHIP;
    if (st != ADF_OK) { adf_painn_destroy(h); return st; }
    *out = h;
    return ADF_OK;
}

// The owners null the fields they filled; what is reset here is the state that is not memory.
static void inc_free(adf_painn* h) {
    h->m_inc.release();
    h->inc_tmp_bytes = 0;
    h->inc_capN = 0; h->inc_valid = false;
}

static void free_workspaces(adf_painn* h) {
    h->m_ws.release();
    h->inc_valid = false;
    h->scan_tmp_bytes = 0;
    h->lift.cap = 0; h->mag_v3_valid = false;
    h->xpart = h->catpart = h->vpart = nullptr; h->part_stride = 0;
    h->part_x = h->part_vec = nullptr; h->dbg_msg_rows = h->dbg_cat_rows = h->dbg_comb_rows = 0; h->dbg_mag = nullptr;
    h->cache_valid = false;
    h->capN = h->capB = h->capE = 0;
}

extern "C" int32_t adf_painn_destroy(adf_painn_t h) {
    if (!h) return ADF_OK;
    if (h->twin) { adf_set_error("destroy: the handle has a live twin that reads its weight images; destroy the twin first"); return ADF_EINVAL; }
    if (h->parent) {   // a twin: the weight images are the parent's and stay; its own stream and events go
        h->parent->twin = nullptr;
        h->parent->split_last = false;
        if (h->split_stream) { (void)hipStreamSynchronize((hipStream_t)h->split_stream); (void)hipStreamDestroy((hipStream_t)h->split_stream); }
        for (void* e : h->split_ev)
            if (e) (void)hipEventDestroy((hipEvent_t)e);
    }
    if (h->inc_cnt_host) (void)hipHostFree(h->inc_cnt_host);
    for (int i = 0; i < 2; ++i)
        if (h->inc_ev[i]) (void)hipEventDestroy((hipEvent_t)h->inc_ev[i]);
    adf_grad_free(h);
    delete h;   // the owners free the device buffers, the profiler its events
    return ADF_OK;
}

// ---- the twin of a handle (adsorbdiff_hip.h, "Two half-batches, two streams"): a second set of everything a forward
// writes, around the parent's weight images.  The images are fields of the parent that its pools own: the twin holds plain
// copies of the pointers, outside its own pools, so it never frees them.  bound = false: forget them (the parent is re-binding).
static void borrow_weights(adf_painn* t, const adf_painn* p, bool bound) {
    t->emb = p->emb; t->rbf_offset = p->rbf_offset;
    memcpy(t->layer, p->layer, sizeof(t->layer));
    memcpy(t->head, p->head, sizeof(t->head));
    memcpy(t->scale, p->scale, sizeof(t->scale));
    t->rbf_pack = p->rbf_pack; t->rbf_bias_pack = p->rbf_bias_pack; t->rbf_pack16 = p->rbf_pack16;
    t->rbf_bias_pack16 = p->rbf_bias_pack16; t->rbf_scales = p->rbf_scales; t->rbf_uniform = p->rbf_uniform;
    t->w16_arena = p->w16_arena; t->w16_bytes = p->w16_bytes; t->w16_scales = p->w16_scales;
    t->w16_bias_perm = p->w16_bias_perm; t->w16_scratch = p->w16_scratch; t->wfrag_arena = p->wfrag_arena;
    t->weights_set = bound && p->weights_set;
    t->rec0_valid = false;
    t->inc_valid = false;
}
// the parent's switches and arithmetic, as they stand now; a change drops what the twin kept under the old ones
static void follow_settings(adf_painn* t, const adf_painn* p) {
    if (t->gemm_f32 != p->gemm_f32 || t->msg_f32 != p->msg_f32 || t->dist_floor != p->dist_floor || t->lift_on != p->lift_on) {
        t->cache_valid = false; t->rec0_valid = false; t->inc_valid = false;
    }
    t->gemm_f32 = p->gemm_f32; t->msg_f32 = p->msg_f32; t->msg_f32_only = p->msg_f32_only; t->dist_floor = p->dist_floor;
    t->lift_on = p->lift_on; t->sw = p->sw;
}

extern "C" int32_t adf_painn_create_twin(adf_painn_t parent, adf_painn_t* out) {
    if (!parent || !out) { adf_set_error("create_twin: null argument"); return ADF_EINVAL; }
    if (parent->parent) { adf_set_error("create_twin: the handle is a twin itself"); return ADF_EINVAL; }
    if (parent->twin) { adf_set_error("create_twin: the handle already has a twin"); return ADF_EINVAL; }
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != parent->device) {
        adf_set_error("create_twin: the parent lives on device %d, the current device is %d", parent->device, dev);
        return ADF_EINVAL;
    }
    adf_painn* t = new (std::nothrow) adf_painn();
    if (!t) { adf_set_error("host allocation failed"); return ADF_EOOM; }
    t->hp = parent->hp; t->device = parent->device; t->num_cus = parent->num_cus;
    t->inc_on = parent->inc_on;
    follow_settings(t, parent);
    // its own: flags, the k-step counter, view B's state and the stream pair's objects.  No weight image is allocated.
    int32_t st = t->m_life.alloc(&t->flags, ADF_NFLAGS);
    if (st == ADF_OK && hipMemset(t->flags, 0, sizeof(int32_t) * ADF_NFLAGS) != hipSuccess) st = ADF_EHIP;
    if (st == ADF_OK) st = t->m_life.alloc(&t->kcount, 8);
    if (st == ADF_OK && hipMemset(t->kcount, 0, 8 * sizeof(unsigned long long)) != hipSuccess) st = ADF_EHIP;
    if (st == ADF_OK) st = t->m_life.alloc(&t->split_state, 16);
    if (st == ADF_OK && hipStreamCreateWithFlags(reinterpret_cast<hipStream_t*>(&t->split_stream), hipStreamNonBlocking) != hipSuccess) st = ADF_EHIP;
    for (int i = 0; i < 2 && st == ADF_OK; ++i)
        if (hipEventCreateWithFlags(reinterpret_cast<hipEvent_t*>(&t->split_ev[i]), hipEventDisableTiming) != hipSuccess) st = ADF_EHIP;
    if (st != ADF_OK) {
        if (st == ADF_EHIP) adf_set_error("create_twin: %s", hipGetErrorString(hipGetLastError()));
        t->parent = parent;       // (so that the destroy below releases the stream and the events)
        parent->twin = t;
        adf_painn_destroy(t);
        return st;
    }
    borrow_weights(t, parent, true);
    t->prof.enable(parent->prof.on);
    t->parent = parent;
    parent->twin = t;
    *out = t;
    return ADF_OK;
}

extern "C" int32_t adf_painn_set_split(adf_painn_t h, int32_t on) {
    if (!h) { adf_set_error("null handle"); return ADF_EINVAL; }
    h->sw.tune.sample_split = on != 0;
    return ADF_OK;
}

extern "C" int32_t adf_split_stats(adf_painn_t h, int64_t* split_runs, int64_t* fallback_runs) {
    if (!h) { adf_set_error("null handle"); return ADF_EINVAL; }
    if (split_runs) *split_runs = (int64_t)h->split_runs;
    if (fallback_runs) *fallback_runs = (int64_t)h->split_fallbacks;
    return ADF_OK;
}

// A parent that ran view A of a split run holds a graph cache, layer-0 records and kept layer state of that view, under the
// same static-atom promise as the whole batch: before it runs anything else they go.
static void leave_split(adf_painn* h) {
    if (!h || !h->split_last) return;
    h->split_last = false;
    h->cache_valid = false; h->rec0_valid = false; h->inc_valid = false;
}

extern "C" int32_t adf_painn_set_weights(adf_painn_t h, int32_t n_weights, const void* const* w,
                                         const float* scale_factors, void* stream) {
    if (!h || !w || !scale_factors) { adf_set_error("null argument"); return ADF_EINVAL; }
    if (h->parent) { adf_set_error("set_weights: a twin reads its parent's weights; bind them there"); return ADF_EINVAL; }
    if (h->twin) borrow_weights(h->twin, h, false);   // whatever happens below, the twin trusts nothing it borrowed before
    const int L = h->hp.num_layers;
    const int expect = 2 + ADF_WEIGHTS_PER_LAYER * L + ADF_WEIGHTS_PER_HEAD * h->hp.num_heads;
    if (n_weights != expect) {
        adf_set_error("expected %d weight tensors, got %d", expect, n_weights);
        return ADF_EINVAL;
    }
    for (int i = 0; i < n_weights; ++i)
        if (!w[i]) { adf_set_error("weight %d is null", i); return ADF_EINVAL; }
    auto f = [&](int i) { return reinterpret_cast<const float*>(w[i]); };
    h->emb = f(0);
    h->rbf_offset = f(1);
    int k = 2;
    for (int l = 0; l < L; ++l) {
        adf_layer_weights& lw = h->layer[l];
        lw.ln_w = f(k++); lw.ln_b = f(k++); lw.xp0_w = f(k++); lw.xp0_b = f(k++); lw.xp2_w = f(k++); lw.xp2_b = f(k++);
        lw.rbf_w = f(k++); lw.rbf_b = f(k++); lw.vp_w = f(k++); lw.xv0_w = f(k++); lw.xv0_b = f(k++);
        lw.xv2_w = f(k++); lw.xv2_b = f(k++);
        h->scale[l] = scale_factors[l];
    }
    for (int hd = 0; hd < h->hp.num_heads; ++hd)
        for (int b = 0; b < 2; ++b) {
            adf_block_weights& bw = h->head[hd][b];
            bw.vec1_w = f(k++); bw.vec2_w = f(k++); bw.un0_w = f(k++); bw.un0_b = f(k++); bw.un2_w = f(k++);
            bw.un2_b = f(k++);
        }
    ADF_TRY(adf_pack_rbf(h, (hipStream_t)stream));
    {   // split every GEMM weight into fp16 hi/lo (gemm16.hip)
        hipStream_t s = (hipStream_t)stream;
        const long long H = h->hp.hidden_channels, HH = H * H;
        unsigned char* cur = h->w16_arena;
        unsigned char* fcur = h->wfrag_arena;
        int nscale = 0;
        float* bperm = h->w16_bias_perm;
        // w [rows, K] -> hi / lo planes (+ the permutations of the fused layers) and their fragment-ordered image
        auto split = [&](const float* w, long long rows, long long K, adf_w16* out, const float* fused_bias = nullptr,
                         bool pair_perm = false) -> int32_t {
            const long long n = rows * K;
            out->hi = cur; cur += n * 2;
            out->lo = cur; cur += n * 2;
            out->inv_scale = h->w16_scales + nscale++;
            out->bias_perm = nullptr;
            out->frag = nullptr;
            if (fused_bias) {  // 3H-wide layer feeding a fused epilogue: rows permuted (gemm16.hip)
                out->bias_perm = bperm; bperm += 3 * H;
                ADF_TRY(adf_split_weight(w, n, out, h->w16_scratch, s, (int)H, (int)H, fused_bias));
            } else if (pair_perm) {  // vec_proj [2H, H]: (v1, v2) rows of the same channels side by side (gemm16.hip EPI 3)
                ADF_TRY(adf_split_weight(w, n, out, h->w16_scratch, s, (int)H, (int)H, nullptr, 2));
            } else {
                ADF_TRY(adf_split_weight(w, n, out, h->w16_scratch, s));
            }
            if (rows % 32 == 0 && K % 16 == 0) {
                out->frag = fcur; fcur += n * 4;
                ADF_TRY(adf_pack_frag(out, (int)rows, (int)K, out->frag, s));
            }
            return ADF_OK;
        };
        for (int l = 0; l < L; ++l) {
            adf_layer_weights& lw = h->layer[l];
            ADF_TRY(split(lw.xp0_w, H, H, &lw.xp0_16));
            ADF_TRY(split(lw.xp2_w, 3 * H, H, &lw.xp2_16, lw.xp2_b));
            ADF_TRY(split(lw.vp_w, 2 * H, H, &lw.vp_16, nullptr, true));
            ADF_TRY(split(lw.xv0_w, H, 2 * H, &lw.xv0_16));
            ADF_TRY(split(lw.xv2_w, 3 * H, H, &lw.xv2_16, lw.xv2_b));
        }
        for (int hd = 0; hd < h->hp.num_heads; ++hd) {
            adf_block_weights& b0 = h->head[hd][0];
            adf_block_weights& b1 = h->head[hd][1];
            ADF_TRY(split(b0.vec1_w, H, H, &b0.vec1_16));
            ADF_TRY(split(b0.vec2_w, H / 2, H, &b0.vec2_16));
            ADF_TRY(split(b0.un0_w, H, 2 * H, &b0.un0_16));
            ADF_TRY(split(b0.un2_w, H, H, &b0.un2_16));
            ADF_TRY(split(b1.vec1_w, H / 2, H / 2, &b1.vec1_16));
            ADF_TRY(split(b1.un0_w, H / 2, H, &b1.un0_16));
        }
        if ((size_t)(cur - h->w16_arena) > h->w16_bytes || (size_t)(fcur - h->wfrag_arena) > h->w16_bytes || nscale > 256) {
            adf_set_error("internal: fp16 weight arena overflow");
            return ADF_EINVAL;
        }
    }
    h->weights_set = true;
    h->rec0_valid = false;
    h->inc_valid = false;
    adf_grad_invalidate(h);
    if (h->twin) borrow_weights(h->twin, h, true);
    return ADF_OK;
}

// grow-only workspaces for N atoms in B systems
static int32_t ensure_capacity(adf_painn* h, int64_t N, int64_t B) {
    if (N <= h->capN && B <= h->capB) return ADF_OK;
    const int64_t capN = N > h->capN ? N : h->capN;
    const int64_t capB = B > h->capB ? B : h->capB;
    // synchronise before freeing buffers that enqueued work may still use
    ADF_HIP_CHECK(hipDeviceSynchronize());
    free_workspaces(h);
    const int64_t H = h->hp.hidden_channels, K = h->hp.max_neighbors;
    // symmetrised edges: every directed top-K entry (j -> i) survives at most once (j < i, or a
    // self image with a negative shift) and is then doubled: E <= 2*N*K.
    const int64_t capE = 2 * capN * K;
    int32_t st = ADF_OK;
#define ALLOC(field, count) if (st == ADF_OK) st = h->m_ws.alloc(&h->field, (size_t)(count))
    ALLOC(nbr_cnt, capN);
    ALLOC(nbr_src, capN * K);
    ALLOC(nbr_shift, capN * K);
    ALLOC(cache_d2, capN * K);
    ALLOC(cache_cid, capN * K);
    ALLOC(cache_cnt, capN);
    ALLOC(deg, capN + 1);
    ALLOC(nptr, capN + 1);
    ALLOC(cursor, capN);
    ALLOC(img_cnt, capB);
    ALLOC(sys_slow, capB);
    ALLOC(e_src, capE);
    ALLOC(e_geom, capE);
    if (h->inc_on) {  // previous build's CSR (incremental layers); swapped with the live one per build
        ALLOC(prev_nptr, capN + 1);
        ALLOC(prev_src, capE);
        ALLOC(prev_geom, capE);
    }
    if (st == ADF_OK) {
        h->scan_tmp_bytes = adf_scan_temp_bytes(capN + 1);
        st = h->m_ws.alloc(&h->scan_tmp, h->scan_tmp_bytes + 16);
    }
    ALLOC(x, capN * H);
    ALLOC(vecA, capN * 3 * H);
    ALLOC(vecB, capN * 3 * H);
    ALLOC(rec, (capN + 1) * 5 * H);  // + one all-zero record row: gather target of padded edge rows
    ALLOC(y, capN * H);
    ALLOC(xh, capN * 3 * H);
    ALLOC(vv, capN * 6 * H);
    ALLOC(cat, capN * 2 * H);
    ALLOC(dot, capN * H);
    ALLOC(sys, capB * 16);
    ALLOC(lift.buf, capN * 3);
    ALLOC(mag_a, capN);
    ALLOC(mag_b, capN);
    ALLOC(mag_v3, capN * 3);
    const int64_t ps = (capN + 31) / 32 * 32, ns = H / ADF_SLICE_CH;
    if (h->sw.row_maxima) ALLOC(rmx_part, (4 * ns + H / 32 + 4) * ps);
#undef ALLOC
    h->lift.cap = st == ADF_OK ? capN * 3 : 0;
    if (st != ADF_OK) { free_workspaces(h); return st; }
    if (h->sw.row_maxima) {   // xpart and catpart side by side: the [x | |v2|] rows' maxima are one run of parts
        h->part_stride = ps;
        h->xpart = h->rmx_part; h->catpart = h->xpart + ns * ps; h->vpart = h->catpart + (H / 32) * ps;
        h->dbg_mag = h->vpart + 3 * ns * ps;
    }
    h->capN = capN; h->capB = capB; h->capE = capE;
    return ADF_OK;
}

static int32_t check_batch(const adf_painn* h, const adf_batch* b) {
    if (!h || !b) { adf_set_error("null argument"); return ADF_EINVAL; }
    if (b->num_atoms <= 0 || b->num_systems <= 0) { adf_set_error("empty batch"); return ADF_EINVAL; }
    if (!b->pos || !b->cell || !b->batch || !b->atom_offset) { adf_set_error("null batch array"); return ADF_EINVAL; }
    for (int k = 0; k < 3; ++k)
        if (b->reps[k] < 0 || b->reps[k] > 16) { adf_set_error("reps[%d]=%d out of range", k, b->reps[k]); return ADF_EINVAL; }
    return ADF_OK;
}

// The flags are sticky on the device: kernels only ever set them, so a condition raised at any step of a sampling
// loop survives until it is read here (which clears them).
static int32_t read_flags(adf_painn* h, hipStream_t s) {
    int32_t f[ADF_NFLAGS];
    ADF_HIP_CHECK(hipMemcpyAsync(f, h->flags, sizeof(f), hipMemcpyDeviceToHost, s));
    ADF_HIP_CHECK(hipMemsetAsync(h->flags, 0, sizeof(f), s));
    int32_t f2[ADF_NFLAGS] = {};
    if (h->twin) {   // the pair's flags are one set: a split run has joined view B's stream into `s`
        ADF_HIP_CHECK(hipMemcpyAsync(f2, h->twin->flags, sizeof(f2), hipMemcpyDeviceToHost, s));
        ADF_HIP_CHECK(hipMemsetAsync(h->twin->flags, 0, sizeof(f2), s));
    }
    ADF_HIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < ADF_NFLAGS; ++i) f[i] |= f2[i];
    if (f[4]) { adf_set_error("atomic number outside [1, %d] (rows of the embedding table)", h->hp.num_elements); return ADF_EINVAL; }
    if (f[0]) { adf_set_error("a centre atom has more than %d in-cutoff candidates", ADF_MAX_CAND); return ADF_EOVERFLOW; }
    if (f[2]) { adf_set_error("edge buffer overflow"); return ADF_EOVERFLOW; }
    if (f[3]) { adf_set_error("an atom has more than %d incoming edges", ADF_MAX_INDEG); return ADF_EOVERFLOW; }
    if (f[1]) { adf_set_error("An image has no neighbors"); return ADF_ENONEIGHBOR; }
    if (f[6]) { adf_set_error("energy gradient: an edge row has no reverse row in its partner's segment (asymmetric graph)"); return ADF_EINVAL; }
    if (f[5]) {
        adf_set_error("non-finite model output%s", h->gemm_f32 ? " (exact-f32 arithmetic: the inputs or weights are not finite)"
                      : " in f16x3 arithmetic: an activation left the fp16 range or the inputs are not finite; "
                        "adf_painn_set_arithmetic(h, 1) selects exact f32");
        return ADF_ENUMERIC;
    }
    return ADF_OK;
}

extern "C" int32_t adf_graph_set_moving(adf_painn_t h, const int32_t* moving, const int32_t* mov_idx,
                                        const int32_t* mov_off) {
    if (!h) { adf_set_error("null handle"); return ADF_EINVAL; }
    if (moving && (!mov_idx || !mov_off)) { adf_set_error("moving mask needs mov_idx and mov_off"); return ADF_EINVAL; }
    h->moving = moving; h->mov_idx = mov_idx; h->mov_off = mov_off;
    ++h->moving_serial;
    ADF_HIP_CHECK(hipMemset(h->flags, 0, sizeof(int32_t) * ADF_NFLAGS));  // a new promise starts with clean flags
    h->cache_valid = false;
    h->rec0_valid = false;
    h->inc_valid = false;
    return ADF_OK;
}

extern "C" int32_t adf_graph_build(adf_painn_t h, const adf_batch* b, void* stream, int64_t* num_edges) {
    ADF_TRY(check_batch(h, b));
    leave_split(h);
    ADF_TRY(ensure_capacity(h, b->num_atoms, b->num_systems));
    hipStream_t s = (hipStream_t)stream;
    ADF_TRY(adf_graph_build_impl(h, b, s));
    if (num_edges) {
        int32_t e = 0;
        ADF_HIP_CHECK(hipMemcpyAsync(&e, h->nptr + b->num_atoms, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        ADF_TRY(read_flags(h, s));
        *num_edges = e;
    }
    return ADF_OK;
}

__global__ void adf_export_edges_kernel(const int32_t* nptr, const int32_t* e_src, const float4* eg, int N,
                                        int32_t* src, int32_t* dst, float* dist, float* vec, long long cap) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    for (int e = nptr[n] + (threadIdx.x & 63); e < nptr[n + 1]; e += 64) {
        if (e >= cap) continue;
        if (src) src[e] = e_src[e];
        if (dst) dst[e] = n;
        const float4 q = eg[e];
        if (dist) dist[e] = q.w;
        if (vec) { vec[3 * (size_t)e] = q.x; vec[3 * (size_t)e + 1] = q.y; vec[3 * (size_t)e + 2] = q.z; }
    }
}

__global__ void adf_export_shift_kernel(const int32_t* nbr_shift, int32_t* out, long long n, int r0, int r1, int r2) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = nbr_shift[i];
    const int n2 = 2 * r2 + 1, n1 = 2 * r1 + 1;
    const int ia = c / (n1 * n2), rem = c - ia * (n1 * n2);
    out[3 * i] = ia - r0;
    out[3 * i + 1] = rem / n2 - r1;
    out[3 * i + 2] = rem % n2 - r2;
}

extern "C" int32_t adf_graph_export(adf_painn_t h, int32_t* nbr_count, int32_t* nbr_src, int32_t* nbr_shift,
                                    int64_t edge_capacity, int32_t* edge_src, int32_t* edge_dst, float* edge_dist,
                                    float* edge_vec, int64_t* num_edges, void* stream) {
    if (!h || h->lastN <= 0) { adf_set_error("no graph built"); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = h->lastN, K = h->hp.max_neighbors;
    if (nbr_count) ADF_HIP_CHECK(hipMemcpyAsync(nbr_count, h->nbr_cnt, sizeof(int32_t) * N, hipMemcpyDeviceToDevice, s));
    if (nbr_src) ADF_HIP_CHECK(hipMemcpyAsync(nbr_src, h->nbr_src, sizeof(int32_t) * N * K, hipMemcpyDeviceToDevice, s));
    if (nbr_shift)
        hipLaunchKernelGGL(adf_export_shift_kernel, dim3((unsigned)((N * K + 255) / 256)), dim3(256), 0, s, h->nbr_shift,
                           nbr_shift, (long long)(N * K), h->last_reps[0], h->last_reps[1], h->last_reps[2]);
    if (edge_src || edge_dst || edge_dist || edge_vec)
        hipLaunchKernelGGL(adf_export_edges_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, h->nptr, h->e_src,
                           h->e_geom, (int)N, edge_src, edge_dst, edge_dist, edge_vec, (long long)edge_capacity);
    ADF_HIP_CHECK(hipGetLastError());
    int32_t e = 0;
    ADF_HIP_CHECK(hipMemcpyAsync(&e, h->nptr + N, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ADF_HIP_CHECK(hipStreamSynchronize(s));
    if (num_edges) *num_edges = e;
    return ADF_OK;
}

// Record row N is the all-zero gather target of padded edge rows (message.hip); rows beyond the
// current N may hold data of an earlier, larger batch, so it is re-zeroed per forward.
static int32_t zero_pad_rows(adf_painn* h, int N, hipStream_t s) {
    const size_t row = (size_t)5 * h->hp.hidden_channels;
    ADF_HIP_CHECK(hipMemsetAsync(h->rec + (size_t)N * row, 0, sizeof(float) * row, s));
    return ADF_OK;
}

// Gather records of layer l for the n rows (x, vec): xh = x_proj(LayerNorm(x)) (painn_denoising.py:531), packed with
// vec for the message kernel.  row_map != null: row r of (x, vec) is atom row_map[r] of the record table.
static int32_t make_records(adf_painn* h, int l, int n, const float* x, const float* vec, bool vec_is_zero, float* rec,
                            const int32_t* row_map, hipStream_t s) {
    const int H = h->hp.hidden_channels;
    const adf_layer_weights& w = h->layer[l];
    if (n <= 0) return ADF_OK;
    adf_prof_begin(h, ADF_PROF_NODE, s);
    const bool lift = h->lift_on && !h->gemm_f32;
    const bool em = lift && h->sw.tune.lift_emit;
    // row magnitudes travel with the rows: LayerNorm -> x_proj.0 -> (its epilogue) -> x_proj.2
    ADF_TRY(adf_nodewise_layernorm(x, w.ln_w, w.ln_b, h->y, n, H, s, em ? h->mag_a : nullptr, h->rows_dev));
    ADF_TRY(adf_linear(h, h->y, H, w.xp0_w, &w.xp0_16, w.xp0_b, h->cat, H, n, H, H, 1, s, em ? h->mag_a : nullptr,
                       em ? h->mag_b : nullptr));
    if (h->gemm_f32) {
        if (row_map) { adf_set_error("internal: mapped records need the f16x3 path"); return ADF_EINVAL; }
        ADF_TRY(adf_launch_gemm(h->cat, H, w.xp2_w, H, w.xp2_b, h->xh, 3 * H, n, 3 * H, H, 0, s));
        ADF_TRY(adf_pack_records(h, n, h->xh, vec, vec_is_zero, s, rec));
    } else {  // x_proj.2 with the gather records written from the accumulators (xh never materialised)
        adf_epi ep = {};
        ep.vec_in = vec; ep.rec = rec ? rec : h->rec; ep.H = H; ep.vec_is_zero = vec_is_zero ? 1 : 0;
        ep.row_map = row_map;
        ep.rmag = em ? h->mag_b : nullptr;
        ep.m_dev = h->rows_dev;
        ADF_TRY(adf_launch_gemm16_fused(h->cat, H, &w.xp2_16, n, H, H, 1, &ep, s, h->sw.tune, lift ? &h->lift : nullptr));
    }
    adf_prof_end(h, s);
    return ADF_OK;
}

// tlist != null: only the listed targets are evaluated and x_out / vec_out are compact [n_targets, ...] rows
// rec != null: gather records go to / come from this buffer instead of h->rec; records_ready: they are already there
static int32_t message_layer(adf_painn* h, int l, int N, const float* x, const float* vec, float* x_out,
                             float* vec_out, bool vec_is_zero, hipStream_t s, const int32_t* tlist = nullptr,
                             int n_targets = 0, float* rec = nullptr, bool records_ready = false) {
    if (!records_ready) ADF_TRY(make_records(h, l, N, x, vec, vec_is_zero, rec, nullptr, s));
    adf_prof_begin(h, ADF_PROF_MESSAGE, s);
    // the f16x3 kernel also leaves the partial maxima of its output rows for update_layer's products (MsgParams::xpart)
    const int items = tlist ? n_targets : N;
    const bool emit = h->sw.row_maxima && h->lift_on && !h->gemm_f32 && !h->msg_f32 && items > 0 && items <= h->part_stride;
    h->part_x = h->part_vec = nullptr;
    const int32_t st = adf_message_impl(h, l, N, x, h->xh, vec, x_out, vec_out, vec_is_zero, s, tlist, n_targets, rec,
                                        tlist ? h->rows_dev : nullptr, emit ? h->xpart : nullptr, h->vpart, h->part_stride);
    if (st == ADF_OK && emit) {
        h->part_x = x_out; h->part_vec = vec_out; h->part_n = items; h->part_dev = tlist ? h->rows_dev : nullptr;
        h->dbg_msg_rows = items;
    }
    adf_prof_end(h, s);
    return st;
}

// from_message: (x, vec) are the rows the last message_layer call wrote, untouched since.  (Rows the caller owns - the
// public per-layer entry - may have been rewritten between the two calls: never trusted, their maxima are measured.)
static int32_t update_layer(adf_painn* h, int l, int N, float* x, float* vec, hipStream_t s, bool from_message = true) {
    const int H = h->hp.hidden_channels;
    const adf_layer_weights& w = h->layer[l];
    adf_prof_begin(h, ADF_PROF_NODE, s);
    // are the partial maxima of exactly these rows current?  They are consumed here: the rows are rewritten in place below.
    const bool parts = from_message && h->sw.row_maxima && h->lift_on && !h->gemm_f32 && N > 0 && h->part_x == x && h->part_vec == vec &&
                       h->part_n == N && h->part_dev == h->rows_dev;
    h->part_x = h->part_vec = nullptr;
    if (h->gemm_f32) {
        ADF_TRY(adf_launch_gemm(vec, H, w.vp_w, H, nullptr, h->vv, 2 * H, 3 * N, 2 * H, H, 0, s));
        ADF_TRY(adf_nodewise_update_prep(h->vv, x, h->cat, h->dot, N, H, s));
        ADF_TRY(adf_linear(h, h->cat, 2 * H, w.xv0_w, &w.xv0_16, w.xv0_b, h->y, H, N, H, 2 * H, 1, s));
    } else {  // vec_proj with dot and |v2| formed on the accumulators (v1 -> vv [N,3,H], |v2| -> cat [N,H]);
              // xvec_proj.0 then reads its [x | |v2|] input from the two arrays
        adf_epi ep = {};
        ep.v1 = h->vv; ep.dotw = h->dot; ep.cat = h->cat; ep.H = H; ep.m_dev = h->rows_dev;
        const adf_lift* lf = h->lift_on ? &h->lift : nullptr;
        // The magnitudes of the vec rows and of the [x | |v2|] rows come from the rows' producers: the message kernel and
        // vec_proj's epilogue each leave the maximum over the columns they own in a slot of their own (plain stores, nothing
        // to zero) and adf_rowmax_combine_kernel takes the maximum over a row's 8 resp. 24 slots - 6 + 19 MB per layer of
        // 200k rows where the two measuring passes (adf_rowmag_kernel) read 1.23 + 0.82 GB.  A maximum is exact, so the lifts
        // and with them every bit of the results are the same.  ADF_ROW_MAXIMA=0, and rows that did not come from the
        // message kernel (from_message), keep the passes.  xvec_proj.0 hands its output rows' magnitudes on as before.
        // (Earlier form of the same fusion, measured and dropped: 4 atomicMax per target and channel slice from the message
        // kernel into a zeroed array - measuring passes -11 ms, message kernel +9 ms per 10 full steps of 1000 systems: a
        // wash.  Float atomics execute at the memory side and stay in the wave's in-order vmcnt in front of every younger
        // gather; the plain stores here do not.)
        // The heads keep their five passes per step: their vec / x rows come out of the kept per-layer tables, which mix
        // rows computed in different steps, so no launch of this step holds a whole table's maxima.
        if (parts) {
            ADF_TRY(adf_launch_rowmax_combine(h->vpart, 3 * h->part_stride, H / ADF_SLICE_CH, 3ll * N, h->lift.buf, s, h->rows_dev, 3));
            ep.rmag = h->lift.buf;
            if (h->dbg_capture) ADF_HIP_CHECK(hipMemcpyAsync(h->dbg_mag, h->lift.buf, sizeof(float) * 3 * (size_t)N, hipMemcpyDeviceToDevice, s));
        }
        // vec_proj stores its |v2| slots only where somebody reads them: the combine below, or the test hook (dbg_capture)
        if (parts || (h->dbg_capture && h->sw.row_maxima && lf && N <= h->part_stride)) {
            ep.catpart = h->catpart; ep.part_stride = h->part_stride; h->dbg_cat_rows = N;
        }
        ADF_TRY(adf_launch_gemm16_fused(vec, H, &w.vp_16, N, H, H, 3, &ep, s, h->sw.tune, lf));
        if (parts) {   // [x | |v2|]: xpart and catpart lie side by side
            ADF_TRY(adf_launch_rowmax_combine(h->xpart, h->part_stride, H / ADF_SLICE_CH + H / 32, N, h->lift.buf, s, h->rows_dev, 1));
            if (h->dbg_capture) {
                ADF_HIP_CHECK(hipMemcpyAsync(h->dbg_mag + 3 * h->part_stride, h->lift.buf, sizeof(float) * (size_t)N, hipMemcpyDeviceToDevice, s));
                h->dbg_comb_rows = N;
            }
        }
        adf_epi e0 = {};   // xvec_proj.0 on [x | |v2|]; its output rows' magnitudes go on to xvec_proj.2
        e0.A2 = h->cat; e0.K1 = H; e0.m_dev = h->rows_dev;
        e0.rmag = parts ? h->lift.buf : nullptr;
        e0.out_mag = h->lift_on ? reinterpret_cast<unsigned int*>(h->mag_b) : nullptr;
        ADF_TRY(adf_launch_gemm16(x, H, &w.xv0_16, w.xv0_b, h->y, H, N, H, 2 * H, 1, &e0, s, lf, h->sw.tune, h->num_cus));
    }
    int32_t st;
    if (h->gemm_f32) {
        ADF_TRY(adf_launch_gemm(h->y, H, w.xv2_w, H, w.xv2_b, h->xh, 3 * H, N, 3 * H, H, 0, s));
        st = adf_nodewise_update_apply(h->xh, h->dot, h->vv, x, vec, h->scale[l], N, H, s);
    } else {  // xvec_proj.2 with gating + residuals + ScaleFactor applied on the accumulators
        adf_epi ep = {};
        ep.x = x; ep.vec = vec; ep.dot = h->dot; ep.vv = h->vv; ep.scale = h->scale[l]; ep.H = H;
        ep.rmag = h->lift_on ? h->mag_b : nullptr;
        ep.m_dev = h->rows_dev;
        st = adf_launch_gemm16_fused(h->y, H, &w.xv2_16, N, H, H, 2, &ep, s, h->sw.tune);
    }
    adf_prof_end(h, s);
    return st;
}

extern "C" int32_t adf_painn_message_layer(adf_painn_t h, int32_t layer, int32_t N, const float* x, const float* vec,
                                           float* x_out, float* vec_out, void* stream) {
    if (!h || !h->weights_set || layer < 0 || layer >= h->hp.num_layers || N != h->lastN) {
        adf_set_error("message_layer: bad handle/layer, or N differs from the built graph");
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    ADF_TRY(zero_pad_rows(h, N, s));
    ADF_TRY(message_layer(h, layer, N, x, vec, x_out, vec_out, false, s));
    return ADF_OK;
}

extern "C" int32_t adf_painn_update_layer(adf_painn_t h, int32_t layer, int32_t N, float* x, float* vec, void* stream) {
    if (!h || !h->weights_set || layer < 0 || layer >= h->hp.num_layers) {
        adf_set_error("update_layer: bad handle/layer");
        return ADF_EINVAL;
    }
    ADF_TRY(ensure_capacity(h, N, 1));
    return update_layer(h, layer, N, x, vec, (hipStream_t)stream, false);
}

// Test hook: the kernel selection the handle holds (read from the environment by adf_painn_create)
extern "C" int32_t adf_painn_get_tune(adf_painn_t h, adf_tune* out) {
    if (!h || !out) { adf_set_error("get_tune: null handle or output"); return ADF_EINVAL; }
    *out = h->sw.tune;
    return ADF_OK;
}

// Test hook: the row maxima as the producers of the last launch left them, combined over their slots.  which = 0: max|x_out|
// [rows] and 1: max|vec_out| [3 rows] of the last message launch; 2: max |v2| [rows] of the last vec_proj launch; 3: the
// |v2| rows themselves [rows, H].  4: capture on (capacity != 0) / off, nothing returned: vec_proj emits its slots on the public
// per-layer entry too and update_layer keeps what it combined; 5 / 6: the magnitudes of the vec rows [3 rows] / of the
// [x | |v2|] rows [rows] exactly as the last update_layer that took them from the slots handed them to its products.
// *rows receives the row count; out (device, may be null to query rows) holds `capacity` floats.
extern "C" int32_t adf_painn_debug_row_maxima(adf_painn_t h, int32_t which, float* out, int64_t capacity, int32_t* rows,
                                              void* stream) {
    if (!h || which < 0 || which > 6) { adf_set_error("debug_row_maxima: null handle or which outside 0..6"); return ADF_EINVAL; }
    if (which == 4) { h->dbg_capture = capacity != 0; h->dbg_comb_rows = 0; return ADF_OK; }
    const int H = h->hp.hidden_channels, ns = H / ADF_SLICE_CH;
    const int n = which <= 1 ? h->dbg_msg_rows : which <= 3 ? h->dbg_cat_rows : h->dbg_comb_rows;
    if (!h->rmx_part || n <= 0) { adf_set_error("debug_row_maxima: no launch has emitted row maxima (ADF_ROW_MAXIMA=0?)"); return ADF_EINVAL; }
    if (rows) *rows = n;
    if (!out) return ADF_OK;
    const int64_t need = (which == 1 || which == 5) ? 3ll * n : which == 3 ? (int64_t)n * H : n;
    if (capacity < need) { adf_set_error("debug_row_maxima: out holds %lld floats, need %lld", (long long)capacity, (long long)need); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    if (which == 0) return adf_launch_rowmax_combine(h->xpart, h->part_stride, ns, n, out, s);
    if (which == 1) return adf_launch_rowmax_combine(h->vpart, 3 * h->part_stride, ns, 3ll * n, out, s);
    if (which == 2) return adf_launch_rowmax_combine(h->catpart, h->part_stride, H / 32, n, out, s);
    if (which >= 5) {
        ADF_HIP_CHECK(hipMemcpyAsync(out, h->dbg_mag + (which == 5 ? 0 : 3 * h->part_stride), sizeof(float) * (size_t)need, hipMemcpyDeviceToDevice, s));
        return ADF_OK;
    }
    ADF_HIP_CHECK(hipMemcpyAsync(out, h->cat, sizeof(float) * (size_t)n * H, hipMemcpyDeviceToDevice, s));
    return ADF_OK;
}

__global__ void adf_scatter_rows3_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx, int n,
                                         float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3 * n) dst[(size_t)idx[i / 3] * 3 + i % 3] = src[i];
}

// compact rows of a subset forward: sub_x / sub_vec / sub_f for n_out rows
static int32_t ensure_subset(adf_painn* h, int32_t n_out) {
    if (n_out <= h->capS) return ADF_OK;
    const int64_t cap = (int64_t)n_out + n_out / 4 + 64;
    const size_t H = h->hp.hidden_channels;
    h->m_sub.release();
    h->capS = 0;
    ADF_TRY(h->m_sub.alloc(&h->sub_x, (size_t)cap * H));
    ADF_TRY(h->m_sub.alloc(&h->sub_vec, (size_t)cap * 3 * H));
    ADF_TRY(h->m_sub.alloc(&h->sub_f, (size_t)cap * 3));
    h->capS = cap;
    return ADF_OK;
}

// Incremental layers usable for this forward?  0 = no; 1 = yes and the kept state is current; 2 = yes, but every row has
// to be computed.  Allocates the kept state on first use (an allocation failure switches the feature off: the plain
// path needs none of it) and swaps the CSR buffers so that the coming graph build leaves the previous build's CSR in
// prev_*.  The state is marked invalid until forward_incremental has finished: an error on the way (graph overflow,
// launch failure) must not leave rows behind that a later forward would trust.
static int inc_prepare(adf_painn* h, int N) {
    const int L = h->hp.num_layers, H = h->hp.hidden_channels;
    if (!h->inc_on || !h->moving || h->gemm_f32 || h->msg_f32 || L > ADF_MAX_LAYERS || !h->prev_nptr)
        return 0;
    if (N > h->inc_capN) {
        (void)hipDeviceSynchronize();
        inc_free(h);
        const size_t cap = (size_t)N;
        int32_t st = ADF_OK;
        for (int l = 0; l <= L && st == ADF_OK; ++l) {
            st = h->m_inc.alloc(&h->incX[l], cap * H);
            if (st == ADF_OK && l >= 1) st = h->m_inc.alloc(&h->incV[l], cap * 3 * H);
            if (st == ADF_OK && l < L) st = h->m_inc.alloc(&h->incR[l], (cap + 1) * 5 * H);
        }
        if (st == ADF_OK) st = h->m_inc.alloc(&h->inc_c0, cap);
        if (st == ADF_OK) st = h->m_inc.alloc(&h->inc_chg, 2 * cap);
        if (st == ADF_OK) st = h->m_inc.alloc(&h->inc_pend, cap * L);
        if (st == ADF_OK) st = h->m_inc.alloc(&h->inc_need, cap * L);
        if (st == ADF_OK) st = h->m_inc.alloc(&h->inc_tf, cap * L);
        if (st == ADF_OK) st = h->m_inc.alloc(&h->inc_list, cap * L);
        if (st == ADF_OK) st = h->m_inc.alloc(&h->inc_cnt, (size_t)2 * ADF_MAX_LAYERS + 1);
        if (st == ADF_OK) {
            h->inc_tmp_bytes = adf_inc_temp_bytes((int64_t)cap);
            st = h->m_inc.alloc(&h->inc_tmp, h->inc_tmp_bytes + 16);
        }
        if (st == ADF_OK && !h->inc_cnt_host &&
            hipHostMalloc(reinterpret_cast<void**>(&h->inc_cnt_host), sizeof(int32_t) * 2 * (2 * ADF_MAX_LAYERS + 1)) != hipSuccess)
            st = ADF_EOOM;
        for (int i = 0; i < 2 && st == ADF_OK; ++i)
            if (!h->inc_ev[i] && hipEventCreateWithFlags(reinterpret_cast<hipEvent_t*>(&h->inc_ev[i]), hipEventDisableTiming) != hipSuccess)
                st = ADF_EHIP;
        if (st != ADF_OK) {
            (void)hipGetLastError();
            inc_free(h);
            h->inc_on = false;
            fprintf(stderr, "adsorbdiff_hip: no memory for incremental layers (%d atoms), continuing without\n", N);
            return 0;
        }
        h->inc_capN = (int64_t)cap;
    }
    if (h->inc_N != N || h->inc_layers != L || h->build_serial != h->inc_serial) h->inc_valid = false;
    h->inc_N = N; h->inc_layers = L;
    int32_t* tn = h->nptr; h->nptr = h->prev_nptr; h->prev_nptr = tn;
    int32_t* ts = h->e_src; h->e_src = h->prev_src; h->prev_src = ts;
    float4* tg = h->e_geom; h->e_geom = h->prev_geom; h->prev_geom = tg;
    const int state = h->inc_valid ? 1 : 2;
    h->inc_valid = false;
    return state;
}

// Counts of an earlier forward that have reached the pinned buffer: remember them (they steer the next forwards' choice
// between the list and the all-rows form of a layer) and book that forward's statistics.  wait: block until they are there.
static int32_t inc_harvest(adf_painn* h, int slot, bool wait, bool peek = false) {
    // peek: only read the counts (they steer THIS forward, ADF_INC_SYNC=1); the statistics are booked by a later call, once
    // the forward has noted which form each layer took
    if (!h->inc_ev_live[slot]) return ADF_OK;
    hipEvent_t ev = (hipEvent_t)h->inc_ev[slot];
    if (wait) {
        ADF_HIP_CHECK(hipEventSynchronize(ev));
    } else {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipErrorNotReady) { (void)hipGetLastError(); return ADF_OK; }
        ADF_HIP_CHECK(q);
    }
    const int L = h->inc_layers, N = h->inc_pend_N[slot];
    const int32_t* c = h->inc_cnt_host + (size_t)slot * (2 * ADF_MAX_LAYERS + 1);
    for (int i = 0; i < 2 * L + 1; ++i) h->inc_seen[i] = c[i];
    h->inc_seen_valid = true;
    h->inc_pend_Nseen = N;
    if (peek) return ADF_OK;
    h->inc_ev_live[slot] = false;
    for (int l = 0; l < L; ++l) {
        const bool whole = h->inc_pend_whole[slot][l] != 0;
        h->inc_rows += (unsigned long long)(whole ? N : c[l]);
        h->inc_rows_full += (unsigned long long)N;
        h->inc_edges += (unsigned long long)(whole ? c[2 * L] : c[L + l]);
        if (whole || c[l] > 0) ++h->inc_launches;
    }
    return ADF_OK;
}

// One forward on the kept per-layer state.  The graph of this step is built; prev_* hold the previous build's CSR.
static int32_t forward_incremental(adf_painn* h, int N, const int32_t* Z, const int32_t* out_idx, int32_t n_out,
                                   float* f1, float* f2, bool first, int heads, hipStream_t s) {
    const int L = h->hp.num_layers, H = h->hp.hidden_channels;
    const size_t cap = (size_t)h->inc_capN, row = (size_t)5 * H;
    if (out_idx && n_out == 0) return ADF_OK;  // nothing wanted; the state stays invalid (this build was not applied)
    adf_prof_begin(h, ADF_PROF_GRAPH, s);
    if (first) {
        ADF_TRY(adf_nodewise_embed(h, Z, N, h->incX[0], s));
        for (int l = 0; l < L; ++l) ADF_HIP_CHECK(hipMemsetAsync(h->incR[l] + (size_t)N * row, 0, sizeof(float) * row, s));
        ADF_HIP_CHECK(hipMemsetAsync(h->inc_pend, 0, cap * L, s));
    } else {
        ADF_TRY(adf_inc_compare(h, N, s));
    }
    ADF_HIP_CHECK(hipMemsetAsync(h->inc_cnt, 0, sizeof(int32_t) * (2 * ADF_MAX_LAYERS + 1), s));
    if (out_idx) ADF_TRY(adf_inc_need_from_list(h, N, L, out_idx, n_out, s));
    for (int l = 0; l < L; ++l) ADF_TRY(adf_inc_plan_layer(h, l, N, first, out_idx != nullptr, s));
    ADF_HIP_CHECK(hipMemcpyAsync(h->inc_cnt + 2 * L, h->nptr + N, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    // the counts go to the host behind an event; nobody waits for them (unless ADF_INC_SYNC=1)
    const int slot = h->inc_slot;
    h->inc_slot ^= 1;
    if (h->inc_ev_live[slot]) ADF_TRY(inc_harvest(h, slot, true));  // two forwards behind: cannot happen on one stream, but be safe
    int32_t* host = h->inc_cnt_host + (size_t)slot * (2 * ADF_MAX_LAYERS + 1);
    ADF_HIP_CHECK(hipMemcpyAsync(host, h->inc_cnt, sizeof(int32_t) * (2 * L + 1), hipMemcpyDeviceToHost, s));
    ADF_HIP_CHECK(hipEventRecord((hipEvent_t)h->inc_ev[slot], s));
    h->inc_ev_live[slot] = true;
    h->inc_pend_N[slot] = N;
    ADF_TRY(inc_harvest(h, slot ^ 1, false));   // the previous forward's counts, if they have arrived
    if (h->sw.inc_sync) ADF_TRY(inc_harvest(h, slot, true, true));
    adf_prof_end(h, s);
    if (first) ADF_TRY(make_records(h, 0, N, h->incX[0], nullptr, true, h->incR[0], nullptr, s));
    for (int l = 0; l < L; ++l) {
        // all rows (straight into the next layer's tables) or the listed rows.  Recomputing a row that was not listed is
        // harmless: a row without pending changes has unchanged inputs and gets the same value again; a pending but
        // unwanted row keeps its flag and is recomputed before it is next read.  Above ~90 % the compaction costs more
        // than the rows it saves.  The choice rests on the latest counts the host has seen (this forward's with
        // ADF_INC_SYNC=1, else an earlier forward's: only the choice is late, never a result); none seen yet = all rows.
        const int n_seen = h->inc_seen_valid ? h->inc_seen[l] : N;
        const bool whole = first || !h->inc_seen_valid || h->inc_pend_Nseen != N || (long long)n_seen * 10 >= (long long)N * 9;
        h->inc_pend_whole[slot][l] = whole ? 1 : 0;
        if (h->sw.inc_sync && !whole && n_seen == 0) continue;  // exact count: nothing to do
        const float* vin = l == 0 ? h->vecA : h->incV[l];  // layer 0: vec is zero, the pointer is not read
        if (whole) {
            ADF_TRY(message_layer(h, l, N, h->incX[l], vin, h->incX[l + 1], h->incV[l + 1], l == 0, s, nullptr, 0,
                                  h->incR[l], true));
            ADF_TRY(update_layer(h, l, N, h->incX[l + 1], h->incV[l + 1], s));
            if (l + 1 < L)
                ADF_TRY(make_records(h, l + 1, N, h->incX[l + 1], h->incV[l + 1], false, h->incR[l + 1], nullptr, s));
            continue;
        }
        // listed rows: launches sized for `cap` rows, the kernels stop at the list length they read from inc_cnt[l]
        const int32_t* list = h->inc_list + cap * l;
        const int ncap = h->sw.inc_sync ? n_seen : N;
        h->rows_dev = h->inc_cnt + l;
        int32_t st = message_layer(h, l, N, h->incX[l], vin, h->x, h->vecB, l == 0, s, list, ncap, h->incR[l], true);
        if (st == ADF_OK) st = update_layer(h, l, ncap, h->x, h->vecB, s);
        if (st == ADF_OK) {
            adf_prof_begin(h, ADF_PROF_NODE, s);
            st = adf_inc_scatter_rows(h->x, list, ncap, H, h->incX[l + 1], s, h->rows_dev);
            if (st == ADF_OK) st = adf_inc_scatter_rows(h->vecB, list, ncap, 3 * H, h->incV[l + 1], s, h->rows_dev);
            adf_prof_end(h, s);
        }
        if (st == ADF_OK && l + 1 < L) st = make_records(h, l + 1, ncap, h->x, h->vecB, false, h->incR[l + 1], list, s);
        h->rows_dev = nullptr;
        ADF_TRY(st);
    }
    adf_prof_begin(h, ADF_PROF_HEADS, s);
    if (!out_idx) {
        if (heads >= 1) ADF_TRY(adf_head_forward(h, 0, N, h->incX[L], h->incV[L], f1, s));
        if (heads == 2) ADF_TRY(adf_head_forward(h, 1, N, h->incX[L], h->incV[L], f2, s));
        h->x_last = h->incX[L];
    } else {
        ADF_TRY(ensure_subset(h, n_out));
        ADF_TRY(adf_inc_gather_rows(h->incX[L], out_idx, n_out, H, h->sub_x, s));
        ADF_TRY(adf_inc_gather_rows(h->incV[L], out_idx, n_out, 3 * H, h->sub_vec, s));
        for (int hd = 0; hd < heads; ++hd) {
            ADF_TRY(adf_head_forward(h, hd, n_out, h->sub_x, h->sub_vec, h->sub_f, s));
            hipLaunchKernelGGL(adf_scatter_rows3_kernel, dim3((3 * n_out + 255) / 256), dim3(256), 0, s, h->sub_f, out_idx,
                               n_out, hd == 0 ? f1 : f2);
        }
        ADF_HIP_CHECK(hipGetLastError());
    }
    adf_prof_end(h, s);
    h->inc_valid = true;
    return ADF_OK;
}

// head1_only (internal: the translation-only samplers read head 1 alone): f2 may be NULL and no out_forces2 product runs;
// f1 is bit-identical to the two-head forward's
static int32_t forward_impl(adf_painn_t h, const adf_batch* b, const int32_t* out_idx, int32_t n_out, float* f1,
                            float* f2, void* stream, bool head1_only = false) {
    ADF_TRY(check_batch(h, b));
    if (!h->weights_set) { adf_set_error("weights not set"); return ADF_EINVAL; }
    const int heads = head1_only ? 1 : h->hp.num_heads;
    if (heads > h->hp.num_heads) { adf_set_error("the model has no force head"); return ADF_EINVAL; }
    if (!b->atomic_numbers || (heads >= 1 && !f1) || (heads == 2 && !f2)) { adf_set_error("null argument"); return ADF_EINVAL; }
    h->x_last = nullptr;
    hipStream_t s = (hipStream_t)stream;
    const int N = b->num_atoms;
    ADF_TRY(ensure_capacity(h, N, b->num_systems));
    const int inc = inc_prepare(h, N);
    adf_prof_begin(h, ADF_PROF_GRAPH, s);
    ADF_TRY(adf_graph_build_impl(h, b, s));
    adf_prof_end(h, s);
    if (inc) {
        h->inc_serial = h->build_serial;
        return forward_incremental(h, N, b->atomic_numbers, out_idx, n_out, f1, f2, inc == 2, heads, s);
    }
    ADF_TRY(zero_pad_rows(h, N, s));
    ADF_TRY(adf_nodewise_embed(h, b->atomic_numbers, N, h->x, s));  // vec = 0 is implicit in layer 0
    float* vin = h->vecA;
    float* vout = h->vecB;
    const int L = h->hp.num_layers, H = h->hp.hidden_channels;
    // layer-0 records: invariant while the static-atom promise holds (same batch and weights)
    float* rec0 = nullptr;
    bool rec0_ready = false;
    if (h->moving) {
        const size_t row = (size_t)5 * H;
        if ((int64_t)N + 1 > h->rec0_cap) {
            h->rec0_cap = 0; h->rec0_valid = false;
            ADF_TRY(h->m_rec0.alloc(&h->rec0, ((size_t)N + 1) * row));
            h->rec0_cap = (int64_t)N + 1;
        }
        rec0 = h->rec0;
        rec0_ready = h->rec0_valid && h->rec0_N == N;
        if (!rec0_ready) ADF_HIP_CHECK(hipMemsetAsync(rec0 + (size_t)N * row, 0, sizeof(float) * row, s));
        h->rec0_valid = true; h->rec0_N = N;
    }
    if (!out_idx) {
        for (int l = 0; l < L; ++l) {
            if (l == 0) ADF_TRY(message_layer(h, 0, N, h->x, vin, h->x, vout, true, s, nullptr, 0, rec0, rec0_ready));
            else
            ADF_TRY(message_layer(h, l, N, h->x, vin, h->x, vout, l == 0, s));
            ADF_TRY(update_layer(h, l, N, h->x, vout, s));
            float* t = vin; vin = vout; vout = t;
        }
        adf_prof_begin(h, ADF_PROF_HEADS, s);
        if (heads >= 1) ADF_TRY(adf_head_forward(h, 0, N, h->x, vin, f1, s));
        if (heads == 2) ADF_TRY(adf_head_forward(h, 1, N, h->x, vin, f2, s));
        adf_prof_end(h, s);
        h->x_last = h->x;
        return ADF_OK;
    }
    // Outputs wanted on a subset only.  Every layer but the last is needed in full (the listed atoms' messages
    // gather from all their neighbours); in the last layer only the listed atoms are message targets, and their
    // update and the heads run on compact rows.  Per-row arithmetic is unchanged, so the listed rows of f1 / f2
    // are bit-identical to adf_painn_forward's.
    if (n_out == 0) return ADF_OK;
    ADF_TRY(ensure_subset(h, n_out));
    for (int l = 0; l + 1 < L; ++l) {
        if (l == 0) ADF_TRY(message_layer(h, 0, N, h->x, vin, h->x, vout, true, s, nullptr, 0, rec0, rec0_ready));
        else
        ADF_TRY(message_layer(h, l, N, h->x, vin, h->x, vout, l == 0, s));
        ADF_TRY(update_layer(h, l, N, h->x, vout, s));
        float* t = vin; vin = vout; vout = t;
    }
    ADF_TRY(message_layer(h, L - 1, N, h->x, vin, h->sub_x, h->sub_vec, L == 1, s, out_idx, n_out,
                          L == 1 ? rec0 : nullptr, L == 1 && rec0_ready));
    ADF_TRY(update_layer(h, L - 1, n_out, h->sub_x, h->sub_vec, s));
    adf_prof_begin(h, ADF_PROF_HEADS, s);
    for (int hd = 0; hd < heads; ++hd) {
        ADF_TRY(adf_head_forward(h, hd, n_out, h->sub_x, h->sub_vec, h->sub_f, s));
        hipLaunchKernelGGL(adf_scatter_rows3_kernel, dim3((3 * n_out + 255) / 256), dim3(256), 0, s, h->sub_f, out_idx,
                           n_out, hd == 0 ? f1 : f2);
    }
    ADF_HIP_CHECK(hipGetLastError());
    adf_prof_end(h, s);
    return ADF_OK;
}

extern "C" int32_t adf_painn_forward(adf_painn_t h, const adf_batch* b, float* f1, float* f2, void* stream) {
    leave_split(h);
    return forward_impl(h, b, nullptr, 0, f1, f2, stream);
}

extern "C" int32_t adf_painn_forward_subset(adf_painn_t h, const adf_batch* b, const int32_t* out_idx, int32_t n_out,
                                            float* f1, float* f2, void* stream) {
    if (!out_idx || n_out < 0) { adf_set_error("forward_subset: null index list"); return ADF_EINVAL; }
    leave_split(h);
    return forward_impl(h, b, out_idx, n_out, f1, f2, stream);
}

// ---- the forward that the scale-factor fit observes (scale_fit.hip; modules/scaling/fit.py:204-213).  The same launches as
// forward_impl's all-rows branch up to layer `upto`, with the column variance of x taken after every update layer.
extern "C" int32_t adf_painn_forward_observe(adf_painn_t h, const adf_batch* b, int32_t upto, double* layer_var, float* f1,
                                             float* f2, void* stream) {
    ADF_TRY(check_batch(h, b));
    if (!h->weights_set) { adf_set_error("weights not set"); return ADF_EINVAL; }
    const int L = h->hp.num_layers, H = h->hp.hidden_channels, N = b->num_atoms;
    if (!layer_var || !b->atomic_numbers) { adf_set_error("forward_observe: null argument"); return ADF_EINVAL; }
    if (upto < 0 || upto >= L) { adf_set_error("forward_observe: upto=%d outside [0, %d)", upto, L); return ADF_EINVAL; }
    if (N < 2) { adf_set_error("forward_observe: the variance over the atoms needs at least 2 of them, got %d", N); return ADF_EINVAL; }
    const int heads = f1 ? h->hp.num_heads : 0;
    if (f2 && !f1) { adf_set_error("forward_observe: f2 without f1"); return ADF_EINVAL; }
    if (f1 && upto < L - 1) { adf_set_error("forward_observe: the heads need every layer (upto=%d of %d): pass f1 = f2 = NULL", upto, L); return ADF_EINVAL; }
    if (f1 && heads == 0) { adf_set_error("the model has no force head"); return ADF_EINVAL; }
    if (heads == 2 && !f2) { adf_set_error("forward_observe: a two-head handle needs f2 with f1"); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    leave_split(h);
    // a static-atom promise ends here: this is no forward of its sequence
    if (h->moving) { h->moving = nullptr; h->mov_idx = nullptr; h->mov_off = nullptr; ++h->moving_serial; }
    h->cache_valid = false; h->rec0_valid = false; h->inc_valid = false;
    h->x_last = nullptr;
    ADF_TRY(ensure_capacity(h, N, b->num_systems));
    const int64_t need = adf_op_column_variance_scratch(N, H);
    if (need > h->obs_bytes) {
        ADF_HIP_CHECK(hipDeviceSynchronize());   // enqueued work may still use the buffer
        h->obs_bytes = 0;
        ADF_TRY(h->m_obs.alloc(&h->obs_scratch, (size_t)need));
        h->obs_bytes = need;
    }
    adf_prof_begin(h, ADF_PROF_GRAPH, s);
    ADF_TRY(adf_graph_build_impl(h, b, s));
    adf_prof_end(h, s);
    ADF_TRY(zero_pad_rows(h, N, s));
    ADF_TRY(adf_nodewise_embed(h, b->atomic_numbers, N, h->x, s));
    float* vin = h->vecA;
    float* vout = h->vecB;
    for (int l = 0; l <= upto; ++l) {
        ADF_TRY(message_layer(h, l, N, h->x, vin, h->x, vout, l == 0, s));
        ADF_TRY(update_layer(h, l, N, h->x, vout, s));
        ADF_TRY(adf_op_column_variance(h->x, N, H, layer_var + l, h->obs_scratch, stream));
        float* t = vin; vin = vout; vout = t;
    }
    if (heads) {
        adf_prof_begin(h, ADF_PROF_HEADS, s);
        ADF_TRY(adf_head_forward(h, 0, N, h->x, vin, f1, s));
        if (heads == 2) ADF_TRY(adf_head_forward(h, 1, N, h->x, vin, f2, s));
        adf_prof_end(h, s);
    }
    return ADF_OK;
}

// ---- S2EF energy head (painn.py:412-414): per_atom = out_energy.2(ScaledSiLU(out_energy.0(x))), energy = per-system sum
extern "C" int32_t adf_painn_set_energy_head(adf_painn_t h, int32_t n_weights, const void* const* w, void* stream) {
    if (!h || !w) { adf_set_error("null argument"); return ADF_EINVAL; }
    if (n_weights != 4) { adf_set_error("set_energy_head: expected 4 tensors (out_energy.0.weight/bias, out_energy.2.weight/bias), got %d", n_weights); return ADF_EINVAL; }
    for (int i = 0; i < 4; ++i)
        if (!w[i]) { adf_set_error("energy-head tensor %d is null", i); return ADF_EINVAL; }
    const int H = h->hp.hidden_channels, H2 = H / 2;
    const size_t n = (size_t)H2 * H;
    if (!h->oe0_buf) ADF_TRY(h->m_life.alloc(&h->oe0_buf, n * 4 + 64));
    h->oe0_w = reinterpret_cast<const float*>(w[0]);
    h->oe0_b = reinterpret_cast<const float*>(w[1]);
    h->oe2_w = reinterpret_cast<const float*>(w[2]);
    h->oe2_b = reinterpret_cast<const float*>(w[3]);
    adf_w16& e = h->oe0_16;
    e = adf_w16{};
    e.hi = h->oe0_buf; e.lo = h->oe0_buf + n * 2; e.inv_scale = reinterpret_cast<float*>(h->oe0_buf + n * 4);
    ADF_TRY(adf_split_weight(h->oe0_w, (long long)n, &e, reinterpret_cast<unsigned int*>(h->oe0_buf + n * 4 + 16),
                             (hipStream_t)stream));
    h->energy_set = true;
    adf_grad_invalidate(h);
    return ADF_OK;
}

// Edge distances at or below `floor` are replaced by it before the unit vectors are formed (the denoiser's 1e-3 by default;
// the S2EF PaiNN uses 1e-6).  Takes effect with the next graph build.
extern "C" int32_t adf_painn_set_distance_floor(adf_painn_t h, float floor) {
    if (!h || !(floor > 0.f)) { adf_set_error("set_distance_floor: null handle or non-positive floor"); return ADF_EINVAL; }
    if (floor != h->dist_floor) {
        h->dist_floor = floor;
        h->cache_valid = false;
        h->rec0_valid = false;
        h->inc_valid = false;
    }
    return ADF_OK;
}

// One workgroup per system: the per-atom energies y[a] . w + b (one wave per atom, lanes over channels, fixed butterfly),
// accumulated over the system's atoms in a fixed order (wave w takes atoms w, w + 4, ...; then waves 0..3).  A system's
// energy therefore depends on its own rows only: bit-identical whatever batch it sits in.  No atomics.
__global__ __launch_bounds__(256) void adf_energy_sum_kernel(const float* __restrict__ y, int H2, const float* __restrict__ w,
                                                             const float* __restrict__ bias, const int32_t* __restrict__ atom_offset,
                                                             float* __restrict__ energy) {
    __shared__ float part[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int a0 = atom_offset[b], a1 = atom_offset[b + 1];
    const float b0 = bias[0];
    float acc = 0.f;
    for (int a = a0 + wave; a < a1; a += 4) {
        const float* row = y + (size_t)a * H2;
        float d = 0.f;
        for (int c = lane; c < H2; c += 64) d = fmaf(row[c], w[c], d);
        d = adf_wave_sum(d);
        acc = __fadd_rn(acc, __fadd_rn(d, b0));
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) energy[b] = __fadd_rn(__fadd_rn(part[0], part[1]), __fadd_rn(part[2], part[3]));
}

int32_t adf_energy_sum(const float* y, int H2, const float* w, const float* bias, const int32_t* atom_offset, float* energy,
                       int num_systems, hipStream_t s) {
    hipLaunchKernelGGL(adf_energy_sum_kernel, dim3(num_systems), dim3(256), 0, s, y, H2, w, bias, atom_offset, energy);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}

// energy [B] (and forces [N,3] unless the model has no force head: forces may be NULL then)
extern "C" int32_t adf_painn_forward_energy(adf_painn_t h, const adf_batch* b, float* energy, float* forces, void* stream) {
    ADF_TRY(check_batch(h, b));
    if (!h->energy_set) { adf_set_error("forward_energy: energy head not set (adf_painn_set_energy_head)"); return ADF_EINVAL; }
    if (!energy || (h->hp.num_heads >= 1 && !forces)) { adf_set_error("forward_energy: null output"); return ADF_EINVAL; }
    if (h->hp.num_heads > 1) { adf_set_error("forward_energy: the S2EF model has one force head"); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    leave_split(h);
    ADF_TRY(forward_impl(h, b, nullptr, 0, forces, nullptr, stream));
    if (!h->x_last) { adf_set_error("internal: no node features after the forward"); return ADF_EINVAL; }
    const int N = b->num_atoms, H = h->hp.hidden_channels, H2 = H / 2;
    adf_prof_begin(h, ADF_PROF_HEADS, s);
    // h->y is free once the force head has run ([capN, H] >= [N, H/2])
    ADF_TRY(adf_linear(h, h->x_last, H, h->oe0_w, &h->oe0_16, h->oe0_b, h->y, H2, N, H2, H, 1, s));
    ADF_TRY(adf_energy_sum(h->y, H2, h->oe2_w, h->oe2_b, b->atom_offset, energy, b->num_systems, s));
    adf_prof_end(h, s);
    return ADF_OK;
}

// Stand-alone nn.Linear (unit tests of the two GEMM kernels): C = act(A . W^T + b)
extern "C" int32_t adf_linear_forward(const float* A, const float* W, const float* bias, float* C, int32_t M,
                                      int32_t N, int32_t K, int32_t act_ssilu, int32_t mode, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0) { adf_set_error("bad argument"); return ADF_EINVAL; }
    if (mode == 0) return adf_launch_gemm(A, K, W, K, bias, C, N, M, N, K, act_ssilu, s);
    adf_pool tmp;   // frees buf / mags on every return
    unsigned char* buf = nullptr;
    const size_t n = (size_t)N * K;
    ADF_TRY(tmp.alloc(&buf, n * 4 + 64));
    adf_w16 w16 = {};
    w16.hi = buf; w16.lo = buf + n * 2; w16.inv_scale = reinterpret_cast<float*>(buf + n * 4);
    unsigned int* scratch = reinterpret_cast<unsigned int*>(buf + n * 4 + 16);
    int32_t st = adf_split_weight(W, (long long)n, &w16, scratch, s);
    float* mags = nullptr;
    const bool lift = adf_switches_from_env().lift != 0;   // ADF_LIFT as it stands at this call
    if (st == ADF_OK && lift) st = tmp.alloc(&mags, (size_t)M);
    adf_lift lf = {mags, M};
    if (st == ADF_OK) st = adf_launch_gemm16(A, K, &w16, bias, C, N, M, N, K, act_ssilu, nullptr, s, lift ? &lf : nullptr,
                                             adf_switches_process().tune, adf_current_num_cus());
    (void)hipStreamSynchronize(s);
    return st;
}

// 0 = f16x3 split products on the f16 matrix cores (default), 1 = exact f32 MFMA everywhere (what ADF_GEMM=f32 selects
// at creation).  Takes effect with the next forward; the weight images of both modes are kept by adf_painn_set_weights.
extern "C" int32_t adf_painn_set_arithmetic(adf_painn_t h, int32_t exact_f32) {
    if (!h) { adf_set_error("null handle"); return ADF_EINVAL; }
    h->gemm_f32 = exact_f32 != 0;
    h->msg_f32 = exact_f32 != 0 || h->msg_f32_only;
    h->rec0_valid = false;
    h->inc_valid = false;
    return ADF_OK;
}

// Incremental layers (see incremental.hip): 1 = keep per-layer node state across the forwards of a static-atom promise
// and recompute only rows whose inputs changed (default; bit-identical outputs), 0 = every forward computes every row.
// Resets the row counters reported by adf_get_counters.
extern "C" int32_t adf_painn_set_incremental(adf_painn_t h, int32_t on) {
    if (!h) { adf_set_error("null handle"); return ADF_EINVAL; }
    if ((on != 0) != h->inc_on) {
        ADF_HIP_CHECK(hipDeviceSynchronize());
        h->inc_on = on != 0;
        if (!h->inc_on) inc_free(h);
        if (h->inc_on && h->capN > 0 && !h->prev_nptr) {  // workspaces exist without the previous-CSR buffers
            int32_t st = h->m_ws.alloc(&h->prev_nptr, (size_t)h->capN + 1);
            if (st == ADF_OK) st = h->m_ws.alloc(&h->prev_src, (size_t)h->capE);
            if (st == ADF_OK) st = h->m_ws.alloc(&h->prev_geom, (size_t)h->capE);
            if (st != ADF_OK) { h->inc_on = false; return st; }
        }
    }
    h->inc_valid = false;
    ++h->inc_set_serial;
    (void)inc_harvest(h, h->inc_slot, true);
    (void)inc_harvest(h, h->inc_slot ^ 1, true);
    h->inc_seen_valid = false;
    h->inc_rows = h->inc_rows_full = h->inc_edges = h->inc_launches = 0;
    if (h->twin) {   // the pair's totals are sums: both start from zero together
        ADF_TRY(adf_painn_set_incremental(h->twin, on));
        h->twin->seen_inc_serial = h->inc_set_serial;
    }
    return ADF_OK;
}

extern "C" int32_t adf_check_flags(adf_painn_t h, void* stream) {
    if (!h) { adf_set_error("null handle"); return ADF_EINVAL; }
    return read_flags(h, (hipStream_t)stream);
}

// ---- the stepper entries and the fused sampling loop (stepper.hip) on a PaiNN handle
static int32_t model_check(void* h, const adf_batch* b) { return check_batch((adf_painn*)h, b); }
static int32_t model_grow(void* h, const adf_batch* b, float** sys) {
    adf_painn* p = (adf_painn*)h;
    ADF_TRY(ensure_capacity(p, b->num_atoms, b->num_systems));
    *sys = p->sys;
    return ADF_OK;
}
static int32_t model_forward(void* h, const adf_batch* b, const int32_t* out_idx, int32_t n_out, float* f1, float* f2,
                             hipStream_t s) {
    return forward_impl((adf_painn*)h, b, out_idx, out_idx ? n_out : 0, f1, f2, s, !f2);
}
static void model_prof(void* h, bool begin, hipStream_t s) {
    if (begin) adf_prof_begin((adf_painn*)h, ADF_PROF_STEPPER, s);
    else adf_prof_end((adf_painn*)h, s);
}
static adf_model model(adf_painn_t h) {
    return {h, model_check, model_grow, model_forward, model_prof, h ? h->ps_state : nullptr, h ? h->ps_B : 0};
}

extern "C" int32_t adf_painn_set_per_system_stop(adf_painn_t h, int32_t* sys_state, int32_t B) {
    if (!h) { adf_set_error("null handle"); return ADF_EINVAL; }
    return adf_model_set_per_system_stop(&h->ps_state, &h->ps_B, sys_state, B);
}

extern "C" int32_t adf_sde_init_placement(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags,
                                          const float* noise, void* stream) {
    return adf_model_init_placement(model(h), b, pos, tags, noise, (hipStream_t)stream);
}

extern "C" int32_t adf_sde_step(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags,
                                const int32_t* fixed, const float* f1, const float* f2, const adf_step_coef* coef,
                                const float* z_tr, const float* z_rot, int32_t early_stop_count, int32_t* state,
                                float* dcom, float* drot, void* stream) {
    return adf_model_sde_step(model(h), b, pos, tags, fixed, f1, f2, coef, nullptr, 0, z_tr, z_rot, early_stop_count, state,
                              dcom, drot, (hipStream_t)stream);
}

extern "C" int32_t adf_sde_step_scheduled(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags,
                                          const int32_t* fixed, const float* f1, const float* f2,
                                          const adf_step_coef* coefs_dev, int32_t num_steps, const float* z_tr,
                                          const float* z_rot, int32_t early_stop_count, int32_t* state, float* dcom,
                                          float* drot, void* stream) {
    return adf_model_sde_step(model(h), b, pos, tags, fixed, f1, f2, nullptr, coefs_dev, num_steps, z_tr, z_rot,
                              early_stop_count, state, dcom, drot, (hipStream_t)stream);
}

extern "C" int32_t adf_sample(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags, const int32_t* fixed,
                              const adf_step_coef* coefs_dev, int32_t num_steps, const float* z_tr_all,
                              const float* z_rot_all, int32_t early_stop_count, int32_t poll_every, int32_t* state,
                              const int32_t* out_idx, int32_t n_out, float* f1, float* f2, void* stream) {
    leave_split(h);
    return adf_model_sample(model(h), b, pos, tags, fixed, coefs_dev, num_steps, z_tr_all, z_rot_all, early_stop_count,
                            poll_every, state, out_idx, n_out, f1, f2, nullptr, 0, (hipStream_t)stream);
}

extern "C" int32_t adf_sample_traj(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags, const int32_t* fixed,
                                   const adf_step_coef* coefs_dev, int32_t num_steps, const float* z_tr_all,
                                   const float* z_rot_all, int32_t early_stop_count, int32_t poll_every, int32_t* state,
                                   const int32_t* out_idx, int32_t n_out, float* f1, float* f2, adf_frames_t sink,
                                   int32_t frame_every, void* stream) {
    leave_split(h);
    if (!sink) { adf_set_error("sample_traj: null sink"); return ADF_EINVAL; }
    return adf_model_sample(model(h), b, pos, tags, fixed, coefs_dev, num_steps, z_tr_all, z_rot_all, early_stop_count,
                            poll_every, state, out_idx, n_out, f1, f2, sink, frame_every, (hipStream_t)stream);
}

// Translation-only samplers (reverse_sde_sampling / langevin_dynamics, denoising_torch.py:96-196, 369-458)
extern "C" int32_t adf_tr_step(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags, const float* f1,
                               const adf_tr_coef* coef, const adf_tr_coef* coefs_dev, int32_t num_steps, const float* z,
                               int32_t early_stop_count, int32_t* state, float* dcom, void* stream) {
    return adf_model_tr_step(model(h), b, pos, tags, f1, coef, coefs_dev, num_steps, z, early_stop_count, state, dcom,
                             (hipStream_t)stream);
}

extern "C" int32_t adf_tr_sample(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags,
                                 const adf_tr_coef* coefs_dev, int32_t num_steps, const float* z_all,
                                 int32_t early_stop_count, int32_t poll_every, int32_t* state, const int32_t* out_idx,
                                 int32_t n_out, float* f1, void* stream) {
    leave_split(h);
    return adf_model_tr_sample(model(h), b, pos, tags, coefs_dev, num_steps, z_all, early_stop_count, poll_every, state,
                               out_idx, n_out, f1, nullptr, 0, (hipStream_t)stream);
}

extern "C" int32_t adf_tr_sample_traj(adf_painn_t h, const adf_batch* b, float* pos, const int32_t* tags,
                                      const adf_tr_coef* coefs_dev, int32_t num_steps, const float* z_all,
                                      int32_t early_stop_count, int32_t poll_every, int32_t* state, const int32_t* out_idx,
                                      int32_t n_out, float* f1, adf_frames_t sink, int32_t frame_every, void* stream) {
    leave_split(h);
    if (!sink) { adf_set_error("tr_sample_traj: null sink"); return ADF_EINVAL; }
    return adf_model_tr_sample(model(h), b, pos, tags, coefs_dev, num_steps, z_all, early_stop_count, poll_every, state,
                               out_idx, n_out, f1, sink, frame_every, (hipStream_t)stream);
}

// ---- adf_sample on two views of the batch, two handles, two streams (the header's section of that name; the loop: stepper.hip)
extern "C" int32_t adf_sample_split(adf_painn_t h, adf_painn_t t, const adf_batch* b, const adf_split_view* v, float* pos,
                                    const int32_t* tags, const int32_t* fixed, const adf_step_coef* coefs_dev,
                                    int32_t num_steps, const float* z_tr_all, const float* z_rot_all,
                                    int32_t early_stop_count, int32_t poll_every, int32_t* state, const int32_t* out_idx,
                                    int32_t n_out, float* f1, float* f2, void* stream) {
    ADF_TRY(check_batch(h, b));
    if (!t || t->parent != h) { adf_set_error("sample_split: the second handle is not this handle's twin"); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const bool per_system = h->ps_state != nullptr;
    // The one-stream loop, unchanged, where two chains are not independent or not the same arithmetic: the coupled early
    // stop makes every step wait for all systems; the exact-f32 retry is a decision of the whole batch.
    const bool split = h->sw.tune.sample_split && b->num_systems >= 2 && !h->gemm_f32 && !(early_stop_count > 0 && !per_system);
    if (!split) {
        leave_split(h);
        ++h->split_fallbacks;
        return adf_model_sample(model(h), b, pos, tags, fixed, coefs_dev, num_steps, z_tr_all, z_rot_all, early_stop_count,
                                poll_every, state, out_idx, n_out, f1, f2, nullptr, 0, s);
    }
    const int32_t B = b->num_systems, N = b->num_atoms;
    if (!v || v->cut <= 0 || v->cut >= B || v->atoms_a <= 0 || v->atoms_a >= N || !v->atom_offset || !v->batch) {
        adf_set_error("sample_split: the view does not cut the batch into two non-empty sides");
        return ADF_EINVAL;
    }
    if (!pos || !tags || !f1 || !f2 || !state || num_steps <= 0) { adf_set_error("sample_split: bad argument"); return ADF_EINVAL; }
    if (out_idx && (v->n_out_a < 0 || v->n_out_b < 0 || v->n_out_a + v->n_out_b != n_out || (v->n_out_b > 0 && !v->out_idx))) {
        adf_set_error("sample_split: the view's share of out_idx does not add up to n_out = %d", (int)n_out);
        return ADF_EINVAL;
    }
    if (h->moving && (!v->mov_idx || !v->mov_off)) { adf_set_error("sample_split: a static-atom promise is in force and the view has no moving lists"); return ADF_EINVAL; }
    if (per_system && h->ps_B != B) { adf_set_error("per-system stop is set for %d systems, the batch has %d", (int)h->ps_B, (int)B); return ADF_EINVAL; }
    const int32_t cut = v->cut, NA = v->atoms_a;
    // the parent: whatever it kept of another shape (the whole batch, another cut) under this promise goes
    if (!h->split_last || h->split_cut != cut || h->split_N != N) { h->cache_valid = false; h->rec0_valid = false; h->inc_valid = false; }
    h->split_last = true; h->split_cut = cut; h->split_N = N;
    // the twin follows the parent: switches, arithmetic, the static-atom promise, the incremental-layer switch
    follow_settings(t, h);
    const int32_t* movB = h->moving ? h->moving + NA : nullptr;   // a new promise, or other lists for the same one
    if (t->seen_moving_serial != h->moving_serial || t->moving != movB ||
        (movB && (t->mov_idx != v->mov_idx || t->mov_off != v->mov_off))) {
        ADF_TRY(adf_graph_set_moving(t, h->moving ? h->moving + NA : nullptr, h->moving ? v->mov_idx : nullptr,
                                     h->moving ? v->mov_off : nullptr));
        t->seen_moving_serial = h->moving_serial;
    }
    if (t->seen_inc_serial != h->inc_set_serial || t->inc_on != h->inc_on) {
        ADF_TRY(adf_painn_set_incremental(t, h->inc_on ? 1 : 0));
        t->seen_inc_serial = h->inc_set_serial;
    }
    if (!per_system && num_steps > t->split_hist_cap) {
        ADF_HIP_CHECK(hipDeviceSynchronize());
        t->split_hist_cap = 0;
        ADF_TRY(t->m_life.alloc(&t->split_hist, (size_t)2 * num_steps));
        t->split_hist_cap = num_steps;
    }
    adf_batch bA = *b, bB = *b;   // both views search the whole batch's lattice images (reps)
    bA.num_systems = cut; bA.num_atoms = NA;
    bB.num_systems = B - cut; bB.num_atoms = N - NA;
    bB.pos = b->pos + 3 * (size_t)NA; bB.cell = b->cell + 9 * (size_t)cut;
    bB.atomic_numbers = b->atomic_numbers ? b->atomic_numbers + NA : nullptr;
    bB.batch = v->batch; bB.atom_offset = v->atom_offset;
    adf_model mA = model(h), mB = model(t);
    if (per_system) { mA.sys_B = cut; mB.sys_state = h->ps_state + 4 * (size_t)cut; mB.sys_B = B - cut; }
    else { mB.sys_state = nullptr; mB.sys_B = 0; }
    adf_split_side A = {&bA, pos, tags, fixed, out_idx, out_idx ? v->n_out_a : 0, f1, f2, state,
                        per_system ? nullptr : t->split_hist, 0, s};
    adf_split_side Bv = {&bB, pos + 3 * (size_t)NA, tags + NA, fixed ? fixed + NA : nullptr, out_idx ? v->out_idx : nullptr,
                         out_idx ? v->n_out_b : 0, f1 + 3 * (size_t)NA, f2 + 3 * (size_t)NA, t->split_state,
                         per_system ? nullptr : t->split_hist + t->split_hist_cap, cut, (hipStream_t)t->split_stream};
    ++h->split_runs;
    return adf_model_sample_split(mA, mB, A, Bv, coefs_dev, num_steps, z_tr_all, z_rot_all, B, early_stop_count, poll_every,
                                  t->split_state + 8, (hipEvent_t)t->split_ev[0], (hipEvent_t)t->split_ev[1]);
}

// the counters of one handle
static int32_t handle_counters(adf_painn* h, adf_counters* out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = h->lastN, H = h->hp.hidden_channels, R = h->hp.num_rbf, L = h->hp.num_layers;
    int32_t e = 0;
    ADF_HIP_CHECK(hipMemcpyAsync(&e, h->nptr + N, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ADF_HIP_CHECK(hipStreamSynchronize(s));
    const int64_t E = e;
    out->num_edges = E;
    out->num_atoms = N;
    // E*(3H*4 + 12 + 8) + N*(3H*4 + 3H*4) + N*(H*4 + 3H*4)
    out->message_bytes_per_layer = E * (3 * H * 4 + 12 + 8) + N * (3 * H * 4 + 3 * H * 4) + N * (H * 4 + 3 * H * 4);
    // per layer: node side 30 H^2 N, edge side 2 R 3H E; heads: per head 2*(3N*H*H + 3N*H*H/2 + N*2H*H + N*H*H
    //            + 3N*(H/2)^2 + N*H*H/2)
    const int64_t head = 2 * (3 * N * H * H + 3 * N * H * H / 2 + N * 2 * H * H + N * H * H + 3 * N * (H / 2) * (H / 2) +
                              N * H * H / 2);
    out->dense_flops = L * (30 * H * H * N + 2 * R * 3 * H * E) + h->hp.num_heads * head;
    ADF_TRY(inc_harvest(h, h->inc_slot, true));      // the older of the two outstanding forwards first
    ADF_TRY(inc_harvest(h, h->inc_slot ^ 1, true));
    out->inc_rows = (int64_t)h->inc_rows; out->inc_rows_full = (int64_t)h->inc_rows_full;
    out->inc_msg_launches = (int64_t)h->inc_launches; out->inc_msg_edges = (int64_t)h->inc_edges;
    return ADF_OK;
}

extern "C" int32_t adf_get_counters(adf_painn_t h, adf_counters* out, void* stream) {
    if (!h || !out || h->lastN <= 0) { adf_set_error("no forward has run"); return ADF_EINVAL; }
    ADF_TRY(handle_counters(h, out, stream));
    if (!h->twin || h->twin->lastN <= 0) return ADF_OK;
    // the pair: every field is a sum (all are linear in E and N) - the totals of the incremental layers always, the last
    // graph's only when the last run was split
    adf_counters c;
    ADF_TRY(handle_counters(h->twin, &c, stream));
    if (h->split_last) {
        out->num_edges += c.num_edges; out->num_atoms += c.num_atoms;
        out->message_bytes_per_layer += c.message_bytes_per_layer; out->dense_flops += c.dense_flops;
    }
    out->inc_rows += c.inc_rows; out->inc_rows_full += c.inc_rows_full;
    out->inc_msg_launches += c.inc_msg_launches; out->inc_msg_edges += c.inc_msg_edges;
    return ADF_OK;
}
