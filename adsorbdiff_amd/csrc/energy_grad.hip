// Forces as the gradient of the energy for the S2EF PaiNN: F = -dE/dpos with E the sum of the per-system energies and the
// edge set held fixed - what torch.autograd.grad(out["energy"].sum(), pos) gives on the reference module
// (adsorbdiff/models/painn/painn.py:318-340, 380-414; NOT its direct_forces=False branch, painn.py:421-429, which
// differentiates sum(x) instead of the energy).
//
// One call (adf_painn_forward_energy_gradient):
//   1. graph build, then a forward through the training step's operators that keeps what the backward reads: per layer the
//      inputs x / vec, the LayerNorm moments, the two pre-activations, xh, vv = vec_proj(vec1), [x1 | |v2|], the gates a and
//      dot - 21 H floats per atom and layer (18 H for layer 0: no vec input) (workspace: adf_painn_energy_gradient_workspace);
//   2. the seed d(per-atom energy) = 1 through out_energy, then the update / message / LayerNorm chain from the last layer to
//      the first with DATA gradients only: no weight-gradient product runs (the LayerNorm backward operator still reduces its
//      [H] gain and bias gradients into scratch nobody reads: two small launches per layer), and every product reads an image of the transposed
//      weight that is built once per bound weight set (the weights do not change during a relaxation), not per call;
//      layer 0's x_proj / LayerNorm backward is skipped (its input is the embedding, which does not depend on positions);
//   3. per layer the edge-geometry gradient (message_geo.hip on the matrix cores; in exact-f32 arithmetic or with unequally
//      spaced centres the plain kernel below, which is the message backward and the geometry gradient in one), accumulated
//      in place over the layers: the geometry is the same for all of them;
//   4. once: the reverse-edge index of the graph and the position kernel, forces[n] = sum over n's own rows e of
//      (G_e - G_rev(e)), G_e = alpha_e u_e - (b_e - (b_e . u_e) u_e) / d_e.  No float atomics anywhere: every sum has a fixed
//      order, so the forces are run-to-run identical and an atom's force depends on its own system only.
#include <stdlib.h>
#include <string.h>

#include "message.h"

struct EgW {
    const float* f32;   // [N, K] row-major (exact arithmetic)
    adf_w16 w16;        // its fp16 hi / lo split (+ fragment image)
};
enum { EG_XP0 = 0, EG_XP2, EG_VP, EG_XV0, EG_XV2, EG_NW };

struct adf_grad {
    unsigned char* warena;
    float* wscales;
    bool wvalid;
    EgW fw[ADF_MAX_LAYERS][EG_NW];   // C = A W^T
    EgW bw[ADF_MAX_LAYERS][EG_NW];   // dA = dC W: the transposed weight as a weight
    EgW oe_bw;                       // out_energy.0 transposed
    float* rbf_wt[ADF_MAX_LAYERS];   // rbf_proj.weight transposed [R, 3H] (plain kernel)
    float* act;
    size_t act_floats;
    float4* part;
    int32_t* rev;
    long long ecap;
    int part_slices;
    adf_pool m_w;    // warena, wscales
    adf_pool m_ws;   // act, part, rev
};

static adf_grad* eg_state(adf_painn* h) {
    if (!h->grad) {
        adf_grad* g = new (std::nothrow) adf_grad();
        if (!g) return nullptr;
        h->grad = g;
    }
    return reinterpret_cast<adf_grad*>(h->grad);
}

void adf_grad_invalidate(adf_painn* h) {
    if (h && h->grad) reinterpret_cast<adf_grad*>(h->grad)->wvalid = false;
}

void adf_grad_free(adf_painn* h) {
    if (!h) return;
    delete reinterpret_cast<adf_grad*>(h->grad);
    h->grad = nullptr;
}

// ------------------------------------------------------------------------------------------------ small kernels
__global__ void eg_transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int R, int C) {
    __shared__ float t[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int rr = by + r, cc = bx + threadIdx.x;
        t[r][threadIdx.x] = (rr < R && cc < C) ? src[(size_t)rr * C + cc] : 0.f;
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int cc = bx + r, rr = by + threadIdx.x;
        if (cc < C && rr < R) dst[(size_t)cc * R + rr] = t[threadIdx.x][r];
    }
}

static inline unsigned eg_grid(long long total) {
    long long b = (total + 255) / 256;
    if (b > 256 * 16) b = 256 * 16;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// seed of the backward: d(energy)/d(he0[n, c]) = ScaledSiLU'(he0[n, c]) out_energy.2.weight[c]   (d(per-atom energy) = 1)
__global__ void eg_seed_kernel(const float* __restrict__ he0, const float* __restrict__ w2, float* __restrict__ dhe,
                               long long N, int H2) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < N * H2; t += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(t % H2);
        dhe[t] = adf_dssilu_times(he0[t], w2[c]);   // (shared with adf_op_energy_head_bwd, the dE != 1 case with weight gradients)
    }
}

__global__ void eg_add_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dst[i] += src[i];
}

// Exact-f32 (and unequally spaced centres) form of a message block's backward with the geometry gradient: one workgroup per
// SOURCE atom j over its own CSR segment, as train.hip's tr_msg_bwd_kernel, but rbfh and rbfh' are formed per edge from the
// transposed rbf_proj.weight instead of read from an [E, 3H] tensor, and nothing per edge and channel is written.
//   dxh[j], dvec[j] (unless vec == 0), dx[j] = gx1[j] / sqrt2 as tr_msg_bwd_kernel;  part[e] (+)= (alpha_e, b_e).
__global__ __launch_bounds__(256) void eg_msg_bwd_plain_kernel(
    const int32_t* __restrict__ nptr, const int32_t* __restrict__ e_src, const float4* __restrict__ e_geom,
    const float* __restrict__ xh, const float* __restrict__ vec, const float* __restrict__ wt, const float* __restrict__ bias,
    const float* __restrict__ mu, int R, float inv_cutoff, float coeff, float env_a, float env_b, float env_c, int env_pi,
    const float* __restrict__ gx1, const float* __restrict__ gv1, float* __restrict__ dxh, float* __restrict__ dvec,
    float* __restrict__ dx, float4* __restrict__ part, int H, int vec_is_zero, int accumulate) {
    __shared__ float rbv[128], rbd[128], red[4][4];
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e0 = nptr[j], e1 = nptr[j + 1];
    const float is3 = 0.57735026918962576f, ish = 1.0f / sqrtf((float)H), is2 = 0.70710678118654752f;
    const int H3 = 3 * H;
    for (int cb = 0; cb < H; cb += 256) {
        const int c = cb + tid;
        const bool on = c < H;
        float xa = 0.f, xb = 0.f, xc = 0.f, w0 = 0.f, w1 = 0.f, w2 = 0.f, ba = 0.f, bb = 0.f, bc = 0.f;
        if (on) {
            const float* xr = xh + (size_t)j * H3;
            xa = xr[c]; xb = xr[H + c]; xc = xr[2 * H + c];
            ba = bias[c]; bb = bias[H + c]; bc = bias[2 * H + c];
            if (!vec_is_zero) { const float* vr = vec + (size_t)j * H3; w0 = vr[c]; w1 = vr[H + c]; w2 = vr[2 * H + c]; }
        }
        float dxa = 0.f, dxb = 0.f, dxc = 0.f, dv0 = 0.f, dv1 = 0.f, dv2 = 0.f;
        for (int e = e0; e < e1; ++e) {
            const int i = e_src[e];
            const float4 g = e_geom[e];
            __syncthreads();
            if (tid < R) {
                const float xs = g.w * inv_cutoff;
                float xq = 1.0f;
                for (int k = 1; k < env_pi; ++k) xq *= xs;
                const float xp = xq * xs, pe = (float)env_pi;
                float env = 1.0f + env_a * xp + env_b * (xp * xs) + env_c * (xp * xs * xs);
                float envd = env_a * pe * xq + env_b * (pe + 1.0f) * xp + env_c * (pe + 2.0f) * (xp * xs);
                if (!(xs < 1.0f)) { env = 0.f; envd = 0.f; }
                const float dm = xs - mu[tid];
                const float ga = expf(coeff * dm * dm);
                rbv[tid] = env * ga;
                rbd[tid] = (envd + env * 2.0f * coeff * dm) * ga * inv_cutoff;
            }
            __syncthreads();
            float al = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f;
            if (on) {
                float ra = ba, rb = bb, rc = bc, pa = 0.f, pb = 0.f, pc = 0.f;
                for (int k = 0; k < R; ++k) {
                    const float* wr = wt + (size_t)k * H3;
                    const float wa = wr[c], wb = wr[H + c], wc = wr[2 * H + c];
                    const float v = rbv[k], d = rbd[k];
                    ra = fmaf(wa, v, ra); rb = fmaf(wb, v, rb); rc = fmaf(wc, v, rc);
                    pa = fmaf(wa, d, pa); pb = fmaf(wb, d, pb); pc = fmaf(wc, d, pc);
                }
                const float gx = gx1[(size_t)i * H + c] * is2;
                const size_t vo = (size_t)i * H3 + c;
                const float g0 = gv1[vo] * ish, g1 = gv1[vo + H] * ish, g2 = gv1[vo + 2 * H] * ish;
                const float S = (g0 * w0 + g1 * w1 + g2 * w2) * is3;
                const float T = -(g0 * g.x + g1 * g.y + g2 * g.z);
                dxa += gx * ra; dxb += S * rb; dxc += T * rc;
                const float f = xb * rb * is3;
                dv0 += g0 * f; dv1 += g1 * f; dv2 += g2 * f;
                al = gx * xa * pa + S * xb * pb + T * xc * pc;
                const float fc = xc * rc;
                b0 = g0 * fc; b1 = g1 * fc; b2 = g2 * fc;
            }
            al = adf_wave_sum(al); b0 = adf_wave_sum(b0); b1 = adf_wave_sum(b1); b2 = adf_wave_sum(b2);
            if (lane == 0) { red[wave][0] = al; red[wave][1] = b0; red[wave][2] = b1; red[wave][3] = b2; }
            __syncthreads();
            if (tid < 4) {
                const float sum = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
                float* o = reinterpret_cast<float*>(part + e) + tid;
                *o = (cb == 0 && !accumulate) ? sum : *o + sum;
            }
        }
        if (on) {
            float* dh = dxh + (size_t)j * H3;
            dh[c] = dxa; dh[H + c] = dxb; dh[2 * H + c] = dxc;
            dx[(size_t)j * H + c] = gx1[(size_t)j * H + c] * is2;
            if (!vec_is_zero) {
                const size_t vo = (size_t)j * H3 + c;
                dvec[vo] = gv1[vo] + dv0; dvec[vo + H] = gv1[vo + H] + dv1; dvec[vo + 2 * H] = gv1[vo + 2 * H] + dv2;
            }
        }
    }
}

// rev[e] = the row of the same pair in the partner's segment: same distance bits, exactly negated unit vector
// (graph.hip adf_fill_kernel writes the two rows of a pair that way), which tells parallel periodic images apart.
// One wave per atom.  A row without a partner (an asymmetric graph: not produced by the graph build) gets -1 and raises
// flag 6, so the next adf_check_flags reports an error instead of forces that miss a term.
__global__ __launch_bounds__(256) void eg_reverse_index_kernel(const int32_t* __restrict__ nptr, const int32_t* __restrict__ e_src,
                                                                const float4* __restrict__ e_geom, int N, int32_t* __restrict__ rev,
                                                                int32_t* __restrict__ flags) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    for (int e = nptr[n] + (threadIdx.x & 63); e < nptr[n + 1]; e += 64) {
        const int i = e_src[e];
        const float4 g = e_geom[e];
        int found = -1;
        for (int f = nptr[i]; f < nptr[i + 1]; ++f) {
            if (e_src[f] != n) continue;
            const float4 o = e_geom[f];
            if (o.w == g.w && o.x == -g.x && o.y == -g.y && o.z == -g.z) { found = f; break; }
        }
        rev[e] = found;
        if (found < 0) flags[6] = 1;
    }
}

// gradient of the energy with respect to the stored edge vector of row e (pos[e_src] - pos[owner] + offset), from the
// message owner -> e_src: the slices' partial sums in slice order, then alpha u - (b - (b . u) u) / d.  Every operation is
// spelled out so that the two places that evaluate a row (its owner's sum and its partner's) get the same bits.
__device__ __forceinline__ void eg_row_gradient(const float4* __restrict__ part, long long ecap, int nslices,
                                                const float4 g, int e, float& gx, float& gy, float& gz) {
    float al = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
    for (int sl = 0; sl < nslices; ++sl) {
        const float4 v = part[(size_t)sl * ecap + e];
        al = __fadd_rn(al, v.x); bx = __fadd_rn(bx, v.y); by = __fadd_rn(by, v.z); bz = __fadd_rn(bz, v.w);
    }
    const float bu = fmaf(bz, g.z, fmaf(by, g.y, __fmul_rn(bx, g.x)));
    const float inv = __fdiv_rn(1.0f, g.w);
    gx = __fsub_rn(__fmul_rn(al, g.x), __fmul_rn(fmaf(-bu, g.x, bx), inv));
    gy = __fsub_rn(__fmul_rn(al, g.y), __fmul_rn(fmaf(-bu, g.y, by), inv));
    gz = __fsub_rn(__fmul_rn(al, g.z), __fmul_rn(fmaf(-bu, g.z, bz), inv));
}

// forces[n] = -dE/dpos[n] = sum over n's rows e (ascending) of (G_e - G_rev(e)): one wave per atom, lane l takes rows
// e0 + l, e0 + l + 64, ...; then a fixed butterfly.  G_e is added here and the same float is subtracted at the partner.
__global__ __launch_bounds__(256) void eg_position_kernel(const int32_t* __restrict__ nptr, const float4* __restrict__ e_geom,
                                                           const int32_t* __restrict__ rev, const float4* __restrict__ part,
                                                           long long ecap, int nslices, int N,
                                                           float* __restrict__ forces) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    for (int e = nptr[n] + lane; e < nptr[n + 1]; e += 64) {
        float ax, ay, az, bx = 0.f, by = 0.f, bz = 0.f;
        eg_row_gradient(part, ecap, nslices, e_geom[e], e, ax, ay, az);
        const int f = rev[e];
        if (f >= 0) eg_row_gradient(part, ecap, nslices, e_geom[f], f, bx, by, bz);
        fx = __fadd_rn(fx, __fsub_rn(ax, bx)); fy = __fadd_rn(fy, __fsub_rn(ay, by)); fz = __fadd_rn(fz, __fsub_rn(az, bz));
    }
    // kept inline: as a call to lanes.h this butterfly reorders the kernel's instructions (tools/device_asm_diff.py)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        fx = __fadd_rn(fx, __shfl_xor(fx, o)); fy = __fadd_rn(fy, __shfl_xor(fy, o)); fz = __fadd_rn(fz, __shfl_xor(fz, o));
    }
    if (lane == 0) { forces[3 * (size_t)n] = fx; forces[3 * (size_t)n + 1] = fy; forces[3 * (size_t)n + 2] = fz; }
}

// ------------------------------------------------------------------------------------------------ weight images
static size_t eg_al(size_t b) { return (b + 255) & ~(size_t)255; }
// arena of the weight images: per layer 11 H^2 elements x (forward hi | lo | frag 8 B + transposed f32, hi | lo | frag 12 B),
// the transposed rbf_proj.weight, and out_energy.0 transposed
static size_t eg_weight_bytes(const adf_painn* h) {
    const size_t H = h->hp.hidden_channels, L = h->hp.num_layers, R = h->hp.num_rbf;
    const size_t per_layer = eg_al(H * H * 20) + 2 * eg_al(2 * H * H * 20) + 2 * eg_al(3 * H * H * 20) + eg_al(3 * H * R * 4);
    return per_layer * L + eg_al(H / 2 * H * 12);
}

static int32_t eg_build_weights(adf_painn* h, adf_grad* g, hipStream_t s) {
    const long long H = h->hp.hidden_channels, L = h->hp.num_layers, R = h->hp.num_rbf, H2 = H / 2;
    struct Shape { long long n, k; };
    const Shape shp[EG_NW] = {{H, H}, {3 * H, H}, {2 * H, H}, {H, 2 * H}, {3 * H, H}};
    auto al = eg_al;
    const size_t bytes = eg_weight_bytes(h);
    if (!g->wscales) ADF_TRY(g->m_w.alloc(&g->wscales, (size_t)2 * EG_NW * ADF_MAX_LAYERS + 8));
    ADF_TRY(g->m_w.alloc(&g->warena, bytes));
    unsigned char* cur = g->warena;
    int nscale = 0;
    auto image = [&](const float* w, long long n, long long k, EgW* out) -> int32_t {   // split + fragment image of w [n, k]
        const long long e = n * k;
        out->f32 = w;
        out->w16 = adf_w16{};
        out->w16.hi = cur; out->w16.lo = cur + e * 2; out->w16.frag = cur + e * 4;
        cur += e * 8;
        out->w16.inv_scale = g->wscales + nscale++;
        ADF_TRY(adf_split_weight(w, e, &out->w16, h->w16_scratch, s));
        return adf_pack_frag(&out->w16, (int)n, (int)k, out->w16.frag, s);
    };
    auto transposed = [&](const float* w, long long n, long long k, EgW* out) -> int32_t {   // w [n, k] -> [k, n] + images
        float* t = reinterpret_cast<float*>(cur);
        cur += n * k * 4;
        hipLaunchKernelGGL(eg_transpose_kernel, dim3((unsigned)((k + 31) / 32), (unsigned)((n + 31) / 32)), dim3(32, 8), 0, s,
                           w, t, (int)n, (int)k);
        return image(t, k, n, out);
    };
    for (int l = 0; l < L; ++l) {
        const adf_layer_weights& lw = h->layer[l];
        const float* src[EG_NW] = {lw.xp0_w, lw.xp2_w, lw.vp_w, lw.xv0_w, lw.xv2_w};
        for (int i = 0; i < EG_NW; ++i) {
            unsigned char* start = cur;
            ADF_TRY(image(src[i], shp[i].n, shp[i].k, &g->fw[l][i]));
            ADF_TRY(transposed(src[i], shp[i].n, shp[i].k, &g->bw[l][i]));
            cur = start + al((size_t)shp[i].n * shp[i].k * 20);
        }
        g->rbf_wt[l] = reinterpret_cast<float*>(cur);
        hipLaunchKernelGGL(eg_transpose_kernel, dim3((unsigned)((R + 31) / 32), (unsigned)((3 * H + 31) / 32)), dim3(32, 8), 0, s,
                           lw.rbf_w, g->rbf_wt[l], (int)(3 * H), (int)R);
        cur += al((size_t)3 * H * R * 4);
    }
    ADF_TRY(transposed(h->oe0_w, H2, H, &g->oe_bw));
    ADF_HIP_CHECK(hipGetLastError());
    if ((size_t)(cur - g->warena) > bytes) { adf_set_error("internal: gradient weight arena overflow"); return ADF_EINVAL; }
    g->wvalid = true;
    return ADF_OK;
}

// C (+)= A W^T (+ bias) in the handle's arithmetic; tmp: [M, N] scratch for an accumulating product in exact f32
static int32_t eg_lin(adf_painn* h, const float* A, int lda, const EgW& w, const float* bias, float* C, int ldc, long long M,
                      int N, int K, hipStream_t s, int accumulate = 0, float* tmp = nullptr) {
    if (M * (long long)lda * 4 >= (1ll << 32) || M * (long long)ldc * 4 >= (1ll << 32)) {
        adf_set_error("energy gradient: %lld rows exceed the 32-bit offsets of the products, split the batch", M);
        return ADF_EOOM;
    }
    if (h->gemm_f32) {
        if (!accumulate) return adf_launch_gemm(A, lda, w.f32, K, bias, C, ldc, (int)M, N, K, 0, s);
        if (!tmp || ldc != N) { adf_set_error("internal: accumulating exact product needs contiguous scratch"); return ADF_EINVAL; }
        ADF_TRY(adf_launch_gemm(A, lda, w.f32, K, bias, tmp, N, (int)M, N, K, 0, s));
        hipLaunchKernelGGL(eg_add_kernel, dim3(eg_grid(M * N)), dim3(256), 0, s, tmp, C, M * N);
        ADF_HIP_CHECK(hipGetLastError());
        return ADF_OK;
    }
    adf_epi ep = {};
    ep.accumulate = accumulate;
    return adf_launch_gemm16(A, lda, &w.w16, bias, C, ldc, (int)M, N, K, 0, &ep, s, h->lift_on ? &h->lift : nullptr, h->sw.tune,
                             h->num_cus);
}

// ------------------------------------------------------------------------------------------------ workspace
struct EgLayer { float *x, *vec, *stats, *h0, *xh, *vv, *cat, *u0, *a, *dot; };
struct EgBufs {
    EgLayer layer[ADF_MAX_LAYERS];
    float *x_last, *he0;
    float *t1, *t2, *dx1, *dvec1, *dy;            // forward temporaries y, c, x1, vec1, ua live in these
    float *dxA, *dxB, *dvecA, *dvecB, *da, *ddot, *dv1, *dcat, *dvv, *dxh, *lnw, *lnscratch;
    size_t total;
};
static void eg_layout(long long N, int H, int L, float* base, EgBufs* b) {
    size_t off = 0;
    auto take = [&](long long floats) { float* p = base ? base + off : nullptr; off += ((size_t)floats + 63) & ~(size_t)63; return p; };
    const long long NH = N * H;
    for (int l = 0; l < L; ++l) {
        EgLayer& a = b->layer[l];
        a.x = take(NH); a.vec = l ? take(3 * NH) : nullptr; a.stats = take(2 * N); a.h0 = take(NH); a.xh = take(3 * NH);
        a.vv = take(6 * NH); a.cat = take(2 * NH); a.u0 = take(NH); a.a = take(3 * NH); a.dot = take(NH);
    }
    b->x_last = take(NH); b->he0 = take(NH / 2);
    b->t1 = take(NH); b->t2 = take(NH); b->dx1 = take(NH); b->dvec1 = take(3 * NH); b->dy = take(NH);
    b->dxA = take(NH); b->dxB = take(NH); b->dvecA = take(3 * NH); b->dvecB = take(3 * NH); b->da = take(3 * NH);
    b->ddot = take(NH); b->dv1 = take(3 * NH); b->dcat = take(2 * NH); b->dvv = take(6 * NH); b->dxh = take(3 * NH);
    b->lnw = take(2 * H); b->lnscratch = take((long long)512 * 2 * H + 64);
    b->total = off;
}

static long long eg_ecap(const adf_painn* h, long long N) { return 2 * N * h->hp.max_neighbors; }
// the fused message backward and the fused geometry kernel run together or not at all
static bool eg_fused(adf_painn* h) { return adf_message_geo_supported(h) && adf_op_message_bwd_fused_supported(h); }

extern "C" int32_t adf_painn_energy_gradient_workspace(adf_painn_t h, int64_t num_atoms, int64_t* bytes) {
    if (!h || !bytes || num_atoms <= 0) { adf_set_error("energy_gradient_workspace: bad argument"); return ADF_EINVAL; }
    EgBufs b;
    eg_layout(num_atoms, h->hp.hidden_channels, h->hp.num_layers, nullptr, &b);
    const long long ecap = eg_ecap(h, num_atoms);
    // the per-edge partials are sized for H / 64 slices whatever the arithmetic (the evaluation allocates room for either)
    *bytes = (int64_t)(b.total * sizeof(float) +
                       (size_t)ecap * ((h->hp.hidden_channels / ADF_SLICE_CH) * sizeof(float4) + sizeof(int32_t)) +
                       eg_weight_bytes(h));
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ the evaluation
extern "C" int32_t adf_painn_forward_energy_gradient(adf_painn_t h, const adf_batch* b, float* energy, float* forces,
                                                     void* stream) {
    if (!h || !b || !energy || !forces) { adf_set_error("forward_energy_gradient: null argument"); return ADF_EINVAL; }
    if (!h->weights_set || !h->energy_set) {
        adf_set_error("forward_energy_gradient: weights / energy head not set (adf_painn_set_weights, adf_painn_set_energy_head)");
        return ADF_EINVAL;
    }
    if (!b->atomic_numbers) { adf_set_error("forward_energy_gradient: null atomic numbers"); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    ADF_TRY(adf_graph_build(h, b, stream, nullptr));   // checks the batch, grows the handle's workspaces
    const int N = b->num_atoms, H = h->hp.hidden_channels, L = h->hp.num_layers, R = h->hp.num_rbf, H2 = H / 2;
    adf_grad* g = eg_state(h);
    if (!g) { adf_set_error("host allocation failed"); return ADF_EOOM; }
    if (!g->wvalid) ADF_TRY(eg_build_weights(h, g, s));
    const bool fused = eg_fused(h);
    const int nslices = fused ? H / ADF_SLICE_CH : 1;
    const long long ecap = eg_ecap(h, N);
    EgBufs w;
    eg_layout(N, H, L, nullptr, &w);
    if (w.total > g->act_floats || ecap > g->ecap || nslices > g->part_slices) {
        ADF_HIP_CHECK(hipDeviceSynchronize());   // enqueued work may still use the buffers
        g->m_ws.release();
        g->act_floats = 0; g->ecap = 0; g->part_slices = 0;
        const int sl = H / ADF_SLICE_CH;   // room for either arithmetic
        ADF_TRY(g->m_ws.alloc(&g->act, w.total));
        ADF_TRY(g->m_ws.alloc(&g->part, (size_t)ecap * sl));
        ADF_TRY(g->m_ws.alloc(&g->rev, (size_t)ecap));
        g->act_floats = w.total; g->ecap = ecap; g->part_slices = sl;
    }
    eg_layout(N, H, L, g->act, &w);
    const long long pstride = g->ecap;
    const size_t recrow = (size_t)(H / 32) * 160;

    // ---------------- forward, keeping what the backward reads
    ADF_TRY(adf_nodewise_embed(h, b->atomic_numbers, N, w.layer[0].x, s));
    for (int l = 0; l < L; ++l) {
        const adf_layer_weights& lw = h->layer[l];
        EgLayer& a = w.layer[l];
        const bool vz = l == 0;
        float* xn = l + 1 < L ? w.layer[l + 1].x : w.x_last;
        float* vn = l + 1 < L ? w.layer[l + 1].vec : w.dvecA;   // the last layer's vec feeds nothing the energy reads
        float *y = w.t1, *c = w.t2, *x1 = w.dx1, *vec1 = w.dvec1, *ua = w.dy;
        ADF_TRY(adf_op_layernorm_fwd(a.x, lw.ln_w, lw.ln_b, y, a.stats, N, H, stream));
        ADF_TRY(eg_lin(h, y, H, g->fw[l][EG_XP0], lw.xp0_b, a.h0, H, N, H, H, s));
        ADF_TRY(adf_op_ssilu_fwd(a.h0, c, (int64_t)N * H, stream));
        ADF_TRY(eg_lin(h, c, H, g->fw[l][EG_XP2], lw.xp2_b, a.xh, 3 * H, N, 3 * H, H, s));
        ADF_HIP_CHECK(hipMemsetAsync(h->rec + (size_t)N * recrow, 0, sizeof(float) * recrow, s));
        ADF_TRY(adf_pack_records(h, N, a.xh, a.vec, vz, s));
        {   // profiling of a gradient evaluation times and counts the geometry kernel alone: the forward message kernel
            // must not add its k-steps to the handle's one counter
            const bool prof = h->prof.on;
            h->prof.on = false;
            const int32_t st = adf_message_impl(h, l, N, a.x, a.xh, a.vec, x1, vec1, vz, s);
            h->prof.on = prof;
            ADF_TRY(st);
        }
        ADF_TRY(eg_lin(h, vec1, H, g->fw[l][EG_VP], nullptr, a.vv, 2 * H, 3ll * N, 2 * H, H, s));
        ADF_TRY(adf_op_copy_rows(x1, H, a.cat, 2 * H, N, H, 0, stream));
        ADF_TRY(adf_op_vdot_fwd(a.vv, a.dot, a.cat + H, 2 * H, N, H, 1e-8f, stream));
        ADF_TRY(eg_lin(h, a.cat, 2 * H, g->fw[l][EG_XV0], lw.xv0_b, a.u0, H, N, H, 2 * H, s));
        ADF_TRY(adf_op_ssilu_fwd(a.u0, ua, (int64_t)N * H, stream));
        ADF_TRY(eg_lin(h, ua, H, g->fw[l][EG_XV2], lw.xv2_b, a.a, 3 * H, N, 3 * H, H, s));
        ADF_TRY(adf_op_update_out_fwd(x1, vec1, a.a, a.dot, a.vv, h->scale[l], xn, vn, N, H, stream));
    }
    // energy head: he0 kept (pre-activation), ScaledSiLU, the fixed-order per-system sum of adf_painn_forward_energy
    ADF_TRY(adf_linear(h, w.x_last, H, h->oe0_w, &h->oe0_16, h->oe0_b, w.he0, H2, N, H2, H, 0, s));
    ADF_TRY(adf_op_ssilu_fwd(w.he0, w.t1, (int64_t)N * H2, stream));
    ADF_TRY(adf_energy_sum(w.t1, H2, h->oe2_w, h->oe2_b, b->atom_offset, energy, b->num_systems, s));

    // ---------------- backward: seed, then the layers from the last to the first (data gradients only)
    float *dx = w.dxA, *dx_in = w.dxB, *dvec = w.dvecA, *dvec_in = w.dvecB;
    hipLaunchKernelGGL(eg_seed_kernel, dim3(eg_grid((long long)N * H2)), dim3(256), 0, s, w.he0, h->oe2_w, w.ddot, (long long)N, H2);
    ADF_HIP_CHECK(hipGetLastError());
    ADF_TRY(eg_lin(h, w.ddot, H2, g->oe_bw, nullptr, dx, H, N, H, H2, s));
    ADF_HIP_CHECK(hipMemsetAsync(dvec, 0, sizeof(float) * 3 * (size_t)N * H, s));
    const double step = 1.0 / (R - 1), pe = (double)h->hp.envelope_exponent;
    for (int l = L - 1; l >= 0; --l) {
        const adf_layer_weights& lw = h->layer[l];
        EgLayer& a = w.layer[l];
        const bool vz = l == 0;
        // update block
        ADF_TRY(adf_op_update_out_bwd(a.a, a.dot, a.vv, h->scale[l], dx, dvec, w.da, w.ddot, w.dv1, w.dx1, w.dvec1, N, H, stream));
        ADF_TRY(eg_lin(h, w.da, 3 * H, g->bw[l][EG_XV2], nullptr, w.t1, H, N, H, 3 * H, s));
        ADF_TRY(adf_op_ssilu_bwd(a.u0, w.t1, w.t2, (int64_t)N * H, stream));
        ADF_TRY(eg_lin(h, w.t2, H, g->bw[l][EG_XV0], nullptr, w.dcat, 2 * H, N, 2 * H, H, s));
        ADF_TRY(adf_op_copy_rows(w.dcat, 2 * H, w.dx1, H, N, H, 1, stream));
        ADF_TRY(adf_op_vdot_bwd(a.vv, a.cat + H, 2 * H, w.ddot, w.dcat + H, 2 * H, w.dv1, w.dvv, N, H, stream));
        ADF_TRY(eg_lin(h, w.dvv, 2 * H, g->bw[l][EG_VP], nullptr, w.dvec1, H, 3ll * N, H, 2 * H, s, 1, w.dv1));
        // message block: node-side gradients and the edge-geometry gradient
        if (fused) {
            if (!vz) {
                ADF_TRY(adf_op_message_bwd_fused(h, l, a.xh, a.vec, w.dx1, w.dvec1, w.dxh, nullptr, ecap, dvec_in, dx_in, 0,
                                                 w.da, stream));   // (w.da: the bias-gradient rows nobody reads here)
            } else {
                ADF_TRY(adf_pack_grad_records(h, w.dx1, w.dvec1, nullptr, s));
            }
            ADF_TRY(adf_message_geo(h, l, a.xh, a.vec, vz, g->part, pstride, l != L - 1, s));
        } else {
            hipLaunchKernelGGL(eg_msg_bwd_plain_kernel, dim3((unsigned)N), dim3(256), 0, s, h->nptr, h->e_src, h->e_geom, a.xh,
                               a.vec, g->rbf_wt[l], lw.rbf_b, h->rbf_offset, R, 1.0f / h->hp.cutoff,
                               (float)(-0.5 / (step * step)), (float)(-(pe + 1) * (pe + 2) / 2), (float)(pe * (pe + 2)),
                               (float)(-pe * (pe + 1) / 2), h->hp.envelope_exponent, w.dx1, w.dvec1, w.dxh, dvec_in, dx_in,
                               g->part, H, vz ? 1 : 0, l != L - 1 ? 1 : 0);
            ADF_HIP_CHECK(hipGetLastError());
        }
        if (vz) break;   // x entering layer 0 is the embedding: no dependence on the positions
        ADF_TRY(eg_lin(h, w.dxh, 3 * H, g->bw[l][EG_XP2], nullptr, w.t1, H, N, H, 3 * H, s));
        ADF_TRY(adf_op_ssilu_bwd(a.h0, w.t1, w.t2, (int64_t)N * H, stream));
        ADF_TRY(eg_lin(h, w.t2, H, g->bw[l][EG_XP0], nullptr, w.dy, H, N, H, H, s));
        ADF_TRY(adf_op_layernorm_bwd(a.x, lw.ln_w, a.stats, w.dy, dx_in, w.lnw, w.lnw + H, N, H, w.lnscratch, stream));
        float* t = dx; dx = dx_in; dx_in = t;
        t = dvec; dvec = dvec_in; dvec_in = t;
    }
    // ---------------- per-edge gradients -> forces
    hipLaunchKernelGGL(eg_reverse_index_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, h->nptr, h->e_src, h->e_geom, N,
                       g->rev, h->flags);
    hipLaunchKernelGGL(eg_position_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, h->nptr, h->e_geom, g->rev, g->part,
                       pstride, nslices, N, forces);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}
