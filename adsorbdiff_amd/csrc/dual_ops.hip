// Dual (primal, tangent) forms of the PaiNN training step's nonlinear operators: what PaiNNGradForceTrainStep
// (adsorbdiff_amd/train_step.py) strings together to train on forces that are the gradient of the energy.
//
// The force term of that objective is differentiated as  grad_theta L_F = -grad_theta D,  D = d/d eps sum_b E_b(pos + eps v)
// at eps = 0 with v = dL/dF held constant: D is one tangent forward in which every activation a carries a_dot, and the whole
// gradient is one reverse pass through the joint (primal, tangent) graph.  An operator y = f(x) becomes
//     forward:   (y, y_dot = J x_dot)
//     backward:  x_bar = J^T y_bar + (d/dx [J x_dot])^T y_dot_bar,   x_dot_bar = J^T y_dot_bar   (+ the parameter terms)
// A DUAL OPERAND holds its primal block followed by its tangent block ("stacked"), so that the linear layers in between run
// as one product over twice the rows (adf_op_linear_fwd / adf_op_linear_bwd, train.hip).  Exact f32, one launch per
// direction, no float atomics: every sum runs in a fixed order.
#include "common.h"
#include "dual_ops.h"

#define DU_CHECK_LAUNCH() ADF_HIP_CHECK(hipGetLastError())

static inline unsigned du_grid(long long total, int per_block = 256) {
    long long b = (total + per_block - 1) / per_block;
    if (b > 256 * 16) b = 256 * 16;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// ------------------------------------------------------------------------------------------------ edge tangents
// Row e of atom i's segment holds the edge vector r = pos[src] - pos[i] + offset as (u, d).  Under pos + eps v:
//     delta = v[src] - v[i];   d_dot = u . delta;   u_dot = (delta - u (u . delta)) / d
// and where the distance floor holds d is a constant: d_dot = 0, u_dot = delta / d.  e_tan[e] = (u_dot, d_dot).  The two rows
// of a pair get exactly negated u_dot and the same d_dot bits (negated operands in the same order).  One wave per atom.
__global__ __launch_bounds__(256) void du_edge_tangent_kernel(const int32_t* __restrict__ nptr, const int32_t* __restrict__ e_src,
                                                               const float4* __restrict__ e_geom, const float* __restrict__ v,
                                                               float4* __restrict__ e_tan, int N, long long E, float floor_) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    const float vx = v[3 * (size_t)i], vy = v[3 * (size_t)i + 1], vz = v[3 * (size_t)i + 2];
    for (long long e = nptr[i] + lane; e < nptr[i + 1] && e < E; e += 64) {
        const int j = e_src[e];
        const float4 g = e_geom[e];
        const float dx = __fsub_rn(v[3 * (size_t)j], vx), dy = __fsub_rn(v[3 * (size_t)j + 1], vy),
                    dz = __fsub_rn(v[3 * (size_t)j + 2], vz);
        const float p = fmaf(g.z, dz, fmaf(g.y, dy, __fmul_rn(g.x, dx)));
        const bool floored = g.w <= floor_;
        const float inv = __fdiv_rn(1.0f, g.w), q = floored ? 0.f : p;
        e_tan[e] = make_float4(__fmul_rn(fmaf(-q, g.x, dx), inv), __fmul_rn(fmaf(-q, g.y, dy), inv),
                               __fmul_rn(fmaf(-q, g.z, dz), inv), q);
    }
}
extern "C" int32_t adf_op_edge_tangent(adf_painn_t h, const float* v, float* e_tan, int64_t num_edges, void* stream) {
    if (!h || h->lastN <= 0 || !v || !e_tan || num_edges < 0) { adf_set_error("edge_tangent: bad argument or no graph"); return ADF_EINVAL; }
    const int N = (int)h->lastN;
    hipLaunchKernelGGL(du_edge_tangent_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, h->nptr, h->e_src,
                       h->e_geom, v, reinterpret_cast<float4*>(e_tan), N, (long long)num_edges, h->dist_floor);
    DU_CHECK_LAUNCH();
    return ADF_OK;
}

// The radial basis of tr_rbf_kernel (train.hip) and its tangent rbf'(d) d_dot: rbf2 [2 E, R], primal rows then tangent rows.
// Nothing is differentiated with respect to the basis: positions are not parameters.
__global__ void du_rbf_kernel(const float4* __restrict__ e_geom, const float4* __restrict__ e_tan, long long E,
                              const float* __restrict__ mu, int R, float inv_cutoff, float coeff, float env_a, float env_b,
                              float env_c, int env_pi, float* __restrict__ rbf2) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < E * R; t += (long long)gridDim.x * blockDim.x) {
        const long long e = t / R;
        const int k = (int)(t - e * R);
        const float xs = e_geom[e].w * inv_cutoff;
        float xq = 1.0f;
        for (int i = 1; i < env_pi; ++i) xq *= xs;
        const float xp = xq * xs, pe = (float)env_pi;
        float env = 1.0f + env_a * xp + env_b * (xp * xs) + env_c * (xp * xs * xs);
        float envd = env_a * pe * xq + env_b * (pe + 1.0f) * xp + env_c * (pe + 2.0f) * (xp * xs);
        if (!(xs < 1.0f)) { env = 0.f; envd = 0.f; }
        const float dm = xs - mu[k];
        const float ga = expf(coeff * dm * dm);
        rbf2[t] = env * ga;
        rbf2[(size_t)E * R + t] = (envd + env * 2.0f * coeff * dm) * ga * inv_cutoff * e_tan[e].w;
    }
}
extern "C" int32_t adf_op_rbf_dual(adf_painn_t h, const float* e_tan, float* rbf2, int64_t num_edges, void* stream) {
    if (!h || h->lastN <= 0 || !h->weights_set || !e_tan || !rbf2 || num_edges < 0) {
        adf_set_error("rbf_dual: bad argument, no graph or no weights");
        return ADF_EINVAL;
    }
    const int R = h->hp.num_rbf;
    const double step = 1.0 / (R - 1), pe = (double)h->hp.envelope_exponent;
    hipLaunchKernelGGL(du_rbf_kernel, dim3(du_grid((long long)num_edges * R)), dim3(256), 0, (hipStream_t)stream, h->e_geom,
                       reinterpret_cast<const float4*>(e_tan), (long long)num_edges, h->rbf_offset, R, 1.0f / h->hp.cutoff,
                       (float)(-0.5 / (step * step)), (float)(-(pe + 1) * (pe + 2) / 2), (float)(pe * (pe + 2)),
                       (float)(-pe * (pe + 1) / 2), h->hp.envelope_exponent, rbf2);
    DU_CHECK_LAUNCH();
    return ADF_OK;
}

// y[m, :] += bias for the first M rows of a stacked product: the tangent rows of a linear layer take no bias
__global__ void du_bias_kernel(float* __restrict__ y, int ldy, const float* __restrict__ bias, long long M, int N) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < M * N; t += (long long)gridDim.x * blockDim.x) {
        const long long m = t / N;
        const int c = (int)(t - m * N);
        y[(size_t)m * ldy + c] += bias[c];
    }
}
extern "C" int32_t adf_op_dual_bias(float* y, int32_t ldy, const float* bias, int64_t M, int32_t N, void* stream) {
    if (!y || !bias || M < 0 || N <= 0 || ldy < N) { adf_set_error("dual_bias: bad argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(du_bias_kernel, dim3(du_grid(M * N)), dim3(256), 0, (hipStream_t)stream, y, ldy, bias, (long long)M, N);
    DU_CHECK_LAUNCH();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ ScaledSiLU
// f = x sigmoid(x) / 0.6;  f' = sg (1 + x (1 - sg)) / 0.6;  f'' = sg (1 - sg) (2 + x (1 - 2 sg)) / 0.6
__device__ __forceinline__ float du_d2ssilu(float x) {
    const float sg = 1.0f / (1.0f + expf(-x));
    return sg * (1.0f - sg) * (2.0f + x * (1.0f - 2.0f * sg)) * 1.6666666666666667f;
}
__global__ void du_ssilu_fwd_kernel(const float* __restrict__ h2, float* __restrict__ y2, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float h = h2[i];
        y2[i] = adf_ssilu(h);
        y2[n + i] = adf_dssilu(h) * h2[n + i];
    }
}
__global__ void du_ssilu_bwd_kernel(const float* __restrict__ h2, const float* __restrict__ dy2, float* __restrict__ dh2,
                                    long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float h = h2[i], d1 = adf_dssilu(h), gd = dy2[n + i];
        dh2[i] = dy2[i] * d1 + gd * du_d2ssilu(h) * h2[n + i];
        dh2[n + i] = gd * d1;
    }
}
extern "C" int32_t adf_op_ssilu_dual_fwd(const float* h2, float* y2, int64_t n, void* stream) {
    if (!h2 || !y2 || n < 0) { adf_set_error("ssilu_dual_fwd: bad argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(du_ssilu_fwd_kernel, dim3(du_grid(n)), dim3(256), 0, (hipStream_t)stream, h2, y2, (long long)n);
    DU_CHECK_LAUNCH();
    return ADF_OK;
}
extern "C" int32_t adf_op_ssilu_dual_bwd(const float* h2, const float* dy2, float* dh2, int64_t n, void* stream) {
    if (!h2 || !dy2 || !dh2 || n < 0) { adf_set_error("ssilu_dual_bwd: bad argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(du_ssilu_bwd_kernel, dim3(du_grid(n)), dim3(256), 0, (hipStream_t)stream, h2, dy2, dh2, (long long)n);
    DU_CHECK_LAUNCH();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ LayerNorm
// One wave per row, the corrected two-pass moments of tr_ln_fwd_kernel (train.hip): the primal rows are that kernel's.
//     xhat = (x - mean) rstd;   xhat_dot = rstd (a - mean(a) - xhat mean(xhat a)),  a = x_dot;   y_dot = xhat_dot w
__global__ __launch_bounds__(256) void du_ln_fwd_kernel(const float* __restrict__ x2, const float* __restrict__ w,
                                                         const float* __restrict__ b, float* __restrict__ y2,
                                                         float2* __restrict__ stats, int N, int H) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const size_t tan = (size_t)N * H;
    const float* xr = x2 + (size_t)row * H;
    const float* ar = xr + tan;
    float s = 0.f;
    for (int c = lane; c < H; c += 64) s += xr[c];
    const float m0 = adf_wave_sum(s) / (float)H;
    float q = 0.f, r = 0.f;
    for (int c = lane; c < H; c += 64) { const float d = xr[c] - m0; q += d * d; r += d; }
    const float cm = adf_wave_sum(r) / (float)H;
    const float rstd = 1.0f / sqrtf(fmaxf(adf_wave_sum(q) / (float)H - cm * cm, 0.f) + 1e-5f);
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < H; c += 64) {
        const float xh = ((xr[c] - m0) - cm) * rstd, a = ar[c];
        s1 += a; s2 += xh * a;
    }
    const float m1 = adf_wave_sum(s1) / (float)H, m2 = adf_wave_sum(s2) / (float)H;
    for (int c = lane; c < H; c += 64) {
        const float xh = ((xr[c] - m0) - cm) * rstd;
        y2[(size_t)row * H + c] = xh * w[c] + b[c];
        y2[tan + (size_t)row * H + c] = rstd * (ar[c] - m1 - xh * m2) * w[c];
    }
    if (lane == 0) stats[row] = make_float2(m0 + cm, rstd);
}
// With P(g) = rstd (g - mean(g) - xhat mean(g xhat)) (the symmetric Jacobian), g = dy w, gd = dy_dot w:
//     dx_dot += P(gd)
//     dx     += P(g) - rstd (xhat u + P(gd) m2 + q xhat_dot),   u = mean(gd xhat_dot), m2 = mean(xhat a), q = mean(gd xhat)
//     dw = sum_rows dy xhat + dy_dot xhat_dot;   db = sum_rows dy.   Partial [dw | db] rows go to part[blocks][2H].
__global__ __launch_bounds__(256) void du_ln_bwd_kernel(const float* __restrict__ x2, const float* __restrict__ w,
                                                         const float2* __restrict__ stats, const float* __restrict__ dy2,
                                                         float* __restrict__ dx2, float* __restrict__ part, int N, int H,
                                                         int rows_per_block) {
    extern __shared__ float sh[];  // [4 waves][2H]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* mine = sh + wave * 2 * H;
    for (int c = lane; c < 2 * H; c += 64) mine[c] = 0.f;
    const size_t tan = (size_t)N * H;
    const float ih = 1.0f / (float)H;
    const int r0 = blockIdx.x * rows_per_block;
    for (int row = r0 + wave; row < min(N, r0 + rows_per_block); row += 4) {
        const float2 st = stats[row];
        const float* xr = x2 + (size_t)row * H;
        const float* ar = xr + tan;
        const float* gr = dy2 + (size_t)row * H;
        const float* hr = gr + tan;
        float r = 0.f;
        for (int c = lane; c < H; c += 64) r += xr[c] - st.x;
        const float cm = adf_wave_sum(r) * ih;
        float sg = 0.f, sgx = 0.f, sd = 0.f, sq = 0.f, sa = 0.f, sT = 0.f, sA = 0.f;
        for (int c = lane; c < H; c += 64) {
            const float xh = ((xr[c] - st.x) - cm) * st.y, g = gr[c] * w[c], gd = hr[c] * w[c], a = ar[c];
            sg += g; sgx += g * xh; sd += gd; sq += gd * xh; sa += a; sT += xh * a; sA += gd * a;
        }
        const float mg = adf_wave_sum(sg) * ih, mgx = adf_wave_sum(sgx) * ih, mgd = adf_wave_sum(sd) * ih;
        const float q = adf_wave_sum(sq) * ih, m1 = adf_wave_sum(sa) * ih, m2 = adf_wave_sum(sT) * ih;
        const float u = st.y * (adf_wave_sum(sA) * ih - mgd * m1 - q * m2);
        for (int c = lane; c < H; c += 64) {
            const float xh = ((xr[c] - st.x) - cm) * st.y, g = gr[c] * w[c], gd = hr[c] * w[c];
            const float xhd = st.y * (ar[c] - m1 - xh * m2);
            const float pg = st.y * (g - mg - xh * mgx), pgd = st.y * (gd - mgd - xh * q);
            dx2[(size_t)row * H + c] += pg - st.y * (xh * u + pgd * m2 + q * xhd);
            dx2[tan + (size_t)row * H + c] += pgd;
            mine[c] += gr[c] * xh + hr[c] * xhd;   // dw
            mine[H + c] += gr[c];                  // db
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * H; c += 256)
        part[(size_t)blockIdx.x * 2 * H + c] = sh[c] + sh[2 * H + c] + sh[4 * H + c] + sh[6 * H + c];
}
// dst[i] = sum_s part[s][i] in ascending s
__global__ void du_reduce_rows_kernel(const float* __restrict__ part, long long stride, float* __restrict__ dst, long long n,
                                      int rows) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int k = 0; k < rows; ++k) s += part[(size_t)k * stride + i];
        dst[i] = s;
    }
}
extern "C" int32_t adf_op_layernorm_dual_fwd(const float* x2, const float* w, const float* b, float* y2, float* stats, int32_t N,
                                             int32_t H, void* stream) {
    if (!x2 || !w || !b || !y2 || !stats || N <= 0 || H <= 0) { adf_set_error("layernorm_dual_fwd: bad argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(du_ln_fwd_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, x2, w, b, y2,
                       reinterpret_cast<float2*>(stats), N, H);
    DU_CHECK_LAUNCH();
    return ADF_OK;
}
// dx2 is ACCUMULATED into; dw, db [H] are written.  scratch: 512 * 2H floats, as adf_op_layernorm_bwd.
extern "C" int32_t adf_op_layernorm_dual_bwd(const float* x2, const float* w, const float* stats, const float* dy2, float* dx2,
                                             float* dw, float* db, int32_t N, int32_t H, float* scratch, void* stream) {
    if (!x2 || !w || !stats || !dy2 || !dx2 || !dw || !db || !scratch || N <= 0 || H <= 0 || H > 1024) {
        adf_set_error("layernorm_dual_bwd: bad argument");
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    int blocks = (N + 63) / 64;
    if (blocks > 512) blocks = 512;
    if (blocks < 1) blocks = 1;
    const int rows = (N + blocks - 1) / blocks;
    hipLaunchKernelGGL(du_ln_bwd_kernel, dim3(blocks), dim3(256), sizeof(float) * 8 * H, s, x2, w,
                       reinterpret_cast<const float2*>(stats), dy2, dx2, scratch, N, H, rows);
    hipLaunchKernelGGL(du_reduce_rows_kernel, dim3(du_grid(H)), dim3(256), 0, s, scratch, (long long)2 * H, dw, (long long)H, blocks);
    hipLaunchKernelGGL(du_reduce_rows_kernel, dim3(du_grid(H)), dim3(256), 0, s, scratch + H, (long long)2 * H, db, (long long)H,
                       blocks);
    DU_CHECK_LAUNCH();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ update block
// vv [N,3,2C] = (v1 | v2):  dot = sum_k v1 v2 / sqrtC,  nrm = sqrt(sum_k v2^2 + eps)
//     dot_dot = sum_k (v1_dot v2 + v1 v2_dot) / sqrtC,   nrm_dot = sum_k v2 v2_dot / nrm
// nrm2 is written with row stride ldn, its tangent block N * ldn floats behind the primal one.
__global__ void du_vdot_fwd_kernel(const float* __restrict__ vv2, float* __restrict__ dot2, float* __restrict__ nrm2, int ldn,
                                   long long N, int C, float eps) {
    const float isc = 1.0f / sqrtf((float)C);
    const size_t tvv = (size_t)N * 6 * C, tdot = (size_t)N * C, tn = (size_t)N * ldn;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < N * C; t += (long long)gridDim.x * blockDim.x) {
        const long long n = t / C;
        const int c = (int)(t - n * C);
        float d = 0.f, q = 0.f, dd = 0.f, qd = 0.f;
        for (int k = 0; k < 3; ++k) {
            const size_t o = ((size_t)n * 3 + k) * 2 * C + c;
            const float a = vv2[o], b = vv2[o + C], ad = vv2[tvv + o], bd = vv2[tvv + o + C];
            d += a * b; q += b * b; dd += ad * b + a * bd; qd += b * bd;
        }
        const float nv = sqrtf(q + eps);
        dot2[t] = d * isc;
        dot2[tdot + t] = dd * isc;
        nrm2[(size_t)n * ldn + c] = nv;
        nrm2[tn + (size_t)n * ldn + c] = qd / nv;
    }
}
// dvv2 from (ddot2, dnrm2 [stride lddn]) plus an optional direct gradient of v1 (dv1_2 [2][N,3,C], may be null)
__global__ void du_vdot_bwd_kernel(const float* __restrict__ vv2, const float* __restrict__ nrm2, int ldn,
                                   const float* __restrict__ ddot2, const float* __restrict__ dnrm2, int lddn,
                                   const float* __restrict__ dv1_2, float* __restrict__ dvv2, long long N, int C) {
    const float isc = 1.0f / sqrtf((float)C);
    const size_t tvv = (size_t)N * 6 * C, tdot = (size_t)N * C, tdn = (size_t)N * lddn, tv1 = (size_t)N * 3 * C;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < N * C; t += (long long)gridDim.x * blockDim.x) {
        const long long n = t / C;
        const int c = (int)(t - n * C);
        const float dd = ddot2[t] * isc, ddd = ddot2[tdot + t] * isc;
        const float inv = 1.0f / nrm2[(size_t)n * ldn + c];
        const float dn = dnrm2[(size_t)n * lddn + c] * inv, dnd = dnrm2[tdn + (size_t)n * lddn + c] * inv;
        float qd = 0.f;
        for (int k = 0; k < 3; ++k) {
            const size_t o = ((size_t)n * 3 + k) * 2 * C + c;
            qd += vv2[o + C] * vv2[tvv + o + C];
        }
        const float corr = dnd * qd * inv * inv;
        for (int k = 0; k < 3; ++k) {
            const size_t o = ((size_t)n * 3 + k) * 2 * C + c, p = ((size_t)n * 3 + k) * C + c;
            const float a = vv2[o], b = vv2[o + C], ad = vv2[tvv + o], bd = vv2[tvv + o + C];
            dvv2[o] = dd * b + ddd * bd + (dv1_2 ? dv1_2[p] : 0.f);
            dvv2[tvv + o] = ddd * b + (dv1_2 ? dv1_2[tv1 + p] : 0.f);
            dvv2[o + C] = dd * a + ddd * ad + dn * b + dnd * bd - corr * b;
            dvv2[tvv + o + C] = ddd * a + dnd * b;
        }
    }
}
extern "C" int32_t adf_op_vdot_dual_fwd(const float* vv2, float* dot2, float* nrm2, int32_t ldn, int64_t N, int32_t C, float eps,
                                        void* stream) {
    if (!vv2 || !dot2 || !nrm2 || N < 0 || C <= 0 || ldn < C) { adf_set_error("vdot_dual_fwd: bad argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(du_vdot_fwd_kernel, dim3(du_grid(N * C)), dim3(256), 0, (hipStream_t)stream, vv2, dot2, nrm2, ldn,
                       (long long)N, C, eps);
    DU_CHECK_LAUNCH();
    return ADF_OK;
}
extern "C" int32_t adf_op_vdot_dual_bwd(const float* vv2, const float* nrm2, int32_t ldn, const float* ddot2, const float* dnrm2,
                                        int32_t lddn, const float* dv1_2, float* dvv2, int64_t N, int32_t C, void* stream) {
    if (!vv2 || !nrm2 || !ddot2 || !dnrm2 || !dvv2 || N < 0 || C <= 0 || ldn < C || lddn < C) {
        adf_set_error("vdot_dual_bwd: bad argument");
        return ADF_EINVAL;
    }
    hipLaunchKernelGGL(du_vdot_bwd_kernel, dim3(du_grid(N * C)), dim3(256), 0, (hipStream_t)stream, vv2, nrm2, ldn, ddot2, dnrm2,
                       lddn, dv1_2, dvv2, (long long)N, C);
    DU_CHECK_LAUNCH();
    return ADF_OK;
}

// x2 = (x1 + (a1 + a2 dot) / sqrt2) s;  vec2 = vec1 + a3 (x) v1   and their tangents (product rule on a2 dot and a3 v1)
__global__ void du_upd_out_fwd_kernel(const float* __restrict__ x1, const float* __restrict__ vec1, const float* __restrict__ a,
                                      const float* __restrict__ dot, const float* __restrict__ vv, float s,
                                      float* __restrict__ x2, float* __restrict__ vec2, long long N, int H) {
    const float is2 = 0.70710678118654752f;
    const size_t tx = (size_t)N * H, tv = (size_t)N * 3 * H, tvv = (size_t)N * 6 * H;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < N * H; t += (long long)gridDim.x * blockDim.x) {
        const long long n = t / H;
        const int c = (int)(t - n * H);
        const float* ar = a + (size_t)n * 3 * H;
        const float* adr = ar + tv;
        const float a2 = ar[H + c], a3 = ar[2 * H + c], a3d = adr[2 * H + c], dt = dot[t];
        x2[t] = (x1[t] + (ar[c] + a2 * dt) * is2) * s;
        x2[tx + t] = (x1[tx + t] + (adr[c] + adr[H + c] * dt + a2 * dot[tx + t]) * is2) * s;
        for (int k = 0; k < 3; ++k) {
            const size_t o = ((size_t)n * 3 + k) * H + c, p = ((size_t)n * 3 + k) * 2 * H + c;
            vec2[o] = vec1[o] + a3 * vv[p];
            vec2[tv + o] = vec1[tv + o] + a3d * vv[p] + a3 * vv[tvv + p];
        }
    }
}
// given dx2, dvec2 (dual): da [2][N,3H], ddot [2][N,H], dv1 [2][N,3,H], dx1 [2][N,H], dvec1 [2][N,3,H] written
__global__ void du_upd_out_bwd_kernel(const float* __restrict__ a, const float* __restrict__ dot, const float* __restrict__ vv,
                                      float s, const float* __restrict__ dx2, const float* __restrict__ dvec2,
                                      float* __restrict__ da, float* __restrict__ ddot, float* __restrict__ dv1,
                                      float* __restrict__ dx1, float* __restrict__ dvec1, long long N, int H) {
    const float is2 = 0.70710678118654752f;
    const size_t tx = (size_t)N * H, tv = (size_t)N * 3 * H, tvv = (size_t)N * 6 * H;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < N * H; t += (long long)gridDim.x * blockDim.x) {
        const long long n = t / H;
        const int c = (int)(t - n * H);
        const float* ar = a + (size_t)n * 3 * H;
        const float* adr = ar + tv;
        const float a2 = ar[H + c], a2d = adr[H + c], a3 = ar[2 * H + c], a3d = adr[2 * H + c];
        const float dt = dot[t], dtd = dot[tx + t];
        const float g = dx2[t] * s, gd = dx2[tx + t] * s;
        float* dr = da + (size_t)n * 3 * H;
        float* ddr = dr + tv;
        dr[c] = g * is2;
        ddr[c] = gd * is2;
        dr[H + c] = (g * dt + gd * dtd) * is2;
        ddr[H + c] = gd * dt * is2;
        ddot[t] = (g * a2 + gd * a2d) * is2;
        ddot[tx + t] = gd * a2 * is2;
        dx1[t] = g;
        dx1[tx + t] = gd;
        float d3 = 0.f, d3d = 0.f;
        for (int k = 0; k < 3; ++k) {
            const size_t o = ((size_t)n * 3 + k) * H + c, p = ((size_t)n * 3 + k) * 2 * H + c;
            const float gv = dvec2[o], gvd = dvec2[tv + o];
            d3 += gv * vv[p] + gvd * vv[tvv + p];
            d3d += gvd * vv[p];
            dv1[o] = gv * a3 + gvd * a3d;
            dv1[tv + o] = gvd * a3;
            dvec1[o] = gv;
            dvec1[tv + o] = gvd;
        }
        dr[2 * H + c] = d3;
        ddr[2 * H + c] = d3d;
    }
}
extern "C" int32_t adf_op_update_out_dual_fwd(const float* x1_2, const float* vec1_2, const float* a2, const float* dot2,
                                              const float* vv2, float s, float* x2_2, float* vec2_2, int64_t N, int32_t H,
                                              void* stream) {
    if (!x1_2 || !vec1_2 || !a2 || !dot2 || !vv2 || !x2_2 || !vec2_2 || N < 0 || H <= 0) {
        adf_set_error("update_out_dual_fwd: bad argument");
        return ADF_EINVAL;
    }
    hipLaunchKernelGGL(du_upd_out_fwd_kernel, dim3(du_grid(N * H)), dim3(256), 0, (hipStream_t)stream, x1_2, vec1_2, a2, dot2, vv2,
                       s, x2_2, vec2_2, (long long)N, H);
    DU_CHECK_LAUNCH();
    return ADF_OK;
}
extern "C" int32_t adf_op_update_out_dual_bwd(const float* a2, const float* dot2, const float* vv2, float s, const float* dx2_2,
                                              const float* dvec2_2, float* da2, float* ddot2, float* dv1_2, float* dx1_2,
                                              float* dvec1_2, int64_t N, int32_t H, void* stream) {
    if (!a2 || !dot2 || !vv2 || !dx2_2 || !dvec2_2 || !da2 || !ddot2 || !dv1_2 || !dx1_2 || !dvec1_2 || N < 0 || H <= 0) {
        adf_set_error("update_out_dual_bwd: bad argument");
        return ADF_EINVAL;
    }
    hipLaunchKernelGGL(du_upd_out_bwd_kernel, dim3(du_grid(N * H)), dim3(256), 0, (hipStream_t)stream, a2, dot2, vv2, s, dx2_2,
                       dvec2_2, da2, ddot2, dv1_2, dx1_2, dvec1_2, (long long)N, H);
    DU_CHECK_LAUNCH();
    return ADF_OK;
}
