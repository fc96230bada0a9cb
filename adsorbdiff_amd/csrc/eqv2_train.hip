// Training operators of the EquiformerV2 denoiser: the edge side of a step, forward and backward, as
// stateless adf_op_eq_* entries on caller-owned float32 buffers.  The handle is read for its dimensions (eq_dims) and its
// constant tables (to_red / from_red, the bound atom_radii) only.
//
// Reference (adsorbdiff/models/equiformer_v2/): rotate in / out so3.py:493-506, SO(2) convolution so2_ops.py:158-262,
// separable S2 activation activation.py:155-202, attention weights transformer_block.py:312-345, edge-degree embedding
// input_block.py:84-138, radial function radial_function.py:11-32.  oracle/eqv2_oracle.py restates each piece.
//
// Plain kernels, one per stage and direction: exact f32 (no split products), no float atomics, every sum over edges, rows
// or chunks in one fixed order - two calls on the same input give the same bits.  Layouts as in eqv2_kernels.hip, except
// that a tensor in the edges' frames is ONE buffer [E, S_r, W] with the coefficients order-major (eq_dims::r_m / r_sgn /
// r_l), not one buffer per order, and that an entry works on all E edges at once (no chunks of targets).
#include "eqv2.h"
#include "eqv2_train.h"

#define EQT_FOR_L(L_, MACRO) \
    switch (L_) {            \
        case 1: MACRO(1); break; \
        case 2: MACRO(2); break; \
        case 3: MACRO(3); break; \
        case 4: MACRO(4); break; \
        case 5: MACRO(5); break; \
        case 6: MACRO(6); break; \
        default: adf_set_error("eqv2 training: lmax %d not instantiated (1..6)", L_); return ADF_EINVAL; \
    }
#define EQT_LAUNCHED() ADF_HIP_CHECK(hipGetLastError())
#define EQT_SR_MAX 49     // adf_eqv2_create refuses S_r > 49
#define EQT_CHUNK 256     // edges per partial row of the attention weights' parameter gradients

static inline unsigned eqt_grid(long long n, int per = 256) {
    long long g = (n + per - 1) / per;
    if (g < 1) g = 1;
    if (g > 1048576) g = 1048576;
    return (unsigned)g;
}
static inline int eqt_block(int n) {
    int b = (n + 63) / 64 * 64;
    return b < 64 ? 64 : (b > 256 ? 256 : b);
}
static int32_t eqt_handle(const adf_eqv2* h, const char* who) {
    if (!h) { adf_set_error("%s: null handle", who); return ADF_EINVAL; }
    if (!h->consts_set) { adf_set_error("%s: set_constants first", who); return ADF_EINVAL; }
    return ADF_OK;
}

// order-major reduced index of (degree l, order mp) with |mp| <= min(l, M)
__device__ __forceinline__ int eqt_ridx(const eq_dims& d, int l, int mp) {
    const int am = mp < 0 ? -mp : mp;
    return d.rbase[am] + (mp < 0 ? d.L - am + 1 : 0) + (l - am);
}

__device__ __forceinline__ float eqt_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float eqt_dsilu(float x) {
    const float sg = eqt_sigmoid(x);
    return sg * (1.0f + x * (1.0f - sg));
}
// smooth leaky ReLU with slope 0.2 (activation.py:46-58): 0.6 x + 0.4 x (2 sigmoid(x) - 1)
__device__ __forceinline__ float eqt_slrelu(float x) { return 0.6f * x + 0.4f * x * (2.0f * eqt_sigmoid(x) - 1.0f); }
__device__ __forceinline__ float eqt_dslrelu(float x) {
    const float sg = eqt_sigmoid(x);
    return 0.6f + 0.4f * (2.0f * sg - 1.0f) + 0.8f * x * sg * (1.0f - sg);
}

// ------------------------------------------------------------------------------------------------ dense products
// C[r, j] (+)= sum_i A(r, i) B(j, i) + bias[j] with A(r, i) = A[r sar + i sai], B(j, i) = B[j sbj + i sbi]: one kernel for
// y = x W^T (sar = lda, sai = 1, sbj = ldw, sbi = 1), the data gradient dC W (sbj = 1, sbi = ldw) and the weight gradient
// dC^T A (sar = 1, sai = ldc, sbj = 1, sbi = lda; the sum over the rows of the batch).  64 x 64 tile per workgroup, 4 x 4
// per thread, the inner index in steps of 16 through LDS; a thread adds its products in index order.
__global__ __launch_bounds__(256) void eqt_gemm_kernel(const float* __restrict__ A, long long sar, long long sai,
                                                       const float* __restrict__ B, long long sbj, long long sbi,
                                                       const float* __restrict__ bias, float* __restrict__ Cm, long long ldc,
                                                       int acc, long long R, int J, long long I) {
    __shared__ float As[16][65], Bs[16][65];
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const long long r0 = (long long)blockIdx.x * 64;
    const int j0 = blockIdx.y * 64;
    float c[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) c[a][b] = 0.f;
    const bool a_inner_fast = sai == 1, b_inner_fast = sbi == 1;
    for (long long i0 = 0; i0 < I; i0 += 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + 256 * q;
            {
                const int rr = a_inner_fast ? idx >> 4 : idx & 63, ii = a_inner_fast ? idx & 15 : idx >> 6;
                const long long r = r0 + rr, i = i0 + ii;
                As[ii][rr] = (r < R && i < I) ? A[r * sar + i * sai] : 0.f;
            }
            {
                const int jj = b_inner_fast ? idx >> 4 : idx & 63, ii = b_inner_fast ? idx & 15 : idx >> 6;
                const long long i = i0 + ii;
                const int j = j0 + jj;
                Bs[ii][jj] = (j < J && i < I) ? B[j * sbj + i * sbi] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int ii = 0; ii < 16; ++ii) {
            float av[4], bv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) av[a] = As[ii][tr * 4 + a];
#pragma unroll
            for (int b = 0; b < 4; ++b) bv[b] = Bs[ii][tc * 4 + b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) c[a][b] += av[a] * bv[b];
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long long r = r0 + tr * 4 + a;
        if (r >= R) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + tc * 4 + b;
            if (j >= J) continue;
            float v = c[a][b] + (bias ? bias[j] : 0.f);
            float* o = Cm + r * ldc + j;
            *o = acc ? *o + v : v;
        }
    }
}

static int32_t eqt_gemm(const float* A, long long sar, long long sai, const float* B, long long sbj, long long sbi,
                        const float* bias, float* Cm, long long ldc, int acc, long long R, int J, long long I, hipStream_t s) {
    if (R <= 0 || J <= 0) return ADF_OK;
    const long long gx = (R + 63) / 64;
    if (gx > 2147483647LL) { adf_set_error("eqv2 training: too many rows"); return ADF_EINVAL; }
    hipLaunchKernelGGL(eqt_gemm_kernel, dim3((unsigned)gx, (unsigned)((J + 63) / 64)), dim3(256), 0, s, A, sar, sai, B, sbj, sbi,
                       bias, Cm, ldc, acc, R, J, I);
    EQT_LAUNCHED();
    return ADF_OK;
}

// db[j] += sum_m dC[m, j], rows in index order
__global__ void eqt_colsum_kernel(const float* __restrict__ dC, long long ldc, float* __restrict__ db, long long M, int N) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    float s = 0.f;
    for (long long m = 0; m < M; ++m) s += dC[m * ldc + j];
    db[j] += s;
}

extern "C" int32_t adf_op_eq_linear_fwd(const float* A, int32_t lda, const float* W, int32_t ldw, const float* bias, float* Cm,
                                        int32_t ldc, int32_t acc_C, int64_t M, int32_t N, int32_t K, void* stream) {
    if (!A || !W || !Cm || M < 0 || N <= 0 || K <= 0 || lda < K || ldw < K || ldc < N) { adf_set_error("eq_linear_fwd: bad argument"); return ADF_EINVAL; }
    return eqt_gemm(A, lda, 1, W, ldw, 1, bias, Cm, ldc, acc_C, M, N, K, (hipStream_t)stream);
}

extern "C" int32_t adf_op_eq_linear_bwd(const float* A, int32_t lda, const float* W, int32_t ldw, const float* dC, int32_t ldc,
                                        float* dA, int32_t ldda, int32_t acc_dA, float* dW, int32_t lddw, float* db, int64_t M,
                                        int32_t N, int32_t K, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!dC || M < 0 || N <= 0 || K <= 0 || ldc < N || (dA && (!W || ldw < K || ldda < K)) || (dW && (!A || lda < K || lddw < K))) {
        adf_set_error("eq_linear_bwd: bad argument");
        return ADF_EINVAL;
    }
    if (M == 0) return ADF_OK;
    if (dA) ADF_TRY(eqt_gemm(dC, ldc, 1, W, 1, ldw, nullptr, dA, ldda, acc_dA, M, K, N, s));
    if (dW) ADF_TRY(eqt_gemm(dC, 1, ldc, A, 1, lda, nullptr, dW, lddw, 1, N, K, M, s));
    if (db) {
        hipLaunchKernelGGL(eqt_colsum_kernel, dim3((N + 63) / 64), dim3(64), 0, s, dC, (long long)ldc, db, (long long)M, N);
        EQT_LAUNCHED();
    }
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ SiLU
__global__ void eqt_silu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        y[i] = x[i] * eqt_sigmoid(x[i]);
}
__global__ void eqt_silu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                    long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dx[i] = dy[i] * eqt_dsilu(x[i]);
}
extern "C" int32_t adf_op_eq_silu_fwd(const float* x, float* y, int64_t n, void* stream) {
    if (!x || !y || n < 0) { adf_set_error("eq_silu_fwd: bad argument"); return ADF_EINVAL; }
    if (n == 0) return ADF_OK;
    hipLaunchKernelGGL(eqt_silu_fwd_kernel, dim3(eqt_grid(n)), dim3(256), 0, (hipStream_t)stream, x, y, (long long)n);
    EQT_LAUNCHED();
    return ADF_OK;
}
extern "C" int32_t adf_op_eq_silu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream) {
    if (!x || !dy || !dx || n < 0) { adf_set_error("eq_silu_bwd: bad argument"); return ADF_EINVAL; }
    if (n == 0) return ADF_OK;
    hipLaunchKernelGGL(eqt_silu_bwd_kernel, dim3(eqt_grid(n)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, (long long)n);
    EQT_LAUNCHED();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ edge scalars
// [Gaussian basis | source embedding | target embedding] of every edge (equiformer_v2_denoising.py:207-213, 267;
// GaussianSmearing: exp(coeff (x - mu_k)^2), mu_k = k delta, coeff = -0.5 / (2 delta)^2, equiformer_v2_oc20.py:41-62)
__global__ void eqt_edge_scalars_kernel(const int32_t* __restrict__ Z, const int32_t* __restrict__ src,
                                        const int32_t* __restrict__ dst, const float* __restrict__ vec,
                                        const float* __restrict__ radii, const float* __restrict__ semb,
                                        const float* __restrict__ temb, int NB, int EC, int max_elem, float rc,
                                        float* __restrict__ out) {
    const long long e = blockIdx.x;
    const int zs = min(max(Z[src[e]], 0), max_elem - 1), zt = min(max(Z[dst[e]], 0), max_elem - 1);
    const float vx = vec[3 * e], vy = vec[3 * e + 1], vz = vec[3 * e + 2];
    const float dist = sqrtf(vx * vx + vy * vy + vz * vz);
    const float dd = dist - (radii ? radii[min(zs, 100)] + radii[min(zt, 100)] : 0.f);
    const float delta = rc / (float)(NB - 1);
    const float coeff = -0.5f / ((2.0f * delta) * (2.0f * delta));
    float* o = out + (size_t)e * (NB + 2 * EC);
    for (int k = threadIdx.x; k < NB + 2 * EC; k += blockDim.x) {
        float v;
        if (k < NB) {
            const float t = dd - delta * (float)k;
            v = expf(coeff * t * t);
        } else if (k < NB + EC) {
            v = semb[(size_t)zs * EC + (k - NB)];
        } else {
            v = temb[(size_t)zt * EC + (k - NB - EC)];
        }
        o[k] = v;
    }
}

extern "C" int32_t adf_op_eq_edge_scalars(adf_eqv2_t h, const int32_t* Z, const int32_t* src, const int32_t* dst,
                                          const float* vec, const float* semb, const float* temb, int64_t E, float* out,
                                          void* stream) {
    ADF_TRY(eqt_handle(h, "eq_edge_scalars"));
    if (!Z || !src || !dst || !vec || !semb || !temb || !out || E < 0) { adf_set_error("eq_edge_scalars: bad argument"); return ADF_EINVAL; }
    if (!h->s2ef && !h->weights_set) { adf_set_error("eq_edge_scalars: set_weights first (atom_radii)"); return ADF_EINVAL; }
    if (E == 0) return ADF_OK;
    hipLaunchKernelGGL(eqt_edge_scalars_kernel, dim3((unsigned)E), dim3(256), 0, (hipStream_t)stream, Z, src, dst, vec,
                       h->s2ef ? (const float*)nullptr : h->atom_radii, semb, temb, h->d.NB, h->d.EC, h->hp.max_num_elements,
                       h->hp.max_radius, out);
    EQT_LAUNCHED();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ rotate in
// One workgroup per edge, a thread per input channel of [x_src | x_tgt] (strided when 2C > 256).
template <int LT>
__global__ __launch_bounds__(256) void eqt_rotate_in_fwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ src,
                                                                const int32_t* __restrict__ dst, const float* __restrict__ wig,
                                                                const float* __restrict__ radial, eq_dims d,
                                                                float* __restrict__ out) {
    const long long e = blockIdx.x;
    const int C2 = 2 * d.C;
    const float* D = wig + (size_t)e * d.DR;
    for (int c = threadIdx.x; c < C2; c += blockDim.x) {
        const int node = c < d.C ? src[e] : dst[e];
        const float* xr = x + (size_t)node * d.S * d.C + (c < d.C ? c : c - d.C);
        const float* rr = radial + (size_t)e * d.RW * C2 + c;
        float* o = out + (size_t)e * d.Sr * C2 + c;
#pragma unroll
        for (int l = 0; l <= LT; ++l) {
            float v[2 * LT + 1];
#pragma unroll
            for (int j = 0; j < 2 * l + 1; ++j) v[j] = xr[(size_t)(l * l + j) * d.C];
            const int ml = l < d.M ? l : d.M;
            const float* Dl = D + d.d_off[l];
#pragma unroll
            for (int mp = -l; mp <= l; ++mp) {
                const int am = mp < 0 ? -mp : mp;
                if (am > ml) continue;
                const int ri = mp + ml;
                float a = 0.f;
#pragma unroll
                for (int j = 0; j < 2 * l + 1; ++j) a += Dl[ri * (2 * l + 1) + j] * v[j];
                o[(size_t)eqt_ridx(d, l, mp) * C2] = a * rr[(size_t)(d.rad_off[am] + (l - am)) * C2];
            }
        }
    }
}

// d radial: the rotated, unweighted coefficient is formed again; +m and -m share a weight and are added in that order
template <int LT>
__global__ __launch_bounds__(256) void eqt_rotate_in_drad_kernel(const float* __restrict__ x, const int32_t* __restrict__ src,
                                                                 const int32_t* __restrict__ dst, const float* __restrict__ wig,
                                                                 const float* __restrict__ dout, eq_dims d,
                                                                 float* __restrict__ dradial) {
    const long long e = blockIdx.x;
    const int C2 = 2 * d.C;
    const float* D = wig + (size_t)e * d.DR;
    for (int c = threadIdx.x; c < C2; c += blockDim.x) {
        const int node = c < d.C ? src[e] : dst[e];
        const float* xr = x + (size_t)node * d.S * d.C + (c < d.C ? c : c - d.C);
        const float* g = dout + (size_t)e * d.Sr * C2 + c;
        float* dr = dradial + (size_t)e * d.RW * C2 + c;
#pragma unroll
        for (int l = 0; l <= LT; ++l) {
            float v[2 * LT + 1];
#pragma unroll
            for (int j = 0; j < 2 * l + 1; ++j) v[j] = xr[(size_t)(l * l + j) * d.C];
            const int ml = l < d.M ? l : d.M;
            const float* Dl = D + d.d_off[l];
#pragma unroll
            for (int am = 0; am <= l; ++am) {
                if (am > ml) continue;
                float acc = 0.f;
#pragma unroll
                for (int sg = 0; sg < 2; ++sg) {
                    if (sg == 1 && am == 0) continue;
                    const int mp = sg ? -am : am, ri = mp + ml;
                    float a = 0.f;
#pragma unroll
                    for (int j = 0; j < 2 * l + 1; ++j) a += Dl[ri * (2 * l + 1) + j] * v[j];
                    acc += g[(size_t)eqt_ridx(d, l, mp) * C2] * a;
                }
                dr[(size_t)(d.rad_off[am] + (l - am)) * C2] = acc;
            }
        }
    }
}

// d x: one workgroup per atom, a thread per channel; the atom's incoming edges in list order (target half of the channels),
// then its outgoing edges in the order of the source-sorted permutation (source half)
template <int LT>
__global__ __launch_bounds__(256) void eqt_rotate_in_dx_kernel(const int32_t* __restrict__ eptr, const int32_t* __restrict__ sptr,
                                                               const int32_t* __restrict__ sperm, const float* __restrict__ wig,
                                                               const float* __restrict__ radial, const float* __restrict__ dout,
                                                               eq_dims d, float* __restrict__ dx) {
    const int n = blockIdx.x;
    const int C2 = 2 * d.C;
    constexpr int SS = (LT + 1) * (LT + 1);
    for (int c = threadIdx.x; c < d.C; c += blockDim.x) {
        float acc[SS];
#pragma unroll
        for (int s = 0; s < SS; ++s) acc[s] = 0.f;
        for (int pass = 0; pass < 2; ++pass) {
            const int k0 = pass == 0 ? eptr[n] : sptr[n], k1 = pass == 0 ? eptr[n + 1] : sptr[n + 1];
            const int cc = pass == 0 ? d.C + c : c;
            for (int k = k0; k < k1; ++k) {
                const long long e = pass == 0 ? k : sperm[k];
                const float* D = wig + (size_t)e * d.DR;
                const float* g = dout + (size_t)e * d.Sr * C2 + cc;
                const float* rr = radial + (size_t)e * d.RW * C2 + cc;
#pragma unroll
                for (int l = 0; l <= LT; ++l) {
                    const int ml = l < d.M ? l : d.M;
                    const float* Dl = D + d.d_off[l];
#pragma unroll
                    for (int mp = -l; mp <= l; ++mp) {
                        const int am = mp < 0 ? -mp : mp;
                        if (am > ml) continue;
                        const int ri = mp + ml;
                        const float gv = g[(size_t)eqt_ridx(d, l, mp) * C2] * rr[(size_t)(d.rad_off[am] + (l - am)) * C2];
#pragma unroll
                        for (int j = 0; j < 2 * l + 1; ++j) acc[l * l + j] += Dl[ri * (2 * l + 1) + j] * gv;
                    }
                }
            }
        }
        float* o = dx + (size_t)n * d.S * d.C + c;
#pragma unroll
        for (int s = 0; s < SS; ++s) o[(size_t)s * d.C] = acc[s];
    }
}

extern "C" int32_t adf_op_eq_rotate_in_fwd(adf_eqv2_t h, const float* x, const int32_t* src, const int32_t* dst,
                                           const float* wig, const float* radial, int64_t E, float* out, void* stream) {
    ADF_TRY(eqt_handle(h, "eq_rotate_in_fwd"));
    if (!x || !src || !dst || !wig || !radial || !out || E < 0) { adf_set_error("eq_rotate_in_fwd: bad argument"); return ADF_EINVAL; }
    if (E == 0) return ADF_OK;
    const int bd = eqt_block(2 * h->d.C);
#define EQT_RI(LT_) hipLaunchKernelGGL((eqt_rotate_in_fwd_kernel<LT_>), dim3((unsigned)E), dim3(bd), 0, (hipStream_t)stream, x, src, \
                                       dst, wig, radial, h->d, out)
    EQT_FOR_L(h->d.L, EQT_RI)
#undef EQT_RI
    EQT_LAUNCHED();
    return ADF_OK;
}

extern "C" int32_t adf_op_eq_rotate_in_bwd(adf_eqv2_t h, const float* x, const int32_t* eptr, const int32_t* src,
                                           const int32_t* dst, const float* wig, const float* radial, const float* dout,
                                           const int32_t* sptr, const int32_t* sperm, int32_t N, int64_t E, float* dradial,
                                           float* dx, void* stream) {
    ADF_TRY(eqt_handle(h, "eq_rotate_in_bwd"));
    if (!x || !eptr || !src || !dst || !wig || !radial || !dout || !sptr || !sperm || N <= 0 || E < 0 || !dradial || !dx) {
        adf_set_error("eq_rotate_in_bwd: bad argument");
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const int bd = eqt_block(2 * h->d.C), bn = eqt_block(h->d.C);
#define EQT_RB(LT_)                                                                                                          \
    if (E > 0) hipLaunchKernelGGL((eqt_rotate_in_drad_kernel<LT_>), dim3((unsigned)E), dim3(bd), 0, s, x, src, dst, wig, dout, h->d, \
                                  dradial);                                                                                  \
    hipLaunchKernelGGL((eqt_rotate_in_dx_kernel<LT_>), dim3((unsigned)N), dim3(bn), 0, s, eptr, sptr, sperm, wig, radial, dout, \
                       h->d, dx)
    EQT_FOR_L(h->d.L, EQT_RB)
#undef EQT_RB
    EQT_LAUNCHED();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ separable S2 activation
// One wave per 64 (edge, channel) pairs; a pair's S_r coefficients live in a column of LDS (lane-indexed: no bank conflict,
// run-time indexing without scratch memory).  Grid point by grid point: t = to_red[g] . y, silu(t), out += from_red[g] silu(t).
__global__ __launch_bounds__(64) void eqt_s2act_fwd_kernel(const float* __restrict__ y, const float* __restrict__ gate, int ldg,
                                                           const float* __restrict__ to_red, const float* __restrict__ from_red,
                                                           int Sr, int G, int W, long long total, float* __restrict__ out) {
    __shared__ float sy[EQT_SR_MAX * 64], sa[EQT_SR_MAX * 64];
    const int lane = threadIdx.x;
    const long long idx = (long long)blockIdx.x * 64 + lane;
    if (idx >= total) return;   // no barrier below: the wave's lanes only read their own columns
    const long long e = idx / W;
    const int c = (int)(idx - e * W);
    const float* yr = y + (size_t)e * Sr * W + c;
    for (int r = 0; r < Sr; ++r) { sy[r * 64 + lane] = yr[(size_t)r * W]; sa[r * 64 + lane] = 0.f; }
    for (int g = 0; g < G; ++g) {
        const float* tr = to_red + (size_t)g * Sr;
        const float* fr = from_red + (size_t)g * Sr;
        float t = 0.f;
        for (int r = 0; r < Sr; ++r) t += tr[r] * sy[r * 64 + lane];
        const float sv = t * eqt_sigmoid(t);
        for (int r = 1; r < Sr; ++r) sa[r * 64 + lane] += fr[r] * sv;
    }
    float* o = out + (size_t)e * Sr * W + c;
    const float gt = gate[(size_t)e * ldg + c];
    o[0] = gt * eqt_sigmoid(gt);
    for (int r = 1; r < Sr; ++r) o[(size_t)r * W] = sa[r * 64 + lane];
}

__global__ __launch_bounds__(64) void eqt_s2act_bwd_kernel(const float* __restrict__ y, const float* __restrict__ gate, int ldg,
                                                           const float* __restrict__ dout, const float* __restrict__ to_red,
                                                           const float* __restrict__ from_red, int Sr, int G, int W,
                                                           long long total, float* __restrict__ dy, float* __restrict__ dgate,
                                                           int lddg) {
    __shared__ float sy[EQT_SR_MAX * 64], sd[EQT_SR_MAX * 64], sa[EQT_SR_MAX * 64];
    const int lane = threadIdx.x;
    const long long idx = (long long)blockIdx.x * 64 + lane;
    if (idx >= total) return;
    const long long e = idx / W;
    const int c = (int)(idx - e * W);
    const float* yr = y + (size_t)e * Sr * W + c;
    const float* dr = dout + (size_t)e * Sr * W + c;
    for (int r = 0; r < Sr; ++r) {
        sy[r * 64 + lane] = yr[(size_t)r * W];
        sd[r * 64 + lane] = dr[(size_t)r * W];
        sa[r * 64 + lane] = 0.f;
    }
    for (int g = 0; g < G; ++g) {
        const float* tr = to_red + (size_t)g * Sr;
        const float* fr = from_red + (size_t)g * Sr;
        float t = 0.f, u = 0.f;
        for (int r = 0; r < Sr; ++r) t += tr[r] * sy[r * 64 + lane];
        for (int r = 1; r < Sr; ++r) u += fr[r] * sd[r * 64 + lane];
        u *= eqt_dsilu(t);
        for (int r = 0; r < Sr; ++r) sa[r * 64 + lane] += tr[r] * u;
    }
    float* o = dy + (size_t)e * Sr * W + c;
    for (int r = 0; r < Sr; ++r) o[(size_t)r * W] = sa[r * 64 + lane];
    dgate[(size_t)e * lddg + c] = sd[lane] * eqt_dsilu(gate[(size_t)e * ldg + c]);
}

extern "C" int32_t adf_op_eq_s2act_fwd(adf_eqv2_t h, const float* y, const float* gate, int32_t ldg, int32_t W, int64_t E,
                                       float* out, void* stream) {
    ADF_TRY(eqt_handle(h, "eq_s2act_fwd"));
    if (!y || !gate || !out || W < 1 || ldg < W || E < 0 || h->d.Sr > EQT_SR_MAX) { adf_set_error("eq_s2act_fwd: bad argument"); return ADF_EINVAL; }
    const long long total = (long long)E * W;
    if (total == 0) return ADF_OK;
    if ((total + 63) / 64 > 2147483647LL) { adf_set_error("eq_s2act_fwd: too many rows"); return ADF_EINVAL; }
    hipLaunchKernelGGL(eqt_s2act_fwd_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, (hipStream_t)stream, y, gate, ldg,
                       h->to_red, h->from_red, h->d.Sr, h->d.G, W, total, out);
    EQT_LAUNCHED();
    return ADF_OK;
}

extern "C" int32_t adf_op_eq_s2act_bwd(adf_eqv2_t h, const float* y, const float* gate, int32_t ldg, const float* dout, int32_t W,
                                       int64_t E, float* dy, float* dgate, int32_t lddg, void* stream) {
    ADF_TRY(eqt_handle(h, "eq_s2act_bwd"));
    if (!y || !gate || !dout || !dy || !dgate || W < 1 || ldg < W || lddg < W || E < 0 || h->d.Sr > EQT_SR_MAX) {
        adf_set_error("eq_s2act_bwd: bad argument");
        return ADF_EINVAL;
    }
    const long long total = (long long)E * W;
    if (total == 0) return ADF_OK;
    if ((total + 63) / 64 > 2147483647LL) { adf_set_error("eq_s2act_bwd: too many rows"); return ADF_EINVAL; }
    hipLaunchKernelGGL(eqt_s2act_bwd_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, (hipStream_t)stream, y, gate, ldg,
                       dout, h->to_red, h->from_red, h->d.Sr, h->d.G, W, total, dy, dgate, lddg);
    EQT_LAUNCHED();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ attention weights
// LayerNorm statistics of one (edge, head): mean and 1 / sqrt(biased variance + 1e-5) over the A channels
__device__ __forceinline__ void eqt_ln_stats(const float* __restrict__ xr, int A, float& mean, float& rstd) {
    float s = 0.f;
    for (int k = 0; k < A; ++k) s += xr[k];
    mean = s / (float)A;
    float v = 0.f;
    for (int k = 0; k < A; ++k) { const float t = xr[k] - mean; v += t * t; }
    rstd = 1.0f / sqrtf(v / (float)A + 1e-5f);
}

// logit[e, h] = sum_k slrelu(LN(a_in[e, h, :]))_k alpha_dot[h, k]; a thread per (edge, head)
__global__ void eqt_alpha_logit_kernel(const float* __restrict__ a_in, int lda, const float* __restrict__ w,
                                       const float* __restrict__ b, const float* __restrict__ adot, int NH, int A, long long E,
                                       float* __restrict__ logit) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= E * NH) return;
    const long long e = t / NH;
    const int hd = (int)(t - e * NH);
    const float* xr = a_in + (size_t)e * lda + hd * A;
    float mean, rstd;
    eqt_ln_stats(xr, A, mean, rstd);
    float s = 0.f;
    for (int k = 0; k < A; ++k) s += eqt_slrelu((xr[k] - mean) * rstd * w[k] + b[k]) * adot[hd * A + k];
    logit[t] = s;
}

// softmax over a target's edges, in place on the logits; a thread per (target, head), the edges in list order
__global__ void eqt_alpha_softmax_kernel(float* __restrict__ soft, const int32_t* __restrict__ eptr, const float* __restrict__ mask,
                                         int N, int NH, float* __restrict__ alpha) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * NH) return;
    const int n = t / NH, hd = t - n * NH;
    const int e0 = eptr[n], e1 = eptr[n + 1];
    if (e1 <= e0) return;
    float mx = -INFINITY;
    for (int e = e0; e < e1; ++e) mx = fmaxf(mx, soft[(size_t)e * NH + hd]);
    float den = 0.f;
    for (int e = e0; e < e1; ++e) den += expf(soft[(size_t)e * NH + hd] - mx);
    const float inv = 1.0f / (den + 1e-16f);
    for (int e = e0; e < e1; ++e) {
        const float p = expf(soft[(size_t)e * NH + hd] - mx) * inv;
        soft[(size_t)e * NH + hd] = p;
        alpha[(size_t)e * NH + hd] = mask ? p * mask[(size_t)e * NH + hd] : p;
    }
}

// d logit[e, h] = p (da - sum_j p_j da_j) with da = dalpha * mask (the 1e-16 of the denominator, at most 1e-16 of a
// denominator >= 1, is below f32 resolution and left out of the derivative)
__global__ void eqt_alpha_dlogit_kernel(const float* __restrict__ soft, const float* __restrict__ dalpha,
                                        const float* __restrict__ mask, const int32_t* __restrict__ eptr, int N, int NH,
                                        float* __restrict__ dl) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * NH) return;
    const int n = t / NH, hd = t - n * NH;
    const int e0 = eptr[n], e1 = eptr[n + 1];
    float dot = 0.f;
    for (int e = e0; e < e1; ++e) {
        const size_t i = (size_t)e * NH + hd;
        dot += soft[i] * dalpha[i] * (mask ? mask[i] : 1.0f);
    }
    for (int e = e0; e < e1; ++e) {
        const size_t i = (size_t)e * NH + hd;
        dl[i] = soft[i] * (dalpha[i] * (mask ? mask[i] : 1.0f) - dot);
    }
}

// d a_in through the dot, the activation and the LayerNorm; keeps (mean, rstd) of every (edge, head) for the parameter pass
__global__ void eqt_alpha_dx_kernel(const float* __restrict__ a_in, int lda, const float* __restrict__ w,
                                    const float* __restrict__ b, const float* __restrict__ adot, const float* __restrict__ dl,
                                    int NH, int A, long long E, float* __restrict__ da_in, int ldda, float* __restrict__ stats) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= E * NH) return;
    const long long e = t / NH;
    const int hd = (int)(t - e * NH);
    const float* xr = a_in + (size_t)e * lda + hd * A;
    float mean, rstd;
    eqt_ln_stats(xr, A, mean, rstd);
    stats[2 * t] = mean;
    stats[2 * t + 1] = rstd;
    const float g = dl[t];
    float m1 = 0.f, m2 = 0.f;
    for (int k = 0; k < A; ++k) {
        const float xh = (xr[k] - mean) * rstd;
        const float dxh = g * adot[hd * A + k] * eqt_dslrelu(xh * w[k] + b[k]) * w[k];
        m1 += dxh;
        m2 += dxh * xh;
    }
    m1 /= (float)A;
    m2 /= (float)A;
    float* o = da_in + (size_t)e * ldda + hd * A;
    for (int k = 0; k < A; ++k) {
        const float xh = (xr[k] - mean) * rstd;
        const float dxh = g * adot[hd * A + k] * eqt_dslrelu(xh * w[k] + b[k]) * w[k];
        o[k] = rstd * (dxh - m1 - xh * m2);
    }
}

// parameter gradients, pass 1: per chunk of EQT_CHUNK edges and column (head, k) the sums over the chunk's edges in list
// order -> part [chunks][3][NH A] = (d alpha_dot, d ln_w, d ln_b contributions)
__global__ void eqt_alpha_wpart_kernel(const float* __restrict__ a_in, int lda, const float* __restrict__ w,
                                       const float* __restrict__ b, const float* __restrict__ adot, const float* __restrict__ dl,
                                       const float* __restrict__ stats, int NH, int A, long long E, float* __restrict__ part) {
    const int chunk = blockIdx.x, HA = NH * A;
    const long long e0 = (long long)chunk * EQT_CHUNK, e1 = (e0 + EQT_CHUNK < E) ? e0 + EQT_CHUNK : E;
    for (int j = threadIdx.x; j < HA; j += blockDim.x) {
        const int hd = j / A, k = j - hd * A;
        float sd = 0.f, sw = 0.f, sb = 0.f;
        for (long long e = e0; e < e1; ++e) {
            const size_t t = (size_t)e * NH + hd;
            const float xh = (a_in[(size_t)e * lda + j] - stats[2 * t]) * stats[2 * t + 1];
            const float z = xh * w[k] + b[k];
            const float g = dl[t];
            sd += g * eqt_slrelu(z);
            const float dz = g * adot[j] * eqt_dslrelu(z);
            sw += dz * xh;
            sb += dz;
        }
        float* p = part + (size_t)chunk * 3 * HA;
        p[j] = sd; p[HA + j] = sw; p[2 * HA + j] = sb;
    }
}

// pass 2 (one workgroup): the chunks in index order, then for the LayerNorm parameters the heads in index order
__global__ void eqt_alpha_wsum_kernel(const float* __restrict__ part, int chunks, int NH, int A, float* __restrict__ tmp,
                                      float* __restrict__ d_adot, float* __restrict__ d_w, float* __restrict__ d_b) {
    const int HA = NH * A;
    for (int j = threadIdx.x; j < HA; j += blockDim.x) {
        float sd = 0.f, sw = 0.f, sb = 0.f;
        for (int ch = 0; ch < chunks; ++ch) {
            const float* p = part + (size_t)ch * 3 * HA;
            sd += p[j]; sw += p[HA + j]; sb += p[2 * HA + j];
        }
        d_adot[j] += sd;
        tmp[j] = sw;
        tmp[HA + j] = sb;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < A; k += blockDim.x) {
        float sw = 0.f, sb = 0.f;
        for (int hd = 0; hd < NH; ++hd) { sw += tmp[hd * A + k]; sb += tmp[HA + hd * A + k]; }
        d_w[k] += sw;
        d_b[k] += sb;
    }
}

extern "C" int32_t adf_op_eq_alpha_fwd(adf_eqv2_t h, const float* a_in, int32_t lda, const float* ln_w, const float* ln_b,
                                       const float* alpha_dot, const int32_t* eptr, const float* mask, int32_t N, int64_t E,
                                       float* soft, float* alpha, void* stream) {
    ADF_TRY(eqt_handle(h, "eq_alpha_fwd"));
    const int NH = h->d.NH, A = h->d.A;
    if (!a_in || !ln_w || !ln_b || !alpha_dot || !eptr || !soft || !alpha || N <= 0 || E < 0 || lda < NH * A || soft == alpha) {
        adf_set_error("eq_alpha_fwd: bad argument");
        return ADF_EINVAL;
    }
    if (E == 0) return ADF_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(eqt_alpha_logit_kernel, dim3(eqt_grid((long long)E * NH)), dim3(256), 0, s, a_in, lda, ln_w, ln_b,
                       alpha_dot, NH, A, (long long)E, soft);
    hipLaunchKernelGGL(eqt_alpha_softmax_kernel, dim3(eqt_grid((long long)N * NH, 64)), dim3(64), 0, s, soft, eptr, mask, N, NH,
                       alpha);
    EQT_LAUNCHED();
    return ADF_OK;
}

extern "C" int32_t adf_op_eq_alpha_bwd(adf_eqv2_t h, const float* a_in, int32_t lda, const float* ln_w, const float* ln_b,
                                       const float* alpha_dot, const int32_t* eptr, const float* mask, const float* soft,
                                       const float* dalpha, int32_t N, int64_t E, float* da_in, int32_t ldda, float* d_ln_w,
                                       float* d_ln_b, float* d_alpha_dot, float* scratch, int64_t scratch_floats, void* stream) {
    ADF_TRY(eqt_handle(h, "eq_alpha_bwd"));
    const int NH = h->d.NH, A = h->d.A, HA = NH * A;
    const bool params = d_ln_w || d_ln_b || d_alpha_dot;   // all three or none: none skips the parameter pass
    if (!a_in || !ln_w || !ln_b || !alpha_dot || !eptr || !soft || !dalpha || !da_in || (params && (!d_ln_w || !d_ln_b || !d_alpha_dot)) ||
        !scratch || N <= 0 || E < 0 || lda < HA || ldda < HA) {
        adf_set_error("eq_alpha_bwd: bad argument");
        return ADF_EINVAL;
    }
    if (E == 0) return ADF_OK;
    const long long chunks = (E + EQT_CHUNK - 1) / EQT_CHUNK;
    const long long need = 3 * (long long)E * NH + (3 * chunks + 2) * HA;
    if (scratch_floats < need) { adf_set_error("eq_alpha_bwd: scratch of %lld floats, %lld needed", (long long)scratch_floats, need); return ADF_EINVAL; }
    float* dl = scratch;                           // [E, NH]
    float* stats = dl + (size_t)E * NH;            // [E, NH, 2]
    float* part = stats + 2 * (size_t)E * NH;      // [chunks, 3, HA]
    float* tmp = part + (size_t)chunks * 3 * HA;   // [2, HA]
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(eqt_alpha_dlogit_kernel, dim3(eqt_grid((long long)N * NH, 64)), dim3(64), 0, s, soft, dalpha, mask, eptr, N,
                       NH, dl);
    hipLaunchKernelGGL(eqt_alpha_dx_kernel, dim3(eqt_grid((long long)E * NH)), dim3(256), 0, s, a_in, lda, ln_w, ln_b, alpha_dot,
                       dl, NH, A, (long long)E, da_in, ldda, stats);
    if (params) {
        hipLaunchKernelGGL(eqt_alpha_wpart_kernel, dim3((unsigned)chunks), dim3(eqt_block(HA)), 0, s, a_in, lda, ln_w, ln_b,
                           alpha_dot, dl, stats, NH, A, (long long)E, part);
        hipLaunchKernelGGL(eqt_alpha_wsum_kernel, dim3(1), dim3(256), 0, s, part, (int)chunks, NH, A, tmp, d_alpha_dot, d_ln_w,
                           d_ln_b);
    }
    EQT_LAUNCHED();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ rotate out + aggregation
// One workgroup per target, a thread per output channel (head, v); the target's edges in list order.
template <int LT>
__global__ __launch_bounds__(256) void eqt_rotate_out_fwd_kernel(const float* __restrict__ z, const float* __restrict__ alpha,
                                                                 int NH, int V, const int32_t* __restrict__ eptr,
                                                                 const float* __restrict__ wig, int only_l, eq_dims d,
                                                                 float* __restrict__ agg) {
    const int n = blockIdx.x, HV = NH * V;
    constexpr int SS = (LT + 1) * (LT + 1);
    for (int c = threadIdx.x; c < HV; c += blockDim.x) {
        const int hd = c / V;
        float acc[SS];
#pragma unroll
        for (int s = 0; s < SS; ++s) acc[s] = 0.f;
        for (long long e = eptr[n]; e < eptr[n + 1]; ++e) {
            const float* D = wig + (size_t)e * d.DR;
            const float* zr = z + (size_t)e * d.Sr * HV + c;
            const float a = alpha[(size_t)e * NH + hd];
#pragma unroll
            for (int l = 0; l <= LT; ++l) {
                if (only_l >= 0 && l != only_l) continue;
                const int ml = l < d.M ? l : d.M;
                const float* Dl = D + d.d_off[l];
#pragma unroll
                for (int mp = -l; mp <= l; ++mp) {
                    const int am = mp < 0 ? -mp : mp;
                    if (am > ml) continue;
                    const int ri = mp + ml;
                    const float zv = zr[(size_t)eqt_ridx(d, l, mp) * HV] * a * d.resc[l];
#pragma unroll
                    for (int j = 0; j < 2 * l + 1; ++j) acc[l * l + j] += Dl[ri * (2 * l + 1) + j] * zv;
                }
            }
        }
        float* o = agg + (size_t)n * d.S * HV + c;
#pragma unroll
        for (int s = 0; s < SS; ++s) o[(size_t)s * HV] = acc[s];
    }
}

// One workgroup per edge: d z per channel, and d alpha[e, head] = the head's V channels summed in index order (LDS)
template <int LT>
__global__ __launch_bounds__(256) void eqt_rotate_out_bwd_kernel(const float* __restrict__ z, const float* __restrict__ alpha,
                                                                 int NH, int V, const int32_t* __restrict__ dst,
                                                                 const float* __restrict__ wig, const float* __restrict__ dagg,
                                                                 int only_l, eq_dims d, float* __restrict__ dz,
                                                                 float* __restrict__ dalpha) {
    __shared__ float part[1024];   // NH V <= 1024 (adf_eqv2_create)
    const long long e = blockIdx.x;
    const int HV = NH * V;
    const int n = dst[e];
    const float* D = wig + (size_t)e * d.DR;
    for (int c = threadIdx.x; c < HV; c += blockDim.x) {
        const int hd = c / V;
        const float a = alpha[(size_t)e * NH + hd];
        const float* g = dagg + (size_t)n * d.S * HV + c;
        const float* zr = z + (size_t)e * d.Sr * HV + c;
        float* o = dz + (size_t)e * d.Sr * HV + c;
        float pa = 0.f;
#pragma unroll
        for (int l = 0; l <= LT; ++l) {
            const int ml = l < d.M ? l : d.M;
            const float* Dl = D + d.d_off[l];
            const bool live = only_l < 0 || l == only_l;
#pragma unroll
            for (int mp = -l; mp <= l; ++mp) {
                const int am = mp < 0 ? -mp : mp;
                if (am > ml) continue;
                const int ri = mp + ml, r = eqt_ridx(d, l, mp);
                float t = 0.f;
                if (live) {
#pragma unroll
                    for (int j = 0; j < 2 * l + 1; ++j) t += Dl[ri * (2 * l + 1) + j] * g[(size_t)(l * l + j) * HV];
                    t *= d.resc[l];
                }
                o[(size_t)r * HV] = a * t;
                pa += zr[(size_t)r * HV] * t;
            }
        }
        part[c] = pa;
    }
    __syncthreads();
    for (int hd = threadIdx.x; hd < NH; hd += blockDim.x) {
        float s = 0.f;
        for (int v = 0; v < V; ++v) s += part[hd * V + v];
        dalpha[(size_t)e * NH + hd] = s;
    }
}

extern "C" int32_t adf_op_eq_rotate_out_fwd(adf_eqv2_t h, const float* z, const float* alpha, int32_t NH, int32_t V,
                                            const int32_t* eptr, const float* wig, int32_t only_l, int32_t N, float* agg,
                                            void* stream) {
    ADF_TRY(eqt_handle(h, "eq_rotate_out_fwd"));
    if (!z || !alpha || !eptr || !wig || !agg || NH < 1 || V < 1 || N <= 0 || only_l > h->d.L) { adf_set_error("eq_rotate_out_fwd: bad argument"); return ADF_EINVAL; }
    const int bd = eqt_block(NH * V);
#define EQT_RO(LT_) hipLaunchKernelGGL((eqt_rotate_out_fwd_kernel<LT_>), dim3((unsigned)N), dim3(bd), 0, (hipStream_t)stream, z, alpha, \
                                       NH, V, eptr, wig, only_l, h->d, agg)
    EQT_FOR_L(h->d.L, EQT_RO)
#undef EQT_RO
    EQT_LAUNCHED();
    return ADF_OK;
}

extern "C" int32_t adf_op_eq_rotate_out_bwd(adf_eqv2_t h, const float* z, const float* alpha, int32_t NH, int32_t V,
                                            const int32_t* dst, const float* wig, const float* dagg, int32_t only_l, int64_t E,
                                            float* dz, float* dalpha, void* stream) {
    ADF_TRY(eqt_handle(h, "eq_rotate_out_bwd"));
    if (!z || !alpha || !dst || !wig || !dagg || !dz || !dalpha || NH < 1 || V < 1 || (long long)NH * V > 1024 || E < 0 ||
        only_l > h->d.L) {
        adf_set_error("eq_rotate_out_bwd: bad argument");
        return ADF_EINVAL;
    }
    if (E == 0) return ADF_OK;
    const int bd = eqt_block(NH * V);
#define EQT_ROB(LT_) hipLaunchKernelGGL((eqt_rotate_out_bwd_kernel<LT_>), dim3((unsigned)E), dim3(bd), 0, (hipStream_t)stream, z, alpha, \
                                        NH, V, dst, wig, dagg, only_l, h->d, dz, dalpha)
    EQT_FOR_L(h->d.L, EQT_ROB)
#undef EQT_ROB
    EQT_LAUNCHED();
    return ADF_OK;
}
