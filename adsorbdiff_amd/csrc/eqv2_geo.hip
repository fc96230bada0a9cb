// Geometric gradient of the EquiformerV2 training graph (csrc/eqv2_geo.h states the contracts and the orders):
// the terms the backward of rotate-in, rotate-out and the live radial layer owes to the Wigner rows and the distances, the
// step from (dwig, ddist) to the edge vectors, and the step from the edge vectors to the atoms.
//
// Plain kernels, one wave per edge.  Exact f32; every output element is written by one thread in one written order, and
// no kernel synchronises through memory: two calls on the same input give the same bits.
#include "eqv2.h"
#include "eqv2_gauss.h"
#include "eqv2_geo.h"

#define EQX_LAUNCHED() ADF_HIP_CHECK(hipGetLastError())
#define EQX_ROWS 49      // adf_eqv2_create refuses S_r > 49; S = (lmax + 1)^2 <= 49
#define EQX_LD 65        // row stride of a staged 64-channel panel: rows r and r' of one column lie in different LDS banks
#define EQX_Q 8          // Wigner elements per lane: DR <= sum_l (2l+1)^2 = 455 <= 8 * 64 for lmax <= 6
#define EQX_NJ 455       // floats of one generator table, lmax = 6

static int32_t eqx_handle(const adf_eqv2* h, const char* who) {
    if (!h) { adf_set_error("%s: null handle", who); return ADF_EINVAL; }
    if (!h->consts_set || !h->kgen) { adf_set_error("%s: set_constants first", who); return ADF_EINVAL; }
    if (h->d.DR > 64 * EQX_Q || h->d.Sr > EQX_ROWS || h->d.S > EQX_ROWS || h->d.j_off[h->d.L + 1] > EQX_NJ) {
        adf_set_error("%s: lmax / mmax too large", who);
        return ADF_EINVAL;
    }
    return ADF_OK;
}

// Element t of an edge's Wigner rows -> its degree l, the reduced (order-major) row r(l, m_i) and the full row l^2 + j
__device__ __forceinline__ void eqx_decode(const eq_dims& d, int t, int& l, int& r, int& s) {
    l = 0;
    while (l < d.L && t >= d.d_off[l + 1]) ++l;
    const int loc = t - d.d_off[l], n = 2 * l + 1, ml = l < d.M ? l : d.M;
    const int ri = loc / n, j = loc - ri * n, mp = ri - ml, am = mp < 0 ? -mp : mp;
    r = d.rbase[am] + (mp < 0 ? d.L - am + 1 : 0) + (l - am);
    s = l * l + j;
}

// acc[q] += sum over the nc staged channels, in index order, of As[r_q][c] Bs[s_q][c]
__device__ __forceinline__ void eqx_panel_dot(const float* __restrict__ As, const float* __restrict__ Bs, const int (&ar)[EQX_Q],
                                              const int (&bs)[EQX_Q], const bool (&on)[EQX_Q], int nc, float (&acc)[EQX_Q]) {
#pragma unroll
    for (int q = 0; q < EQX_Q; ++q) {
        if (!on[q]) continue;
        const float* a = As + ar[q] * EQX_LD;
        const float* b = Bs + bs[q] * EQX_LD;
        float v = acc[q];
        for (int c = 0; c < nc; ++c) v += a[c] * b[c];
        acc[q] = v;
    }
}

// ------------------------------------------------------------------------------------------------ rotate in
// One wave per edge; lane + 64 q = element of the edge's Wigner rows.  Per 64 channels of [x[src] | x[dst]]: the S rows of
// the two nodes and the S_r radial-weighted rows of dout go to LDS once (lane = channel, coalesced), then every lane walks
// its elements' two rows.
__global__ __launch_bounds__(64) void eqx_rotate_in_wig_kernel(const float* __restrict__ x, const int32_t* __restrict__ src,
                                                              const int32_t* __restrict__ dst, const float* __restrict__ radial,
                                                              const float* __restrict__ dout, eq_dims d, float* __restrict__ dwig) {
    __shared__ float As[EQX_ROWS * EQX_LD], Bs[EQX_ROWS * EQX_LD];
    const long long e = blockIdx.x;
    const int lane = threadIdx.x, C2 = 2 * d.C;
    int ar[EQX_Q], bs[EQX_Q];
    bool on[EQX_Q];
    float acc[EQX_Q];
#pragma unroll
    for (int q = 0; q < EQX_Q; ++q) {
        const int t = lane + 64 * q;
        int l;
        on[q] = t < d.DR;
        ar[q] = bs[q] = 0;
        acc[q] = 0.f;
        if (on[q]) eqx_decode(d, t, l, ar[q], bs[q]);
    }
    const int ns = src[e], nt = dst[e];
    for (int c0 = 0; c0 < C2; c0 += 64) {
        const int c = c0 + lane;
        const bool live = c < C2;
        const float* xr = x + (size_t)(c < d.C ? ns : nt) * d.S * d.C + (c < d.C ? c : c - d.C);
        const float* g = dout + (size_t)e * d.Sr * C2 + c;
        const float* rr = radial + (size_t)e * d.RW * C2 + c;
        for (int s = 0; s < d.S; ++s) Bs[s * EQX_LD + lane] = live ? xr[(size_t)s * d.C] : 0.f;
        for (int r = 0; r < d.Sr; ++r) {
            const int am = d.r_m[r], l = d.r_l[r];
            As[r * EQX_LD + lane] = live ? g[(size_t)r * C2] * rr[(size_t)(d.rad_off[am] + (l - am)) * C2] : 0.f;
        }
        __syncthreads();
        eqx_panel_dot(As, Bs, ar, bs, on, min(64, C2 - c0), acc);
        __syncthreads();
    }
    float* o = dwig + (size_t)e * d.DR;
#pragma unroll
    for (int q = 0; q < EQX_Q; ++q)
        if (on[q]) o[lane + 64 * q] = o[lane + 64 * q] + acc[q];
}

// ------------------------------------------------------------------------------------------------ rotate out
// The same contraction for agg = sum D^T (rescale alpha z): the staged rows are rescale_l alpha[e, head] z[e, r] and
// dagg[dst[e], s]; with only_l >= 0 the elements of the other degrees are left alone.
__global__ __launch_bounds__(64) void eqx_rotate_out_wig_kernel(const float* __restrict__ z, const float* __restrict__ alpha, int NH,
                                                               int V, const int32_t* __restrict__ dst,
                                                               const float* __restrict__ dagg, int only_l, eq_dims d,
                                                               float* __restrict__ dwig) {
    __shared__ float As[EQX_ROWS * EQX_LD], Bs[EQX_ROWS * EQX_LD];
    const long long e = blockIdx.x;
    const int lane = threadIdx.x, HV = NH * V;
    int ar[EQX_Q], bs[EQX_Q];
    bool on[EQX_Q];
    float acc[EQX_Q];
#pragma unroll
    for (int q = 0; q < EQX_Q; ++q) {
        const int t = lane + 64 * q;
        int l = 0;
        on[q] = t < d.DR;
        ar[q] = bs[q] = 0;
        acc[q] = 0.f;
        if (on[q]) eqx_decode(d, t, l, ar[q], bs[q]);
        on[q] = on[q] && (only_l < 0 || l == only_l);
    }
    const int n = dst[e];
    for (int c0 = 0; c0 < HV; c0 += 64) {
        const int c = c0 + lane;
        const bool live = c < HV;
        const float a = live ? alpha[(size_t)e * NH + c / V] : 0.f;
        const float* zr = z + (size_t)e * d.Sr * HV + c;
        const float* g = dagg + (size_t)n * d.S * HV + c;
        for (int s = 0; s < d.S; ++s) Bs[s * EQX_LD + lane] = live ? g[(size_t)s * HV] : 0.f;
        for (int r = 0; r < d.Sr; ++r) As[r * EQX_LD + lane] = live ? zr[(size_t)r * HV] * a * d.resc[d.r_l[r]] : 0.f;
        __syncthreads();
        eqx_panel_dot(As, Bs, ar, bs, on, min(64, HV - c0), acc);
        __syncthreads();
    }
    float* o = dwig + (size_t)e * d.DR;
#pragma unroll
    for (int q = 0; q < EQX_Q; ++q)
        if (on[q]) o[lane + 64 * q] = o[lane + 64 * q] + acc[q];
}

// ------------------------------------------------------------------------------------------------ live Gaussian basis
// w0t [NB, EC] = the Gaussian columns of W0 [EC, ldw], transposed, so that a wave reads a column's EC weights as one row
__global__ void eqx_w0t_kernel(const float* __restrict__ W0, int ldw, int NB, int EC, float* __restrict__ w0t) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= NB * EC) return;
    const int c = t / NB, k = t - c * NB;
    w0t[(size_t)k * EC + c] = W0[(size_t)c * ldw + k];
}

// One wave per edge.  Lane q evaluates g'_{k0 + q} once, the wave reads it by shuffle; lane = channel forms T_c with k
// ascending and leaves dh0[e, c] T_c in LDS; lane 0 adds the EC products in index order.
__global__ __launch_bounds__(64) void eqx_gauss_dgrad_kernel(const float* __restrict__ dist, const float* __restrict__ w0t,
                                                            const float* __restrict__ dh0, int NB, int EC, float rc, float delta,
                                                            float coeff, float* __restrict__ ddist) {
    __shared__ float part[1024];   // EC <= 1024 (adf_eqv2_create)
    const long long e = blockIdx.x;
    const int lane = threadIdx.x;
    const float dd = dist[e];
    int k0, k1;
    eq_gauss_window(dd, delta, eq_gauss_tmax(coeff), NB, k0, k1);
    if (k1 < k0) return;   // (uniform over the wave) no function of the basis reaches this distance: nothing is added
    float gl = 0.f;
    if (k0 + lane <= k1) gl = eq_gauss_dvalue(dd, k0 + lane, NB, rc, delta, coeff);
    for (int c0 = 0; c0 < EC; c0 += 64) {
        const int c = c0 + lane;
        const bool live = c < EC;
        float acc = 0.f;
        for (int k = k0; k <= k1; ++k) {
            const float gk = __shfl(gl, k - k0);
            if (live) acc += gk * w0t[(size_t)k * EC + c];
        }
        if (live) part[c] = dh0[(size_t)e * EC + c] * acc;
    }
    __syncthreads();
    if (lane == 0) {
        float s = 0.f;
        for (int c = 0; c < EC; ++c) s += part[c];
        ddist[e] = ddist[e] + s;
    }
}

// ------------------------------------------------------------------------------------------------ Wigner rows -> edge vectors
// One wave per edge (a workgroup walks edges blockIdx.x, + gridDim.x, ...; the generator tables are staged once).  Lane
// + 64 i = element (row ri, column j) of degree l: (wig_l K_k)[ri][j] = sum_b wig[ri][b] K_k[b][j], b ascending; the lane's
// products with dwig are added over l, then i, ascending; the 64 partial torques meet in a butterfly (offsets 32 .. 1).
__global__ __launch_bounds__(64) void eqx_wigner_bwd_kernel(const float* __restrict__ vec, const float* __restrict__ wig,
                                                           const float* __restrict__ dwig, const float* __restrict__ ddist,
                                                           const float* __restrict__ kgen, eq_dims d, long long E,
                                                           float* __restrict__ dvec) {
    __shared__ float Ks[3 * EQX_NJ];
    const int lane = threadIdx.x, nJ = d.j_off[d.L + 1];
    for (int t = lane; t < 3 * nJ; t += 64) Ks[t] = kgen[t];
    __syncthreads();
    for (long long e = blockIdx.x; e < E; e += gridDim.x) {
        const float* W = wig + (size_t)e * d.DR;
        const float* G = dwig + (size_t)e * d.DR;
        float tx = 0.f, ty = 0.f, tz = 0.f;
        for (int l = 1; l <= d.L; ++l) {
            const int n = 2 * l + 1, nr = d.nrow[l];
            const float* Kx = Ks + d.j_off[l];
            const float* Ky = Kx + nJ;
            const float* Kz = Ky + nJ;
            const float* Wl = W + d.d_off[l];
            for (int t = lane; t < nr * n; t += 64) {
                const int ri = t / n, j = t - ri * n;
                float ax = 0.f, ay = 0.f, az = 0.f;
                for (int b = 0; b < n; ++b) {
                    const float w = Wl[ri * n + b];
                    ax += w * Kx[b * n + j];
                    ay += w * Ky[b * n + j];
                    az += w * Kz[b * n + j];
                }
                const float g = G[d.d_off[l] + t];
                tx += g * ax;
                ty += g * ay;
                tz += g * az;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            tx += __shfl_xor(tx, off);
            ty += __shfl_xor(ty, off);
            tz += __shfl_xor(tz, off);
        }
        if (lane == 0) {
            const float vx = vec[3 * e], vy = vec[3 * e + 1], vz = vec[3 * e + 2];
            const float inv = 1.0f / eq_gauss_dist(vx, vy, vz);
            const float nx = vx * inv, ny = vy * inv, nz = vz * inv;
            const float dr = ddist[e];
            dvec[3 * e] = dr * nx + (ny * tz - nz * ty) * inv;
            dvec[3 * e + 1] = dr * ny + (nz * tx - nx * tz) * inv;
            dvec[3 * e + 2] = dr * nz + (nx * ty - ny * tx) * inv;
        }
    }
}

// ------------------------------------------------------------------------------------------------ edge vectors -> atoms
// A thread per atom: incoming edges in list order, then outgoing edges in the order of the source-sorted permutation.
__global__ void eqx_edge_to_atoms_kernel(const float* __restrict__ dvec, const int32_t* __restrict__ eptr,
                                         const int32_t* __restrict__ sptr, const int32_t* __restrict__ sperm, int N, long long E,
                                         float* __restrict__ forces) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float gx = 0.f, gy = 0.f, gz = 0.f;
    long long a0 = eptr[n], a1 = eptr[n + 1];
    a0 = a0 < 0 ? 0 : a0; a1 = a1 > E ? E : a1;
    for (long long e = a0; e < a1; ++e) { gx -= dvec[3 * e]; gy -= dvec[3 * e + 1]; gz -= dvec[3 * e + 2]; }
    long long b0 = sptr[n], b1 = sptr[n + 1];
    b0 = b0 < 0 ? 0 : b0; b1 = b1 > E ? E : b1;
    for (long long k = b0; k < b1; ++k) {
        long long e = sperm[k];
        e = e < 0 ? 0 : (e >= E ? E - 1 : e);
        gx += dvec[3 * e]; gy += dvec[3 * e + 1]; gz += dvec[3 * e + 2];
    }
    forces[3 * n] = 0.f - gx;
    forces[3 * n + 1] = 0.f - gy;
    forces[3 * n + 2] = 0.f - gz;
}

// ------------------------------------------------------------------------------------------------ entries
extern "C" int32_t adf_op_eq_rotate_in_bwd_wig(adf_eqv2_t h, const float* x, const int32_t* src, const int32_t* dst,
                                               const float* radial, const float* dout, int64_t E, float* dwig, void* stream) {
    ADF_TRY(eqx_handle(h, "eq_rotate_in_bwd_wig"));
    if (E < 0 || E > 2147483647LL) { adf_set_error("eq_rotate_in_bwd_wig: bad argument"); return ADF_EINVAL; }
    if (E == 0) return ADF_OK;
    if (!x || !src || !dst || !radial || !dout || !dwig) { adf_set_error("eq_rotate_in_bwd_wig: null argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(eqx_rotate_in_wig_kernel, dim3((unsigned)E), dim3(64), 0, (hipStream_t)stream, x, src, dst, radial, dout,
                       h->d, dwig);
    EQX_LAUNCHED();
    return ADF_OK;
}

extern "C" int32_t adf_op_eq_rotate_out_bwd_wig(adf_eqv2_t h, const float* z, const float* alpha, int32_t NH, int32_t V,
                                                const int32_t* dst, const float* dagg, int32_t only_l, int64_t E, float* dwig,
                                                void* stream) {
    ADF_TRY(eqx_handle(h, "eq_rotate_out_bwd_wig"));
    if (E < 0 || E > 2147483647LL || NH < 1 || V < 1 || (long long)NH * V > 2147483647LL / EQX_ROWS || only_l > h->d.L) {
        adf_set_error("eq_rotate_out_bwd_wig: bad argument");
        return ADF_EINVAL;
    }
    if (E == 0) return ADF_OK;
    if (!z || !alpha || !dst || !dagg || !dwig) { adf_set_error("eq_rotate_out_bwd_wig: null argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(eqx_rotate_out_wig_kernel, dim3((unsigned)E), dim3(64), 0, (hipStream_t)stream, z, alpha, (int)NH, (int)V,
                       dst, dagg, (int)only_l, h->d, dwig);
    EQX_LAUNCHED();
    return ADF_OK;
}

extern "C" int32_t adf_op_eq_radial_gauss_dgrad(adf_eqv2_t h, const float* dist, const float* W0, int32_t ldw, const float* dh0,
                                                int64_t E, float* ddist, float* scratch, int64_t scratch_floats, void* stream) {
    if (!h) { adf_set_error("eq_radial_gauss_dgrad: null handle"); return ADF_EINVAL; }
    const int NB = h->d.NB, EC = h->d.EC;
    if (NB < 2 || EC < 1 || EC > 1024 || E < 0 || E > 2147483647LL || ldw < NB) {
        adf_set_error("eq_radial_gauss_dgrad: bad argument");
        return ADF_EINVAL;
    }
    if (E == 0) return ADF_OK;
    if (!dist || !W0 || !dh0 || !ddist || !scratch) { adf_set_error("eq_radial_gauss_dgrad: null argument"); return ADF_EINVAL; }
    if (scratch_floats < (int64_t)NB * EC) {
        adf_set_error("eq_radial_gauss_dgrad: scratch holds %lld floats, needs %lld", (long long)scratch_floats, (long long)NB * EC);
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const float rc = h->hp.max_radius, delta = eq_gauss_delta(rc, NB), coeff = eq_gauss_coeff(delta);
    hipLaunchKernelGGL(eqx_w0t_kernel, dim3((unsigned)(((long long)NB * EC + 255) / 256)), dim3(256), 0, s, W0, (int)ldw, NB, EC,
                       scratch);
    EQX_LAUNCHED();
    hipLaunchKernelGGL(eqx_gauss_dgrad_kernel, dim3((unsigned)E), dim3(64), 0, s, dist, (const float*)scratch, dh0, NB, EC, rc,
                       delta, coeff, ddist);
    EQX_LAUNCHED();
    return ADF_OK;
}

extern "C" int32_t adf_op_eq_wigner_bwd(adf_eqv2_t h, const float* vec, const float* wig, const float* dwig, const float* ddist,
                                        int64_t E, float* dvec, void* stream) {
    ADF_TRY(eqx_handle(h, "eq_wigner_bwd"));
    if (E < 0 || E > 2147483647LL) { adf_set_error("eq_wigner_bwd: bad argument"); return ADF_EINVAL; }
    if (E == 0) return ADF_OK;
    if (!vec || !wig || !dwig || !ddist || !dvec) { adf_set_error("eq_wigner_bwd: null argument"); return ADF_EINVAL; }
    const unsigned grid = (unsigned)(E < 16384 ? E : 16384);
    hipLaunchKernelGGL(eqx_wigner_bwd_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, vec, wig, dwig, ddist,
                       (const float*)h->kgen, h->d, (long long)E, dvec);
    EQX_LAUNCHED();
    return ADF_OK;
}

extern "C" int32_t adf_op_eq_edge_grad_to_atoms(const float* dvec, const int32_t* eptr, const int32_t* sptr, const int32_t* sperm,
                                                int32_t N, int64_t E, float* forces, void* stream) {
    if (N < 0 || E < 0 || E > 2147483647LL) { adf_set_error("eq_edge_grad_to_atoms: bad argument"); return ADF_EINVAL; }
    if (N == 0) return ADF_OK;
    if (!eptr || !sptr || !forces || (E > 0 && (!dvec || !sperm))) { adf_set_error("eq_edge_grad_to_atoms: null argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(eqx_edge_to_atoms_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dvec, eptr,
                       sptr, sperm, (int)N, (long long)E, forces);
    EQX_LAUNCHED();
    return ADF_OK;
}
