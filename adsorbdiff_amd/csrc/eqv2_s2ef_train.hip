// Training operators of the EquiformerV2 S2EF force field: the Gaussian part of a radial MLP's first layer
// on the live distance basis, forward and weight gradient (csrc/eqv2_s2ef_train.h states the contract and the orders).
// The basis - g_k, the centres, coeff, the window - is eqv2_gauss.h's, the definition the inference forward's
// eq_radial_live_kernel evaluates; nothing of it is restated here.
//
// Plain kernels.  Exact f32; every sum in one fixed order and every output element written by one thread, so two calls
// on the same input give the same bits.
#include "eqv2.h"
#include "eqv2_gauss.h"
#include "eqv2_s2ef_train.h"

#define EQG_LAUNCHED() ADF_HIP_CHECK(hipGetLastError())
#define EQG_EPW 4          // consecutive edges per wave of the forward
#define EQG_BWD_WAVES 8    // partial sums P_0 .. P_7 of a column of the weight gradient

struct eqg_basis {
    int NB, EC;
    float rc, delta, coeff;
};

static int32_t eqg_basis_of(const adf_eqv2* h, const char* who, eqg_basis* g) {
    if (!h) { adf_set_error("%s: null handle", who); return ADF_EINVAL; }
    g->NB = h->d.NB; g->EC = h->d.EC; g->rc = h->hp.max_radius;
    if (g->NB < 2 || g->EC < 1) { adf_set_error("%s: the handle has no distance basis", who); return ADF_EINVAL; }
    g->delta = eq_gauss_delta(g->rc, g->NB);
    g->coeff = eq_gauss_coeff(g->delta);
    return ADF_OK;
}

static inline unsigned eqg_blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// ------------------------------------------------------------------------------------------------ distances
__global__ void eqg_dist_kernel(const float* __restrict__ vec, long long E, float* __restrict__ dist) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) dist[e] = eq_gauss_dist(vec[3 * e], vec[3 * e + 1], vec[3 * e + 2]);
}

extern "C" int32_t adf_op_eq_edge_dist(const float* vec, int64_t E, float* dist, void* stream) {
    if (E < 0 || E > 2147483647LL) { adf_set_error("eq_edge_dist: bad argument"); return ADF_EINVAL; }
    if (E == 0) return ADF_OK;   // (an empty tensor has no address)
    if (!vec || !dist) { adf_set_error("eq_edge_dist: null argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(eqg_dist_kernel, dim3(eqg_blocks(E, 256)), dim3(256), 0, (hipStream_t)stream, vec, (long long)E, dist);
    EQG_LAUNCHED();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ forward
// w0t [NB, EC] = the Gaussian columns of W0 [EC, ldw], transposed: thread = element of W0 in its own order (reads coalesced)
__global__ void eqg_transpose_kernel(const float* __restrict__ W0, int ldw, int NB, int EC, float* __restrict__ w0t) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= NB * EC) return;
    const int c = t / NB, k = t - c * NB;
    w0t[(size_t)k * EC + c] = W0[(size_t)c * ldw + k];
}

// One wave per edge, EQG_EPW consecutive edges per wave, four waves per workgroup; lane = channel (64 at a time), so a row
// of w0t is read as coalesced 256-byte segments; lane q evaluates the q-th Gaussian of the window once and the wave
// reads it by shuffle (the layout of eq_radial_live_kernel).
__global__ __launch_bounds__(256) void eqg_fwd_kernel(const float* __restrict__ dist, const float* __restrict__ w0t, eqg_basis g,
                                                      long long E, float* __restrict__ h0) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float tmax = eq_gauss_tmax(g.coeff);
    for (int i = 0; i < EQG_EPW; ++i) {
        const long long e = ((long long)blockIdx.x * 4 + wave) * EQG_EPW + i;
        if (e >= E) return;
        const float d = dist[e];
        int k0, k1;
        eq_gauss_window(d, g.delta, tmax, g.NB, k0, k1);
        if (k1 < k0) continue;   // (wave-uniform: no function of the basis reaches this distance)
        float gl = 0.f;
        if (k0 + lane <= k1) gl = eq_gauss_value(d, k0 + lane, g.NB, g.rc, g.delta, g.coeff);
        float* row = h0 + (size_t)e * g.EC;
        for (int c0 = 0; c0 < g.EC; c0 += 64) {
            const int c = c0 + lane;
            const bool on = c < g.EC;
            float acc = 0.f;
            for (int k = k0; k <= k1; ++k) {
                const float gk = __shfl(gl, k - k0);
                if (on) acc += gk * w0t[(size_t)k * g.EC + c];
            }
            if (on) row[c] = row[c] + acc;
        }
    }
}

extern "C" int32_t adf_op_eq_radial_gauss_fwd(adf_eqv2_t h, const float* dist, const float* W0, int32_t ldw, int64_t E,
                                              float* h0, float* scratch, int64_t scratch_floats, void* stream) {
    eqg_basis g;
    ADF_TRY(eqg_basis_of(h, "eq_radial_gauss_fwd", &g));
    if (E < 0 || E > 2147483647LL || ldw < g.NB) { adf_set_error("eq_radial_gauss_fwd: bad argument"); return ADF_EINVAL; }
    if (E == 0) return ADF_OK;
    if (!dist || !W0 || !h0 || !scratch) { adf_set_error("eq_radial_gauss_fwd: null argument"); return ADF_EINVAL; }
    if (scratch_floats < (int64_t)g.NB * g.EC) {
        adf_set_error("eq_radial_gauss_fwd: scratch holds %lld floats, needs %lld", (long long)scratch_floats, (long long)g.NB * g.EC);
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(eqg_transpose_kernel, dim3(eqg_blocks((long long)g.NB * g.EC, 256)), dim3(256), 0, s, W0, (int)ldw, g.NB,
                       g.EC, scratch);
    EQG_LAUNCHED();
    hipLaunchKernelGGL(eqg_fwd_kernel, dim3(eqg_blocks(E, 4 * EQG_EPW)), dim3(256), 0, s, dist, (const float*)scratch, g,
                       (long long)E, h0);
    EQG_LAUNCHED();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ weight gradient
// Sorted position i: the edge perm[i] (clamped), its distance and its window -> eperm, dsort, k0s, k1s [E] each.
__global__ void eqg_bwd_prepare_kernel(const float* __restrict__ dist, const int32_t* __restrict__ perm, eqg_basis g, long long E,
                                       int32_t* __restrict__ eperm, float* __restrict__ dsort, int32_t* __restrict__ k0s,
                                       int32_t* __restrict__ k1s) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    long long e = perm[i];
    e = e < 0 ? 0 : (e >= E ? E - 1 : e);
    const float d = dist[e];
    int k0, k1;
    eq_gauss_window(d, g.delta, eq_gauss_tmax(g.coeff), g.NB, k0, k1);
    eperm[i] = (int32_t)e;
    dsort[i] = d;
    k0s[i] = k0;
    k1s[i] = k1;
}

// first i in [0, E) with a[i] >= v (a not decreasing), E when there is none
__device__ __forceinline__ long long eqg_lower_bound(const int32_t* __restrict__ a, long long E, int v) {
    long long lo = 0, hi = E;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One workgroup per (column k, 64 channels): the column's edges are the sorted positions [lo, hi) with k1s >= k (from lo
// on) and k0s <= k (before hi).  Wave w walks i = lo + w, lo + w + 8, ... in ascending order, lane = channel: an edge's
// row of dh0 is one coalesced read; the eight partial sums meet in LDS and one thread per channel adds them in wave order.
__global__ __launch_bounds__(64 * EQG_BWD_WAVES) void eqg_bwd_kernel(const int32_t* __restrict__ eperm, const float* __restrict__ dsort,
                                                                    const int32_t* __restrict__ k0s, const int32_t* __restrict__ k1s,
                                                                    const float* __restrict__ dh0, eqg_basis g, long long E,
                                                                    float* __restrict__ dW0, int lddw) {
    __shared__ float part[EQG_BWD_WAVES][64];
    const int k = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 63);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long lo = eqg_lower_bound(k1s, E, k), hi = eqg_lower_bound(k0s, E, k + 1);
    if (hi <= lo) return;   // (uniform over the workgroup) no edge's window holds k: the column is not touched
    const bool on = c < g.EC;
    float acc = 0.f;
#pragma unroll 4
    for (long long i = lo + wave; i < hi; i += EQG_BWD_WAVES) {
        const float gk = eq_gauss_value(dsort[i], k, g.NB, g.rc, g.delta, g.coeff);
        const float v = on ? dh0[(size_t)eperm[i] * g.EC + c] : 0.f;
        acc += gk * v;
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && on) {
        float s = part[0][lane];
#pragma unroll
        for (int w = 1; w < EQG_BWD_WAVES; ++w) s += part[w][lane];
        float* o = dW0 + (size_t)c * lddw + k;
        *o = *o + s;
    }
}

extern "C" int32_t adf_op_eq_radial_gauss_bwd(adf_eqv2_t h, const float* dist, const int32_t* perm, const float* dh0, int64_t E,
                                              float* dW0, int32_t lddw, float* scratch, int64_t scratch_floats, void* stream) {
    eqg_basis g;
    ADF_TRY(eqg_basis_of(h, "eq_radial_gauss_bwd", &g));
    if (E < 0 || E > 2147483647LL || lddw < g.NB) { adf_set_error("eq_radial_gauss_bwd: bad argument"); return ADF_EINVAL; }
    if (E == 0) return ADF_OK;
    if (!dist || !perm || !dh0 || !dW0 || !scratch) { adf_set_error("eq_radial_gauss_bwd: null argument"); return ADF_EINVAL; }
    if (scratch_floats < 4 * E) {
        adf_set_error("eq_radial_gauss_bwd: scratch holds %lld floats, needs %lld", (long long)scratch_floats, (long long)(4 * E));
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    int32_t* eperm = (int32_t*)scratch;
    float* dsort = scratch + E;
    int32_t* k0s = (int32_t*)(scratch + 2 * E);
    int32_t* k1s = (int32_t*)(scratch + 3 * E);
    hipLaunchKernelGGL(eqg_bwd_prepare_kernel, dim3(eqg_blocks(E, 256)), dim3(256), 0, s, dist, perm, g, (long long)E, eperm, dsort,
                       k0s, k1s);
    EQG_LAUNCHED();
    hipLaunchKernelGGL(eqg_bwd_kernel, dim3((unsigned)g.NB, (unsigned)((g.EC + 63) / 64)), dim3(64 * EQG_BWD_WAVES), 0, s,
                       (const int32_t*)eperm, (const float*)dsort, (const int32_t*)k0s, (const int32_t*)k1s, dh0, g, (long long)E,
                       dW0, (int)lddw);
    EQG_LAUNCHED();
    return ADF_OK;
}
