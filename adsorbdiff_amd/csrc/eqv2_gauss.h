// The live Gaussian distance basis of the EquiformerV2 S2EF model (GaussianSmearing, equiformer_v2_oc20.py:41-62), ONE
// definition for the inference forward's first radial layer (eq_radial_live_kernel, eqv2_kernels.hip) and the training
// operators (eqv2_s2ef_train.hip): what is trained is what is inferred.
//
//   g_k(d) = exp(coeff (d - mu_k)^2),  k = 0 .. NB - 1
//
// * delta = rc / (NB - 1) in fp32: mu_1 - mu_0 of torch.linspace(0, rc, NB).
// * mu_k: torch.linspace's fp32 values - delta k from the start in the lower half, rc - delta (NB - 1 - k) in the upper.
// * coeff: the reference's double-precision -0.5 / (2 (mu_1 - mu_0))^2 rounded to fp32.
// * window of an edge: the k with |d - mu_k| < tmax = sqrt(104 / -coeff) = 2 delta sqrt(208) (beyond it exp underflows
//   to zero in fp32), clipped to [0, NB - 1] and to 64 functions (it holds at most 58, whatever NB and the cutoff).  A
//   term outside the window is never formed.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define EQ_GAUSS_WINDOW_MAX 64   // one lane per function of the window

static inline float eq_gauss_delta(float rc, int NB) { return rc / (float)(NB - 1); }
static inline float eq_gauss_coeff(float delta) {
    return (float)(-0.5 / (((double)(2.0f * delta)) * ((double)(2.0f * delta))));
}

// |vec| of an edge, the distance every g_k is evaluated at
__device__ __forceinline__ float eq_gauss_dist(float vx, float vy, float vz) { return sqrtf(vx * vx + vy * vy + vz * vz); }

__host__ __device__ __forceinline__ float eq_gauss_tmax(float coeff) { return sqrtf(104.0f / -coeff); }

// first and last function of the window of distance `dist` (k1 < k0: empty)
__host__ __device__ __forceinline__ void eq_gauss_window(float dist, float delta, float tmax, int NB, int& k0, int& k1) {
    k0 = (int)ceilf((dist - tmax) / delta);
    k1 = (int)floorf((dist + tmax) / delta);
    k0 = k0 > 0 ? k0 : 0;
    k1 = k1 < NB - 1 ? k1 : NB - 1;
    k1 = k1 < k0 + (EQ_GAUSS_WINDOW_MAX - 1) ? k1 : k0 + (EQ_GAUSS_WINDOW_MAX - 1);
}

__host__ __device__ __forceinline__ float eq_gauss_centre(int k, int NB, float rc, float delta) {
    return k < NB / 2 ? delta * (float)k : rc - delta * (float)(NB - 1 - k);
}

__device__ __forceinline__ float eq_gauss_value(float dist, int k, int NB, float rc, float delta, float coeff) {
    const float t = dist - eq_gauss_centre(k, NB, rc, delta);
    return expf(coeff * (t * t));
}

// d g_k / d dist at `dist`: g_k(d) 2 coeff (d - mu_k), the factors of eq_gauss_value (the geometric gradient, eqv2_geo.hip)
__device__ __forceinline__ float eq_gauss_dvalue(float dist, int k, int NB, float rc, float delta, float coeff) {
    const float t = dist - eq_gauss_centre(k, NB, rc, delta);
    return expf(coeff * (t * t)) * (2.0f * coeff * t);
}
