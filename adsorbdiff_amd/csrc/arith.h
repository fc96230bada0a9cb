// Scalar device arithmetic with one definition each.
#pragma once
#include <hip/hip_runtime.h>

// 2^e with mx 2^e in [2^14, 2^15); 1 for mx == 0 or non-finite: the per-row lift of the f16x3 products' A operands
__device__ __forceinline__ float adf_pow2_lift(float mx) {
    if (!(mx > 0.f) || !(mx < 3.0e38f)) return 1.0f;
    int e;
    (void)frexpf(mx, &e);
    e = 15 - e;
    e = e > 120 ? 120 : (e < -120 ? -120 : e);
    return ldexpf(1.0f, e);
}
__device__ __forceinline__ float adf_silu(float x) { return x / (1.0f + expf(-x)); }
// ScaledSiLU f(x) = x sigmoid(x) / 0.6 (gemnet_oc/layers/base_layers.py:65-72), f'(x), and f'(x) w as the energy head's
// backward evaluates it: the seed of the energy gradient (energy_grad.hip) and adf_op_energy_head_bwd (s2ef_train.hip)
__device__ __forceinline__ float adf_ssilu(float x) { return x / (1.0f + expf(-x)) * 1.6666666666666667f; }
__device__ __forceinline__ float adf_dssilu(float x) {
    const float sg = 1.0f / (1.0f + expf(-x));
    return sg * (1.0f + x * (1.0f - sg)) * 1.6666666666666667f;
}
__device__ __forceinline__ float adf_dssilu_times(float x, float w) { return adf_dssilu(x) * w; }
