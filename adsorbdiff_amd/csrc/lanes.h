// Lane-level device helpers, one copy each: reductions over the 64 lanes of a wave, over a workgroup, and the DPP maxima.
// gfx950 only: a wave is 64 lanes.
//
// Order is part of the contract (a floating-point sum depends on it, and callers promise bit-reproducible results):
//   wave:      a butterfly over lane distances 32, 16, 8, 4, 2, 1, in that direction; every lane ends with the result.
//   workgroup: the wave butterfly, one LDS word per wave, then wave 0's word combined with waves 1, 2, ... in index order
//              by every thread.
#pragma once
#include <hip/hip_runtime.h>

struct adf_op_sum {
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct adf_op_max {
    __device__ __forceinline__ int operator()(int a, int b) const { return max(a, b); }
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
};
struct adf_op_min {
    __device__ __forceinline__ int operator()(int a, int b) const { return min(a, b); }
    __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
};

template <typename T, typename Op>
__device__ __forceinline__ T adf_wave_reduce(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
template <typename T> __device__ __forceinline__ T adf_wave_sum(T v) { return adf_wave_reduce(v, adf_op_sum{}); }
template <typename T> __device__ __forceinline__ T adf_wave_max(T v) { return adf_wave_reduce(v, adf_op_max{}); }
template <typename T> __device__ __forceinline__ T adf_wave_min(T v) { return adf_wave_reduce(v, adf_op_min{}); }

// the least (key, idx) of the wave, ties to the lower index, left in every lane
template <typename K>
__device__ __forceinline__ void adf_wave_argmin(K& key, int& idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const K k2 = __shfl_xor(key, o, 64);
        const int i2 = __shfl_xor(idx, o, 64);
        if (k2 < key || (k2 == key && i2 < idx)) { key = k2; idx = i2; }
    }
}
// workgroup of NW waves; red: NW words of LDS, reusable at once (the entry barrier covers the previous reads)
template <int NW, typename T, typename Op>
__device__ __forceinline__ T adf_block_reduce(T v, T* red, Op op) {
    v = adf_wave_reduce(v, op);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) v = op(v, red[w]);
    return v;
}
template <int NW, typename T> __device__ __forceinline__ T adf_block_min(T v, T* red) { return adf_block_reduce<NW>(v, red, adf_op_min{}); }

// max over the 16 lanes of a DPP row (non-negative values), left in every lane: four v_max_f32 with row rotations
__device__ __forceinline__ float adf_row16_max(float v) {
#define ADF_ROR(n_) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + (n_), 0xf, 0xf, false))
    v = fmaxf(v, ADF_ROR(8));
    v = fmaxf(v, ADF_ROR(4));
    v = fmaxf(v, ADF_ROR(2));
    v = fmaxf(v, ADF_ROR(1));
#undef ADF_ROR
    return v;
}
// max over the 32 lanes of a half-wave (non-negative values), left in lanes 16-31 of the half: adf_row16_max, then lane 15
// of DPP rows 0 / 2 is broadcast into rows 1 / 3 (row_bcast:15, row mask 0xa; rows 0 / 2 receive 0)
__device__ __forceinline__ float adf_half32_max_hi(float v) {
    v = adf_row16_max(v);
    return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xa, 0xf, false)));
}
// max over aligned groups of 8 lanes (non-negative values), left in every lane: two quad permutes, then row_half_mirror
__device__ __forceinline__ float adf_lane8_max(float v) {
#define ADF_DPP(c_) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), (c_), 0xf, 0xf, false))
    v = fmaxf(v, ADF_DPP(0xb1));    // quad_perm [1,0,3,2]
    v = fmaxf(v, ADF_DPP(0x4e));    // quad_perm [2,3,0,1]
    v = fmaxf(v, ADF_DPP(0x141));   // row_half_mirror: lane i <-> 7 - i
#undef ADF_DPP
    return v;
}
