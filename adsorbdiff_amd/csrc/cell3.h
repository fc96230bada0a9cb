// Small fp32 / fp64 geometry of a cell (rows = lattice vectors), one copy each.  The expression order of every helper is
// part of its contract: callers promise bit-reproducible results.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define ADF_WRAP_EPS 1e-7   // ASE's wrap eps: f -> (f + eps) mod 1 - eps

template <typename T>
__device__ __forceinline__ void adf_cross3(const T* x, const T* y, T* o) {
    o[0] = x[1] * y[2] - x[2] * y[1];
    o[1] = x[2] * y[0] - x[0] * y[2];
    o[2] = x[0] * y[1] - x[1] * y[0];
}
template <typename T>
__device__ __forceinline__ T adf_dot3(const T* x, const T* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }

// inv = c^-1 by the adjugate: fractional coordinates are f_k = d . inv[:,k].  A cell of zero volume gives inv = 0.
// (unique.hip, symmetry.hip and evaluate.hip keep unguarded inverses of their own: 1 / 0 goes through there, which is
// observable, they assign the entries row by row, which orders their kernels' instructions differently, and
// evaluate.hip compiles its copy without contraction.)
template <typename T>
__device__ __forceinline__ void adf_inv3(const T* c, T* inv) {
    const T m0 = c[4] * c[8] - c[5] * c[7], m1 = c[5] * c[6] - c[3] * c[8], m2 = c[3] * c[7] - c[4] * c[6];
    const T vol = c[0] * m0 + c[1] * m1 + c[2] * m2;
    const T r = vol != (T)0 ? (T)1 / vol : (T)0;
    inv[0] = m0 * r; inv[3] = m1 * r; inv[6] = m2 * r;
    inv[1] = (c[2] * c[7] - c[1] * c[8]) * r; inv[4] = (c[0] * c[8] - c[2] * c[6]) * r; inv[7] = (c[1] * c[6] - c[0] * c[7]) * r;
    inv[2] = (c[1] * c[5] - c[2] * c[4]) * r; inv[5] = (c[2] * c[3] - c[0] * c[5]) * r; inv[8] = (c[0] * c[4] - c[1] * c[3]) * r;
}

// ASE's wrap of one fractional coordinate into [-eps, 1 - eps)
__device__ __forceinline__ double adf_mod1_eps(double f) { return (f + ADF_WRAP_EPS) - floor(f + ADF_WRAP_EPS) - ADF_WRAP_EPS; }

// (The refusing form of the range check, `a0 < 0 || a1 < a0 || a1 > N`, stays spelled out in every slab kernel: as a shared
// predicate it compiled to other instructions in placement, sites, triangulate and voronoi, tools/device_asm_diff.py.)
// the segment of system b clamped into [0, N]: first row and row count
__device__ __forceinline__ void adf_segment_clamp(const int32_t* __restrict__ offset, int b, int N, int& a0, int& n) {
    a0 = min(max(offset[b], 0), N);
    n = min(max(offset[b + 1], a0), N) - a0;
}
