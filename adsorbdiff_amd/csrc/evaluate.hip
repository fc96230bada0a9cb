// Evaluation metrics of both trainers on the device: what modules/evaluator.py computes for the tasks "s2ef", "is2rs" and
// "is2re" (Evaluator.task_metrics), accumulated over the batches of a validation pass without a device-to-host read.
//
// Accumulator: caller-owned device memory, double total[ADF_EVAL_SLOTS] and int64 numel[ADF_EVAL_SLOTS] (the reference's
// {"total", "numel"} per metric name; "metric" = total / numel is formed by the reader).  Every entry ADDS into it; the
// caller zeroes it.  Summation in the style of s2ef_train.hip: one wave per system writes the system's partial sums (each
// lane walks its atoms in ascending order, the lanes are combined by a butterfly), one thread then adds the systems in
// ascending order and adds the batch's sums into the accumulator.  No float atomics: run-to-run bit-identical, and the
// accumulator after batches A, B depends on A, B and their order only.
//
// Arithmetic: every per-element term is formed in float32 with separately rounded operations (no contraction), as the
// reference's float32 tensors form it - denorm is torch.add(torch.mul(x, std), mean), an error is abs(target - prediction),
// the thresholds 0.02 / 0.03 are compared in float32 - and every sum of terms is carried in float64.
//
// The one departure: a system without a free atom.  The reference takes .max() of an empty slice there and raises; here
// the system's force maximum counts as 0, so energy_forces_within_threshold is decided by its energy alone.  In the is2rs
// entry such a system has a NaN mean distance (0 / 0) and lies below no threshold, as numpy's mean of an empty array.
#include "base.h"
#include "lanes.h"

#define EV_CHECK_LAUNCH() ADF_HIP_CHECK(hipGetLastError())

enum { EV_PART = 8 };   // doubles per system, see the two *_part kernels

// Every product, sum and quotient below rounds on its own, as a torch op does: no contraction into fused multiply-adds
// anywhere in this file (a fused one is written fmaf), and the operators are used directly - the __f*_rn wrappers of the HIP
// headers are plain operators that the compiler may still contract, and __fsqrt_rn is the approximate native square root;
// sqrtf and / are the correctly rounded ones.
#pragma clang fp contract(off)
__device__ __forceinline__ float ev_add(float a, float b) { return a + b; }
__device__ __forceinline__ float ev_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float ev_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float ev_div(float a, float b) { return a / b; }
__device__ __forceinline__ double ev_dadd(double a, double b) { return a + b; }

// torch.norm(v, p=2, dim=-1) / linalg.vector_norm of a float32 row: torch's CPU reduction accumulates the squares with a
// fused multiply-add chain (checked bit for bit on 1e5 random rows; with separately rounded adds one row in ten differs)
__device__ __forceinline__ float ev_norm3(const float* v) {
    return sqrtf(fmaf(v[2], v[2], fmaf(v[1], v[1], ev_mul(v[0], v[0]))));
}

// ------------------------------------------------------------------------------------------------------------- s2ef
// part [B, EV_PART]: |dFx| sum, |dFy| sum, |dFz| sum, cosine sum, magnitude-error sum, atoms in scope, |dE|, within (0 / 1)
__global__ __launch_bounds__(64) void ev_s2ef_part_kernel(
    const float* __restrict__ E_pred, const float* __restrict__ F_pred, const float* __restrict__ E_tgt,
    const float* __restrict__ F_tgt, const int32_t* __restrict__ fixed, const int32_t* __restrict__ atom_offset,
    int N, int free_only, float mean_E, float std_E, float mean_F, float std_F, double* __restrict__ part) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int a0 = max(atom_offset[b], 0), a1 = min(atom_offset[b + 1], N);   // (never past the arrays, whatever the offsets say)
    double sx = 0.0, sy = 0.0, sz = 0.0, scos = 0.0, smag = 0.0;
    int cnt = 0;
    float fmax = 0.f;   // (errors are >= 0: the maximum of no atom is the departure's 0)
    for (int a = a0 + lane; a < a1; a += 64) {
        if (free_only && fixed && fixed[a] != 0) continue;
        float p[3], t[3], e[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = ev_add(ev_mul(F_pred[3 * (size_t)a + k], std_F), mean_F);
            t[k] = F_tgt[3 * (size_t)a + k];
            e[k] = fabsf(ev_sub(t[k], p[k]));
        }
        sx += (double)e[0]; sy += (double)e[1]; sz += (double)e[2];
        // a NaN error never passes "< 0.03": fmaxf would drop it, so it is carried as +inf
        const float em = fmaxf(fmaxf(e[0], e[1]), e[2]);
        fmax = (e[0] != e[0] || e[1] != e[1] || e[2] != e[2]) ? INFINITY : fmaxf(fmax, em);
        // torch.cosine_similarity(eps = 1e-8): each row over its norm clamped from below, then the dot product; an all-zero
        // row gives 0
        const float np_ = ev_norm3(p), nt = ev_norm3(t);
        const float dp = fmaxf(np_, 1e-8f), dt = fmaxf(nt, 1e-8f);
        float c = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) c = ev_add(c, ev_mul(ev_div(p[k], dp), ev_div(t[k], dt)));
        scos += (double)c;
        smag += (double)fabsf(ev_sub(np_, nt));
        cnt += 1;
    }
    sx = adf_wave_sum(sx); sy = adf_wave_sum(sy); sz = adf_wave_sum(sz); scos = adf_wave_sum(scos); smag = adf_wave_sum(smag);
    cnt = adf_wave_sum(cnt);
    fmax = adf_wave_max(fmax);
    if (lane == 0) {
        const float ee = fabsf(ev_sub(E_tgt[b], ev_add(ev_mul(E_pred[b], std_E), mean_E)));
        double* o = part + (size_t)EV_PART * b;
        o[0] = sx; o[1] = sy; o[2] = sz; o[3] = scos; o[4] = smag; o[5] = (double)cnt;
        o[6] = (double)ee;
        o[7] = (ee < 0.02f && fmax < 0.03f) ? 1.0 : 0.0;
    }
}

__global__ void ev_s2ef_sum_kernel(const double* __restrict__ part, int B, double* __restrict__ total,
                                   long long* __restrict__ numel) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s[EV_PART];
    for (int j = 0; j < EV_PART; ++j) s[j] = 0.0;
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < EV_PART; ++j) s[j] = ev_dadd(s[j], part[(size_t)EV_PART * b + j]);
    const long long M = (long long)s[5];
    total[ADF_EVAL_ENERGY_MAE] += s[6];                              numel[ADF_EVAL_ENERGY_MAE] += B;
    total[ADF_EVAL_FORCESX_MAE] += s[0];                             numel[ADF_EVAL_FORCESX_MAE] += M;
    total[ADF_EVAL_FORCESY_MAE] += s[1];                             numel[ADF_EVAL_FORCESY_MAE] += M;
    total[ADF_EVAL_FORCESZ_MAE] += s[2];                             numel[ADF_EVAL_FORCESZ_MAE] += M;
    total[ADF_EVAL_FORCES_MAE] += ev_dadd(ev_dadd(s[0], s[1]), s[2]);   numel[ADF_EVAL_FORCES_MAE] += 3 * M;
    total[ADF_EVAL_FORCES_COSINE_SIMILARITY] += s[3];                numel[ADF_EVAL_FORCES_COSINE_SIMILARITY] += M;
    total[ADF_EVAL_FORCES_MAGNITUDE_ERROR] += s[4];                  numel[ADF_EVAL_FORCES_MAGNITUDE_ERROR] += M;
    total[ADF_EVAL_ENERGY_FORCES_WITHIN_THRESHOLD] += s[7];          numel[ADF_EVAL_ENERGY_FORCES_WITHIN_THRESHOLD] += B;
}

extern "C" int64_t adf_eval_scratch(int32_t B) { return (int64_t)EV_PART * (B > 0 ? B : 0); }

extern "C" int32_t adf_eval_s2ef(const float* E_pred, const float* F_pred, const float* E_tgt, const float* F_tgt,
                                 const int32_t* fixed, const int32_t* atom_offset, int32_t B, int32_t N, int32_t free_only,
                                 float mean_E, float std_E, float mean_F, float std_F, double* total, int64_t* numel,
                                 double* scratch, void* stream) {
    if (!E_pred || !F_pred || !E_tgt || !F_tgt || !atom_offset || !total || !numel || !scratch || B <= 0 || N < 0) {
        adf_set_error("eval_s2ef: null argument or no system");
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ev_s2ef_part_kernel, dim3(B), dim3(64), 0, s, E_pred, F_pred, E_tgt, F_tgt, fixed, atom_offset,
                       N, free_only, mean_E, std_E, mean_F, std_F, scratch);
    hipLaunchKernelGGL(ev_s2ef_sum_kernel, dim3(1), dim3(64), 0, s, scratch, B, total, reinterpret_cast<long long*>(numel));
    EV_CHECK_LAUNCH();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------------------ is2rs
// numpy's x %= 1.0 on a float32: fmod, moved into [0, 1) for a negative remainder (the sum can round to 1.0, which is why
// the reference applies it twice)
__device__ __forceinline__ float ev_mod1(float x) {
    float r = fmodf(x, 1.0f);
    if (r != 0.f && r < 0.f) r = ev_add(r, 1.0f);
    return r;
}

// part [B, EV_PART]: |d| sum, d^2 sum, free atoms, thresholds above the system's mean minimum-image distance
__global__ __launch_bounds__(64) void ev_is2rs_part_kernel(
    const float* __restrict__ pos_pred, const float* __restrict__ pos_tgt, const float* __restrict__ cell,
    const int32_t* __restrict__ fixed, const int32_t* __restrict__ atom_offset, int N, const double* __restrict__ thresholds,
    int T, double* __restrict__ part) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int a0 = max(atom_offset[b], 0), a1 = min(atom_offset[b + 1], N);
    // the inverse of the cell (rows = lattice vectors): fractional = d . inv(cell), the reference's solve with cell.T
    float c[9], inv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) c[k] = cell[9 * (size_t)b + k];
    {   // (not cell3.h's adf_inv3: unguarded, assigned row by row, and compiled without contraction here)
        const float m00 = c[4] * c[8] - c[5] * c[7], m01 = c[5] * c[6] - c[3] * c[8], m02 = c[3] * c[7] - c[4] * c[6];
        const float det = c[0] * m00 + c[1] * m01 + c[2] * m02;
        const float r = 1.0f / det;
        inv[0] = m00 * r; inv[1] = (c[2] * c[7] - c[1] * c[8]) * r; inv[2] = (c[1] * c[5] - c[2] * c[4]) * r;
        inv[3] = m01 * r; inv[4] = (c[0] * c[8] - c[2] * c[6]) * r; inv[5] = (c[2] * c[3] - c[0] * c[5]) * r;
        inv[6] = m02 * r; inv[7] = (c[1] * c[6] - c[0] * c[7]) * r; inv[8] = (c[0] * c[4] - c[1] * c[3]) * r;
    }
    double sa = 0.0, sq = 0.0, sd = 0.0;
    int cnt = 0;
    for (int a = a0 + lane; a < a1; a += 64) {
        if (fixed && fixed[a] != 0) continue;
        float d[3], f[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float p = pos_pred[3 * (size_t)a + k], t = pos_tgt[3 * (size_t)a + k];
            d[k] = ev_sub(p, t);                // min_diff: prediction - target
            const float e = ev_sub(t, p);       // mae / mse: target - prediction
            sa += (double)fabsf(e);
            sq += (double)ev_mul(e, e);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float x = d[0] * inv[j] + d[1] * inv[3 + j] + d[2] * inv[6 + j];
            x = ev_mod1(ev_mod1(x));
            f[j] = x > 0.5f ? ev_sub(x, 1.0f) : x;
        }
        float m[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) m[j] = f[0] * c[j] + f[1] * c[3 + j] + f[2] * c[6 + j];
        sd += (double)ev_norm3(m);
        cnt += 1;
    }
    sa = adf_wave_sum(sa); sq = adf_wave_sum(sq); sd = adf_wave_sum(sd);
    cnt = adf_wave_sum(cnt);
    const double mean = sd / (double)cnt;   // no free atom: 0 / 0 = NaN, below no threshold
    int below = 0;
    for (int i = lane; i < T; i += 64) below += mean < thresholds[i] ? 1 : 0;
    below = adf_wave_sum(below);
    if (lane == 0) {
        double* o = part + (size_t)EV_PART * b;
        o[0] = sa; o[1] = sq; o[2] = (double)cnt; o[3] = (double)below;
    }
}

__global__ void ev_is2rs_sum_kernel(const double* __restrict__ part, int B, int T, double* __restrict__ total,
                                    long long* __restrict__ numel) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < 4; ++j) s[j] = ev_dadd(s[j], part[(size_t)EV_PART * b + j]);
    const long long M = (long long)s[2];
    total[ADF_EVAL_POSITIONS_AVERAGE_DISTANCE_WITHIN_THRESHOLD] += s[3];
    numel[ADF_EVAL_POSITIONS_AVERAGE_DISTANCE_WITHIN_THRESHOLD] += (long long)B * T;
    total[ADF_EVAL_POSITIONS_MAE] += s[0];   numel[ADF_EVAL_POSITIONS_MAE] += 3 * M;
    total[ADF_EVAL_POSITIONS_MSE] += s[1];   numel[ADF_EVAL_POSITIONS_MSE] += 3 * M;
}

extern "C" int32_t adf_eval_is2rs(const float* pos_pred, const float* pos_tgt, const float* cell, const int32_t* fixed,
                                  const int32_t* atom_offset, int32_t B, int32_t N, const double* thresholds, int32_t T,
                                  double* total, int64_t* numel, double* scratch, void* stream) {
    if (!pos_pred || !pos_tgt || !cell || !atom_offset || !thresholds || !total || !numel || !scratch || B <= 0 || N < 0 || T <= 0) {
        adf_set_error("eval_is2rs: null argument, no system or no threshold");
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ev_is2rs_part_kernel, dim3(B), dim3(64), 0, s, pos_pred, pos_tgt, cell, fixed, atom_offset, N,
                       thresholds, T, scratch);
    hipLaunchKernelGGL(ev_is2rs_sum_kernel, dim3(1), dim3(64), 0, s, scratch, B, T, total, reinterpret_cast<long long*>(numel));
    EV_CHECK_LAUNCH();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------------------ is2re
// one term per system: a single thread adds them in ascending order
__global__ void ev_is2re_kernel(const float* __restrict__ E_pred, const float* __restrict__ E_tgt, int B,
                                double* __restrict__ total, long long* __restrict__ numel) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double sa = 0.0, sq = 0.0;
    long long within = 0;
    for (int b = 0; b < B; ++b) {
        const float e = ev_sub(E_tgt[b], E_pred[b]);
        sa = ev_dadd(sa, (double)fabsf(e));
        sq = ev_dadd(sq, (double)ev_mul(e, e));
        within += fabsf(e) < 0.02f ? 1 : 0;
    }
    total[ADF_EVAL_ENERGY_MAE] += sa;                          numel[ADF_EVAL_ENERGY_MAE] += B;
    total[ADF_EVAL_ENERGY_MSE] += sq;                          numel[ADF_EVAL_ENERGY_MSE] += B;
    total[ADF_EVAL_ENERGY_WITHIN_THRESHOLD] += (double)within;  numel[ADF_EVAL_ENERGY_WITHIN_THRESHOLD] += B;
}

extern "C" int32_t adf_eval_is2re(const float* E_pred, const float* E_tgt, int32_t B, double* total, int64_t* numel,
                                  void* stream) {
    if (!E_pred || !E_tgt || !total || !numel || B <= 0) { adf_set_error("eval_is2re: null argument or no system"); return ADF_EINVAL; }
    hipLaunchKernelGGL(ev_is2re_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, E_pred, E_tgt, B, total,
                       reinterpret_cast<long long*>(numel));
    EV_CHECK_LAUNCH();
    return ADF_OK;
}

// -------------------------------------------------------------------------------------------------------------- add
// Evaluator.update with a plain number: total += value, numel += 1 (the per-batch loss, averaged over the batches)
__global__ void ev_add_kernel(const float* __restrict__ value, int slot, double* __restrict__ total,
                              long long* __restrict__ numel) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    total[slot] += (double)value[0];
    numel[slot] += 1;
}

extern "C" int32_t adf_eval_add(const float* value, int32_t slot, double* total, int64_t* numel, void* stream) {
    if (!value || !total || !numel || slot < 0 || slot >= ADF_EVAL_SLOTS) { adf_set_error("eval_add: null argument or slot out of range"); return ADF_EINVAL; }
    hipLaunchKernelGGL(ev_add_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, value, slot, total,
                       reinterpret_cast<long long*>(numel));
    EV_CHECK_LAUNCH();
    return ADF_OK;
}
