// S2EF training of the OCP PaiNN force field: the objective and the energy head's backward.
//
// Objective (adf_op_s2ef_loss): OCPTrainer._compute_loss (trainers/ocp_trainer.py:308-356) with DDPLoss (modules/loss.py:48-102)
// over nn.L1Loss for the energy ("mae") and L2MAELoss for the forces ("l2mae"), the loss names of the shipped configs
// (utils/utils.py:1219-1260, 1319-1331), the model's outputs taken as normalised predictions:
//   energy term = c_E W / B_glob  sum_b |E_pred[b] - (E[b] - mean_E) / std_E|
//   force term  = c_F W / M_glob  sum_{i in S} ||F_pred[i] - (F[i] - mean_F) / std_F||_2      S: free atoms (or all atoms)
// Three small launches: one wave per system writes the system's partial sums (fixed lane order, butterfly), one thread
// combines the systems in ascending order and fixes the two divisors, one wave per system writes dE / dF from its own rows
// and the two divisors.  No float atomics: the result is run-to-run identical, and a system's gradient rows do not depend
// on the batch it sits in once the divisors are given.
//
// Energy head backward (adf_op_energy_head_bwd): out_energy.2 (H/2 -> 1), the per-system sum and the ScaledSiLU before it in
// one pass over the stored pre-activation he0 [N, H/2] (models/painn/painn.py:412-414).  A bandwidth-bound column reduction:
// a workgroup owns 64 consecutive rows x 64 consecutive columns, lane = column (a wave reads 256 contiguous bytes of a row),
// wave w takes rows w, w + 4, ...; the four waves' sums are combined in wave order into one partial row, and a second
// launch adds the partial rows in a fixed order: 16 contiguous groups of chunks, each ascending, then the groups in order
// (the scheme of lbfgs.hip's dot products).  energy_grad.hip's seed
// kernel is the dE == 1, data-gradient-only case and evaluates the same adf_dssilu_times().
#include "common.h"

#define S2_CHECK_LAUNCH() ADF_HIP_CHECK(hipGetLastError())

enum { S2_PART = 6 };         // per-system partials: |dE| sum, force-norm sum, |S|, energy abs error, force abs error, free atoms
enum { EH_ROWS = 64, EH_COLS = 64 };

// one wave per system: partial sums of the system
__global__ __launch_bounds__(64) void s2_loss_part_kernel(
    const float* __restrict__ E_pred, const float* __restrict__ F_pred, const float* __restrict__ E_tgt,
    const float* __restrict__ F_tgt, const int32_t* __restrict__ fixed, const int32_t* __restrict__ atom_offset,
    int free_only, float mean_E, float std_E, float mean_F, float std_F, float* __restrict__ part) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int a0 = atom_offset[b], a1 = atom_offset[b + 1];
    float sn = 0.f, cnt = 0.f, fae = 0.f, nfree = 0.f;
    for (int a = a0 + lane; a < a1; a += 64) {
        const bool is_free = !fixed || fixed[a] == 0;
        const bool in_s = !free_only || is_free;
        if (is_free) nfree += 1.f;
        if (in_s) cnt += 1.f;
        if (!F_pred) continue;
        float q = 0.f;
        for (int k = 0; k < 3; ++k) {
            const float p = F_pred[3 * (size_t)a + k], t = F_tgt[3 * (size_t)a + k];
            const float r = p - (t - mean_F) / std_F;
            q = fmaf(r, r, q);
            if (is_free) fae += fabsf(fmaf(p, std_F, mean_F) - t);
        }
        if (in_s) sn += sqrtf(q);
    }
    sn = adf_wave_sum(sn); cnt = adf_wave_sum(cnt); fae = adf_wave_sum(fae); nfree = adf_wave_sum(nfree);
    if (lane == 0) {
        const float p = E_pred[b], t = E_tgt[b];
        float* o = part + (size_t)S2_PART * b;
        o[0] = fabsf(p - (t - mean_E) / std_E);
        o[1] = sn; o[2] = cnt;
        o[3] = fabsf(fmaf(p, std_E, mean_E) - t);
        o[4] = fae; o[5] = nfree;
    }
}

// the systems in ascending order; scale[0] = c_E W / B_glob, scale[1] = c_F W / M_glob for the gradient launch
__global__ void s2_loss_sum_kernel(const float* __restrict__ part, int B, int has_forces, float c_E, float c_F,
                                   const long long* __restrict__ counts, float* __restrict__ loss,
                                   float* __restrict__ metrics, float* __restrict__ scale) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float se = 0.f, sf = 0.f, cnt = 0.f, eae = 0.f, fae = 0.f, nfree = 0.f;
    for (int b = 0; b < B; ++b) {
        const float* p = part + (size_t)S2_PART * b;
        se += p[0]; sf += p[1]; cnt += p[2]; eae += p[3]; fae += p[4]; nfree += p[5];
    }
    const float W = counts ? (float)counts[2] : 1.f;
    const float Bg = counts ? (float)counts[0] : (float)B;
    const float Mg = counts ? (float)counts[1] : cnt;
    const float ke = c_E * W / Bg, kf = c_F * W / Mg;
    const float le = ke * se, lf = has_forces ? kf * sf : 0.f;
    loss[0] = le + lf; loss[1] = le; loss[2] = lf;
    metrics[0] = eae / (float)B;
    metrics[1] = has_forces && nfree > 0.f ? fae / (3.f * nfree) : 0.f;
    scale[0] = ke; scale[1] = kf;
}

// one wave per system: dE[b] = scale[0] sign(r_b), dF[i] = scale[1] r_i / ||r_i|| inside S, zero outside and at r = 0
__global__ __launch_bounds__(64) void s2_loss_grad_kernel(
    const float* __restrict__ E_pred, const float* __restrict__ F_pred, const float* __restrict__ E_tgt,
    const float* __restrict__ F_tgt, const int32_t* __restrict__ fixed, const int32_t* __restrict__ atom_offset,
    int free_only, float mean_E, float std_E, float mean_F, float std_F, const float* __restrict__ scale,
    float* __restrict__ dE, float* __restrict__ dF) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int a0 = atom_offset[b], a1 = atom_offset[b + 1];
    if (lane == 0) {
        const float r = E_pred[b] - (E_tgt[b] - mean_E) / std_E;
        dE[b] = r > 0.f ? scale[0] : (r < 0.f ? -scale[0] : (r == 0.f ? 0.f : r));   // (a NaN residual stays NaN)
    }
    if (!F_pred) return;
    const float kf = scale[1];
    for (int a = a0 + lane; a < a1; a += 64) {
        const bool in_s = !free_only || !fixed || fixed[a] == 0;
        float r[3], q = 0.f;
        for (int k = 0; k < 3; ++k) {
            r[k] = F_pred[3 * (size_t)a + k] - (F_tgt[3 * (size_t)a + k] - mean_F) / std_F;
            q = fmaf(r[k], r[k], q);
        }
        const float nrm = sqrtf(q);
        for (int k = 0; k < 3; ++k) dF[3 * (size_t)a + k] = (in_s && nrm != 0.f) ? kf * (r[k] / nrm) : 0.f;
    }
}

extern "C" int32_t adf_op_s2ef_loss(const float* E_pred, const float* F_pred, const float* E_tgt, const float* F_tgt,
                                    const int32_t* fixed, const int32_t* atom_offset, int32_t B, int32_t free_only,
                                    float mean_E, float std_E, float mean_F, float std_F, float c_E, float c_F,
                                    const int64_t* counts, float* loss, float* dE, float* dF, float* metrics, float* scratch,
                                    void* stream) {
    if (!E_pred || !E_tgt || !atom_offset || !loss || !dE || !metrics || !scratch || B <= 0) {
        adf_set_error("s2ef_loss: null argument or no system");
        return ADF_EINVAL;
    }
    if (F_pred && (!F_tgt || !dF)) { adf_set_error("s2ef_loss: force predictions without targets or gradient output"); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    float* scale = scratch + (size_t)S2_PART * B;
    hipLaunchKernelGGL(s2_loss_part_kernel, dim3(B), dim3(64), 0, s, E_pred, F_pred, E_tgt, F_tgt, fixed, atom_offset,
                       free_only, mean_E, std_E, mean_F, std_F, scratch);
    hipLaunchKernelGGL(s2_loss_sum_kernel, dim3(1), dim3(64), 0, s, scratch, B, F_pred ? 1 : 0, c_E, c_F,
                       reinterpret_cast<const long long*>(counts), loss, metrics, scale);
    hipLaunchKernelGGL(s2_loss_grad_kernel, dim3(B), dim3(64), 0, s, E_pred, F_pred, E_tgt, F_tgt, fixed, atom_offset,
                       free_only, mean_E, std_E, mean_F, std_F, scale, dE, dF);
    S2_CHECK_LAUNCH();
    return ADF_OK;
}

extern "C" int64_t adf_op_s2ef_loss_scratch(int32_t B) { return (int64_t)S2_PART * (B > 0 ? B : 0) + 2; }

// energy[b] = sum over the system's atoms of (y[a] . w + bias) with y the activated hidden layer: the fixed-order sum of
// adf_painn_forward_energy, for a forward that keeps the pre-activation
extern "C" int32_t adf_op_energy_sum(const float* y, int32_t H2, const float* w, const float* bias, const int32_t* atom_offset,
                                     float* energy, int32_t B, void* stream) {
    if (!y || !w || !bias || !atom_offset || !energy || B <= 0 || H2 <= 0) { adf_set_error("energy_sum: bad argument"); return ADF_EINVAL; }
    return adf_energy_sum(y, H2, w, bias, atom_offset, energy, B, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ energy head backward
// workgroup (x: row chunk, y: column tile); part [chunks, H2 + 1]: the chunk's share of dW2, and of db2 in column H2
__global__ __launch_bounds__(256) void eh_bwd_kernel(const float* __restrict__ he0, const float* __restrict__ w2,
                                                     const float* __restrict__ dE, const int32_t* __restrict__ atom_sys,
                                                     float* __restrict__ dhe0, float* __restrict__ part, long long N, int H2) {
    __shared__ float red[4][EH_COLS + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * EH_COLS + lane;
    const bool on = c < H2;
    const long long r0 = (long long)blockIdx.x * EH_ROWS;
    const long long r1 = r0 + EH_ROWS < N ? r0 + EH_ROWS : N;
    const float wc = on ? w2[c] : 0.f;
    const int nrows = (int)(r1 - r0);
    // the chunk's upstream gradients once per wave (lane = row), handed out by shuffles: the row loop then holds no
    // dependent index -> value loads, and its four rows' loads are issued before the first is used
    float gl = 1.0f;
    if (dE && lane < nrows) gl = dE[atom_sys[r0 + lane]];
    float sw = 0.f, sb = 0.f;
    for (int i = wave; i < nrows; i += 16) {   // rows i, i + 4, i + 8, i + 12: this wave's rows in ascending order
        float x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ri = i + 4 * u;
            x[u] = (on && ri < nrows) ? he0[(size_t)(r0 + ri) * H2 + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ri = i + 4 * u;   // (wave-uniform, as is the branch on it)
            const float g = __shfl(gl, ri < nrows ? ri : 0, 64);
            if (ri < nrows) {
                sb = __fadd_rn(sb, g);
                if (on) {
                    dhe0[(size_t)(r0 + ri) * H2 + c] = g * adf_dssilu_times(x[u], wc);
                    sw = fmaf(g, adf_ssilu(x[u]), sw);
                }
            }
        }
    }
    if (!part) return;
    red[wave][lane] = sw;
    if (lane == 0) red[wave][EH_COLS] = sb;
    __syncthreads();
    if (wave == 0) {
        float* row = part + (size_t)blockIdx.x * (H2 + 1);
        if (on) row[c] = __fadd_rn(__fadd_rn(red[0][lane], red[1][lane]), __fadd_rn(red[2][lane], red[3][lane]));
        if (lane == 0 && blockIdx.y == 0)
            row[H2] = __fadd_rn(__fadd_rn(red[0][EH_COLS], red[1][EH_COLS]), __fadd_rn(red[2][EH_COLS], red[3][EH_COLS]));
    }
}

// column c (c == H2: the bias) summed over the chunks: thread (column, group) adds its contiguous share of the chunks in
// ascending order (16 groups, so that no thread walks the whole list alone: its loads are its latency), then the 16 group
// sums are added in group order.  The partition depends on the chunk count only: a fixed order for a given N.
enum { EH_GROUPS = 16 };
__global__ __launch_bounds__(64 * EH_GROUPS) void eh_bwd_sum_kernel(const float* __restrict__ part, long long chunks, int H2,
                                                                    float* __restrict__ dW2, float* __restrict__ db2,
                                                                    int accumulate) {
    __shared__ float red[EH_GROUPS][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const long long span = (chunks + EH_GROUPS - 1) / EH_GROUPS;
    const long long p0 = grp * span, p1 = p0 + span < chunks ? p0 + span : chunks;
    float s = 0.f;
    if (c <= H2)
        for (long long p = p0; p < p1; ++p) s = __fadd_rn(s, part[(size_t)p * (H2 + 1) + c]);
    red[grp][lane] = s;
    __syncthreads();
    if (grp != 0 || c > H2) return;
    float t = 0.f;
    for (int g = 0; g < EH_GROUPS; ++g) t = __fadd_rn(t, red[g][lane]);
    float* o = c < H2 ? dW2 + c : db2;
    *o = accumulate ? *o + t : t;
}

static inline long long eh_chunks(long long N) { return (N + EH_ROWS - 1) / EH_ROWS; }

extern "C" int64_t adf_op_energy_head_bwd_scratch(int64_t N, int32_t H2) {
    return N > 0 && H2 > 0 ? (int64_t)eh_chunks(N) * (H2 + 1) : 0;
}

extern "C" int32_t adf_op_energy_head_bwd(const float* he0, const float* w2, const float* dE, const int32_t* atom_sys,
                                          float* dhe0, float* dW2, float* db2, int32_t accumulate, int64_t N, int32_t H2,
                                          float* scratch, void* stream) {
    if (!he0 || !w2 || !dhe0 || N <= 0 || H2 <= 0) { adf_set_error("energy_head_bwd: bad argument"); return ADF_EINVAL; }
    if (dE && !atom_sys) { adf_set_error("energy_head_bwd: dE without the atoms' system index"); return ADF_EINVAL; }
    const bool params = dW2 || db2;
    if (params && (!dW2 || !db2 || !scratch)) { adf_set_error("energy_head_bwd: dW2, db2 and scratch go together"); return ADF_EINVAL; }
    const long long chunks = eh_chunks(N);
    if (chunks > 0x7fffffffll) { adf_set_error("energy_head_bwd: too many rows"); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(eh_bwd_kernel, dim3((unsigned)chunks, (unsigned)((H2 + EH_COLS - 1) / EH_COLS)), dim3(256), 0, s, he0,
                       w2, dE, atom_sys, dhe0, params ? scratch : nullptr, (long long)N, H2);
    if (params)
        hipLaunchKernelGGL(eh_bwd_sum_kernel, dim3((unsigned)((H2 + 1 + 63) / 64)), dim3(64 * EH_GROUPS), 0, s, scratch, chunks, H2, dW2,
                           db2, accumulate);
    S2_CHECK_LAUNCH();
    return ADF_OK;
}
