// Reproducible optimizer step and embedding backward: what a resumed training needs to retrace the
// uninterrupted one to the bit.  Three entry points, none with a float atomic:
//
//   adf_op_grad_sqnorm_multi   the squared global gradient norm of every tensor in two launches, summed in a fixed order,
//                              and the step's decision (apply / skip, clip factor, bias corrections, EMA decay) written
//                              into a device state block;
//   adf_op_adamw_multi         tr_adamw_kernel's arithmetic (train.hip) over every tensor in one launch, reading that block;
//   adf_op_embed_bwd_ordered   demb[Z[n]-1] += dx[n] in segments of atoms, the segments added in index order.
//
// The tensors are cut into chunks of ADF_OPT_CHUNK elements (the last chunk of a tensor is short); one workgroup owns one
// chunk.  Everything the sums depend on is the data and ADF_OPT_CHUNK: not the grid, the number of CUs or the timing.
#include <math.h>

#include "common.h"

#define OP_CHECK_LAUNCH() ADF_HIP_CHECK(hipGetLastError())

#define ADF_OPT_CHUNK 32768   // L: part of the contract; a multiple of 4 * OP_THREADS
#define OP_THREADS 256
#define OP_SEG 64             // atoms per segment of the ordered embedding backward

// one row per tensor (64 bytes; the host writes it as 8 x int64)
struct op_tensor {
    float* p;
    const float* g;       // null: no gradient, the tensor is skipped (torch skips grad is None)
    float* m;
    float* v;
    float* ema;           // null: no shadow
    long long numel;
    long long decay;      // 1: weight decay applies
    long long reserved;
};
// one row per chunk (16 bytes; 2 x int64)
struct op_chunk {
    long long tensor;
    long long offset;
};
// the state block (40 bytes); the host reads it at state_dict() only
struct op_state {
    long long applied;    // updates really made
    long long skipped;    // steps whose norm was not finite
    int apply;            // this step
    float clip, bc1, bc2, ema_decay, sqnorm;
};

__device__ __forceinline__ bool op_aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

// ------------------------------------------------------------------------------------------------ gradient norm
// Stage 1.  Thread t owns the quads q = t, t + 256, ... of the chunk (quad q = elements 4q .. 4q + 3) and adds their
// squares one by one in element order; the scalar path (pointer not 16-byte aligned, or the chunk's short tail) loads the
// same elements in the same order, so both paths give the same bits.
__global__ void __launch_bounds__(OP_THREADS) op_sqnorm_stage1_kernel(const op_tensor* __restrict__ tensors,
                                                                      const op_chunk* __restrict__ chunks,
                                                                      float* __restrict__ partials) {
    const op_chunk ck = chunks[blockIdx.x];
    const op_tensor tn = tensors[ck.tensor];
    float s = 0.f;
    if (tn.g != nullptr) {
        const float* g = tn.g + ck.offset;
        long long left = tn.numel - ck.offset;
        const int len = left < ADF_OPT_CHUNK ? (int)left : ADF_OPT_CHUNK;
        const bool vec = op_aligned16(g);
        for (int e = threadIdx.x * 4; e < len; e += OP_THREADS * 4) {
            if (vec && e + 3 < len) {
                const float4 x = *reinterpret_cast<const float4*>(g + e);
                s = __fmaf_rn(x.x, x.x, s);
                s = __fmaf_rn(x.y, x.y, s);
                s = __fmaf_rn(x.z, x.z, s);
                s = __fmaf_rn(x.w, x.w, s);
            } else {
                const int hi = e + 4 < len ? e + 4 : len;
                for (int k = e; k < hi; ++k) {
                    const float x = g[k];
                    s = __fmaf_rn(x, x, s);
                }
            }
        }
    }
    // fixed shuffle tree within the wave, then the waves in wave order through LDS
    // kept inline: as a call to lanes.h this butterfly reorders the kernel's instructions (tools/device_asm_diff.py)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    __shared__ float ws[OP_THREADS / 64];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = ws[0];
#pragma unroll
        for (int w = 1; w < OP_THREADS / 64; ++w) t += ws[w];
        partials[blockIdx.x] = t;
    }
}

// Stage 2: one workgroup.  The partials are staged through LDS in tiles (coalesced loads) and added in index order in
// double by one thread, which then decides the step.
__global__ void __launch_bounds__(OP_THREADS) op_sqnorm_stage2_kernel(const float* __restrict__ partials, int nchunks,
                                                                      op_state* __restrict__ state, float max_norm,
                                                                      double beta1, double beta2, float ema_decay,
                                                                      long long ema_updates0) {
    __shared__ float tile[OP_THREADS];
    double total = 0.0;
    for (int base = 0; base < nchunks; base += OP_THREADS) {
        const int i = base + (int)threadIdx.x;
        tile[threadIdx.x] = i < nchunks ? partials[i] : 0.f;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int n = nchunks - base < OP_THREADS ? nchunks - base : OP_THREADS;
            for (int k = 0; k < n; ++k) total += (double)tile[k];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const float sq = (float)total;
    state->sqnorm = sq;
    const bool finite = (sq == sq) && !(sq > 3.0e38f) && !(sq < -3.0e38f);
    if (!finite) {
        state->apply = 0;
        state->skipped += 1;
        return;
    }
    const long long applied = state->applied + 1;
    state->applied = applied;
    state->apply = 1;
    state->bc1 = (float)(1.0 - pow(beta1, (double)applied));
    state->bc2 = (float)(1.0 - pow(beta2, (double)applied));
    float clip = 1.0f;
    if (max_norm > 0.f) {   // torch.nn.utils.clip_grad_norm_: coef = max_norm / (norm + 1e-6), clamped to 1
        const float c = max_norm / (sqrtf(sq) + 1e-6f);
        clip = c < 1.0f ? c : 1.0f;
    }
    state->clip = clip;
    float decay = ema_decay;
    if (ema_updates0 >= 0) {   // the EMA warms its decay up with its update count (exponential_moving_average.py)
        const double n = (double)(ema_updates0 + applied);
        const double w = (1.0 + n) / (10.0 + n);
        if (w < (double)ema_decay) decay = (float)w;
    }
    state->ema_decay = decay;
}

extern "C" int64_t adf_op_optimizer_chunk(void) { return ADF_OPT_CHUNK; }

extern "C" int32_t adf_op_grad_sqnorm_multi(const void* tensors, const void* chunks, int32_t nchunks, float* partials,
                                            void* state, float max_norm, double beta1, double beta2, float ema_decay,
                                            int64_t ema_updates0, void* stream) {
    if (!tensors || !chunks || !partials || !state || nchunks < 1) {
        adf_set_error("grad_sqnorm_multi: null table or no chunk");
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(op_sqnorm_stage1_kernel, dim3(nchunks), dim3(OP_THREADS), 0, s, (const op_tensor*)tensors,
                       (const op_chunk*)chunks, partials);
    hipLaunchKernelGGL(op_sqnorm_stage2_kernel, dim3(1), dim3(OP_THREADS), 0, s, partials, nchunks, (op_state*)state, max_norm,
                       beta1, beta2, ema_decay, (long long)ema_updates0);
    OP_CHECK_LAUNCH();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ AdamW over every tensor
// tr_adamw_kernel's arithmetic (train.hip), element by element, unchanged in order and form
__device__ __forceinline__ void op_adamw_element(float& pi, float gi, float& mi, float& vi, float* ema, bool has_ema, float clip,
                                                 float lr, float beta1, float beta2, float eps, float wd, float bc1, float bc2,
                                                 float ema_decay) {
    gi = gi * clip;
    pi *= 1.0f - lr * wd;
    mi = beta1 * mi + (1.0f - beta1) * gi;
    vi = beta2 * vi + (1.0f - beta2) * gi * gi;
    pi -= lr / bc1 * mi / (sqrtf(vi) / sqrtf(bc2) + eps);
    if (has_ema) *ema += (1.0f - ema_decay) * (pi - *ema);
}

__global__ void __launch_bounds__(OP_THREADS) op_adamw_multi_kernel(const op_tensor* __restrict__ tensors,
                                                                    const op_chunk* __restrict__ chunks,
                                                                    const op_state* __restrict__ state, float lr, float beta1,
                                                                    float beta2, float eps, float weight_decay) {
    if (!state->apply) return;   // a non-finite norm: parameters, moments and shadows keep their bits
    const op_chunk ck = chunks[blockIdx.x];
    const op_tensor tn = tensors[ck.tensor];
    if (tn.g == nullptr) return;
    const float clip = state->clip, bc1 = state->bc1, bc2 = state->bc2, ema_decay = state->ema_decay;
    const float wd = tn.decay ? weight_decay : 0.f;
    float* p = tn.p + ck.offset;
    const float* g = tn.g + ck.offset;
    float* m = tn.m + ck.offset;
    float* v = tn.v + ck.offset;
    const bool has_ema = tn.ema != nullptr;
    float* ema = has_ema ? tn.ema + ck.offset : nullptr;
    long long left = tn.numel - ck.offset;
    const int len = left < ADF_OPT_CHUNK ? (int)left : ADF_OPT_CHUNK;
    const bool vec = op_aligned16(p) && op_aligned16(g) && op_aligned16(m) && op_aligned16(v) && (!has_ema || op_aligned16(ema));
    for (int e = threadIdx.x * 4; e < len; e += OP_THREADS * 4) {
        if (vec && e + 3 < len) {
            float4 p4 = *reinterpret_cast<float4*>(p + e);
            const float4 g4 = *reinterpret_cast<const float4*>(g + e);
            float4 m4 = *reinterpret_cast<float4*>(m + e);
            float4 v4 = *reinterpret_cast<float4*>(v + e);
            float4 s4 = has_ema ? *reinterpret_cast<float4*>(ema + e) : make_float4(0.f, 0.f, 0.f, 0.f);
            op_adamw_element(p4.x, g4.x, m4.x, v4.x, &s4.x, has_ema, clip, lr, beta1, beta2, eps, wd, bc1, bc2, ema_decay);
            op_adamw_element(p4.y, g4.y, m4.y, v4.y, &s4.y, has_ema, clip, lr, beta1, beta2, eps, wd, bc1, bc2, ema_decay);
            op_adamw_element(p4.z, g4.z, m4.z, v4.z, &s4.z, has_ema, clip, lr, beta1, beta2, eps, wd, bc1, bc2, ema_decay);
            op_adamw_element(p4.w, g4.w, m4.w, v4.w, &s4.w, has_ema, clip, lr, beta1, beta2, eps, wd, bc1, bc2, ema_decay);
            *reinterpret_cast<float4*>(p + e) = p4;
            *reinterpret_cast<float4*>(m + e) = m4;
            *reinterpret_cast<float4*>(v + e) = v4;
            if (has_ema) *reinterpret_cast<float4*>(ema + e) = s4;
        } else {
            const int hi = e + 4 < len ? e + 4 : len;
            for (int k = e; k < hi; ++k) {
                float pi = p[k], mi = m[k], vi = v[k];
                float si = has_ema ? ema[k] : 0.f;
                op_adamw_element(pi, g[k], mi, vi, &si, has_ema, clip, lr, beta1, beta2, eps, wd, bc1, bc2, ema_decay);
                p[k] = pi; m[k] = mi; v[k] = vi;
                if (has_ema) ema[k] = si;
            }
        }
    }
}

extern "C" int32_t adf_op_adamw_multi(const void* tensors, const void* chunks, int32_t nchunks, const void* state, float lr,
                                      float beta1, float beta2, float eps, float weight_decay, void* stream) {
    if (!tensors || !chunks || !state || nchunks < 1) {
        adf_set_error("adamw_multi: null table or no chunk");
        return ADF_EINVAL;
    }
    hipLaunchKernelGGL(op_adamw_multi_kernel, dim3(nchunks), dim3(OP_THREADS), 0, (hipStream_t)stream,
                       (const op_tensor*)tensors, (const op_chunk*)chunks, (const op_state*)state, lr, beta1, beta2, eps,
                       weight_decay);
    OP_CHECK_LAUNCH();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ ordered embedding backward
// Stage 1, one workgroup per segment of OP_SEG atoms: for every element present in the segment, the sum of its atoms' rows
// in atom order, stored at the slot of the element's first atom; slot[seg, z] names that slot (-1: absent).
// scratch: partial rows [nseg * OP_SEG, H] floats, then the slot table [nseg, rows] int32.
__global__ void __launch_bounds__(OP_THREADS) op_embed_stage1_kernel(const float* __restrict__ dx, const int32_t* __restrict__ Z,
                                                                     float* __restrict__ partial, int32_t* __restrict__ slot,
                                                                     int N, int H, int rows) {
    __shared__ int zs[OP_SEG];     // row index of every atom of the segment (-1: out of range, contributes nothing)
    __shared__ int nxt[OP_SEG];    // the next atom of the segment with the same row (-1: none)
    __shared__ int first[OP_SEG];  // 1: no earlier atom of the segment has this row
    const int seg = blockIdx.x;
    const int base = seg * OP_SEG;
    const int cnt = N - base < OP_SEG ? N - base : OP_SEG;
    const int t = threadIdx.x;
    if (t < OP_SEG) {
        int z = -1;
        if (t < cnt) {
            z = Z[base + t] - 1;
            if (z < 0 || z >= rows) z = -1;
        }
        zs[t] = z;
    }
    __syncthreads();
    if (t < OP_SEG) {
        const int z = zs[t];
        int n = -1, f = z >= 0 ? 1 : 0;
        if (z >= 0) {
            for (int j = t + 1; j < cnt; ++j)
                if (zs[j] == z) { n = j; break; }
            for (int j = 0; j < t; ++j)
                if (zs[j] == z) { f = 0; break; }
        }
        nxt[t] = n;
        first[t] = f;
    }
    for (int z = t; z < rows; z += OP_THREADS) {
        int sl = -1;
        for (int j = 0; j < cnt; ++j)
            if (zs[j] == z) { sl = j; break; }
        slot[(size_t)seg * rows + z] = sl;
    }
    __syncthreads();
    for (int c = t; c < H; c += OP_THREADS) {
        for (int i = 0; i < cnt; ++i) {
            if (!first[i]) continue;
            float s = 0.f;
            for (int j = i; j >= 0; j = nxt[j]) s += dx[(size_t)(base + j) * H + c];
            partial[((size_t)base + i) * H + c] = s;
        }
    }
}

// Stage 2, one workgroup per embedding row and block of 256 columns: the segments in index order.  Eight partial rows are
// loaded at a time (an absent one counts as +0, which changes no sum) and added in segment order.
__global__ void __launch_bounds__(OP_THREADS) op_embed_stage2_kernel(const float* __restrict__ partial,
                                                                     const int32_t* __restrict__ slot, float* __restrict__ demb,
                                                                     int nseg, int H, int rows) {
    __shared__ int sl[OP_THREADS];
    const int z = blockIdx.x;
    const int c = blockIdx.y * OP_THREADS + threadIdx.x;
    float acc = 0.f;
    int present = 0;
    for (int s0 = 0; s0 < nseg; s0 += OP_THREADS) {
        const int mine = s0 + (int)threadIdx.x;
        sl[threadIdx.x] = mine < nseg ? slot[(size_t)mine * rows + z] : -1;
        __syncthreads();
        const int n = nseg - s0 < OP_THREADS ? nseg - s0 : OP_THREADS;
        if (c < H) {
            for (int k0 = 0; k0 < n; k0 += 8) {
                float x[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int i = k0 + k < n ? sl[k0 + k] : -1;
                    present |= i >= 0;
                    x[k] = i >= 0 ? partial[((size_t)(s0 + k0 + k) * OP_SEG + i) * H + c] : 0.f;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) acc += x[k];
            }
        }
        __syncthreads();
    }
    if (c < H && present) demb[(size_t)z * H + c] += acc;   // rows of absent elements are not touched
}

extern "C" int64_t adf_op_embed_bwd_ordered_scratch(int64_t N, int32_t H, int32_t rows) {
    const int64_t nseg = (N + OP_SEG - 1) / OP_SEG;
    return nseg * OP_SEG * (int64_t)H + nseg * (int64_t)rows;
}

extern "C" int32_t adf_op_embed_bwd_ordered(const float* dx, const int32_t* Z, float* demb, int32_t N, int32_t H, int32_t rows,
                                            float* scratch, void* stream) {
    if (!dx || !Z || !demb || !scratch || N < 1 || H < 1 || rows < 1) {
        adf_set_error("embed_bwd_ordered: null pointer or empty shape");
        return ADF_EINVAL;
    }
    const int nseg = (N + OP_SEG - 1) / OP_SEG;
    float* partial = scratch;
    int32_t* slot = reinterpret_cast<int32_t*>(scratch + (size_t)nseg * OP_SEG * H);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(op_embed_stage1_kernel, dim3(nseg), dim3(OP_THREADS), 0, s, dx, Z, partial, slot, N, H, rows);
    hipLaunchKernelGGL(op_embed_stage2_kernel, dim3(rows, (H + OP_THREADS - 1) / OP_THREADS), dim3(OP_THREADS), 0, s,
                       (const float*)partial, (const int32_t*)slot, demb, nseg, H, rows);
    OP_CHECK_LAUNCH();
    return ADF_OK;
}
