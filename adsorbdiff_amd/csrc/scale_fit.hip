// The statistic the scale-factor fit observes (modules/scaling/scale_factor.py:144-147): torch.mean(torch.var(x, dim=0)) of
// a float32 [N, H] table - the unbiased variance over the rows of every column, averaged over the columns.
//
// Float64 and two passes, as the textbook form: column means first, then the sums of the centred squares.  The rows are cut
// into R chunks; a workgroup owns one chunk of one tile of 256 columns, its four waves walk the chunk's rows (wave w takes
// rows w, w + 4, ...), every lane carries the 4 columns of its 16-byte load, and the four waves' sums meet in LDS in the
// order 0, 1, 2, 3.  The chunk partials are plain stores into scratch; a second kernel adds the R partials of a column in
// ascending order.  The last kernel is one workgroup: thread t adds columns t, t + 256, ... in ascending order, then a fixed
// tree over the 256 threads.  No atomics anywhere, and no order depends on timing: run-to-run bit-identical.
//
// Widths that are no multiple of 4 (the stand-alone operator takes any H >= 1; the handle's are multiples of 64) read their
// rows with scalar loads: the rows of such a table are not 16-byte aligned.
#include "base.h"

enum { CV_THREADS = 256, CV_TILE = 256, CV_MAX_CHUNKS = 256, CV_MIN_ROWS = 64 };

static int cv_chunks(int64_t N) {
    const int64_t r = (N + CV_MIN_ROWS - 1) / CV_MIN_ROWS;
    return (int)(r < 1 ? 1 : r > CV_MAX_CHUNKS ? CV_MAX_CHUNKS : r);
}

// part[chunk][c] = sum over the chunk's rows of x[r][c] (mean == null) or of (x[r][c] - mean[c])^2
template <bool VEC>
__global__ __launch_bounds__(CV_THREADS) void cv_partial_kernel(const float* __restrict__ x, int64_t N, int H, int rows_per_chunk,
                                                                const double* __restrict__ mean, double* __restrict__ part) {
    __shared__ double lds[3][CV_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * CV_TILE + 4 * lane;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
    const int64_t r1 = r0 + rows_per_chunk < N ? r0 + rows_per_chunk : N;
    double m[4] = {0.0, 0.0, 0.0, 0.0}, acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (mean) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k < H) m[k] = mean[c0 + k];
    }
    if (c0 < H) {
        for (int64_t r = r0 + wave; r < r1; r += 4) {
            const float* row = x + (size_t)r * H + c0;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (VEC) {   // H % 4 == 0: the whole quad is inside the row and 16-byte aligned
                const float4 q = *reinterpret_cast<const float4*>(row);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c0 + k < H) v[k] = row[k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double d = (double)v[k] - m[k];
                acc[k] += mean ? d * d : d;
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) lds[wave - 1][4 * lane + k] = acc[k];
    }
    __syncthreads();
    if (wave == 0 && c0 < H) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (c0 + k >= H) continue;
            const int j = 4 * lane + k;
            part[(size_t)blockIdx.y * H + c0 + k] = ((acc[k] + lds[0][j]) + lds[1][j]) + lds[2][j];
        }
    }
}

// out[c] = (part[0][c] + part[1][c] + ... + part[R-1][c]) / denom
__global__ __launch_bounds__(CV_THREADS) void cv_combine_kernel(const double* __restrict__ part, int R, int H, double denom,
                                                                double* __restrict__ out) {
    const int c = blockIdx.x * CV_THREADS + threadIdx.x;
    if (c >= H) return;
    double s = 0.0;
    for (int r = 0; r < R; ++r) s += part[(size_t)r * H + c];
    out[c] = s / denom;
}

// out[0] = (sum over the columns of (sum over the chunks of part[r][c]) / (N - 1)) / H
__global__ __launch_bounds__(CV_THREADS) void cv_final_kernel(const double* __restrict__ part, int R, int H, double nm1,
                                                              double* __restrict__ out) {
    __shared__ double lds[CV_THREADS];
    const int t = threadIdx.x;
    double tot = 0.0;
    for (int c = t; c < H; c += CV_THREADS) {
        double s = 0.0;
        for (int r = 0; r < R; ++r) s += part[(size_t)r * H + c];
        tot += s / nm1;
    }
    lds[t] = tot;
    __syncthreads();
    for (int w = CV_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) lds[t] += lds[t + w];
        __syncthreads();
    }
    if (t == 0) out[0] = lds[0] / (double)H;
}

extern "C" int64_t adf_op_column_variance_scratch(int64_t N, int32_t H) {
    if (N < 1 || H < 1) return 0;
    return (int64_t)sizeof(double) * ((int64_t)cv_chunks(N) + 1) * H;
}

extern "C" int32_t adf_op_column_variance(const float* x, int64_t N, int32_t H, double* out, void* scratch, void* stream) {
    if (!x || !out || !scratch) { adf_set_error("column_variance: null argument"); return ADF_EINVAL; }
    if (H < 1) { adf_set_error("column_variance: H=%d", H); return ADF_EINVAL; }
    if (N < 2) { adf_set_error("column_variance: the unbiased variance needs at least 2 rows, got %lld", (long long)N); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const int R = cv_chunks(N);
    const int rows = (int)((N + R - 1) / R);
    double* part = reinterpret_cast<double*>(scratch);   // [R][H]
    double* mean = part + (size_t)R * H;                 // [H]
    const dim3 grid((H + CV_TILE - 1) / CV_TILE, R);
    const bool vec = H % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
    if (vec) hipLaunchKernelGGL(cv_partial_kernel<true>, grid, dim3(CV_THREADS), 0, s, x, N, H, rows, (const double*)nullptr, part);
    else hipLaunchKernelGGL(cv_partial_kernel<false>, grid, dim3(CV_THREADS), 0, s, x, N, H, rows, (const double*)nullptr, part);
    hipLaunchKernelGGL(cv_combine_kernel, dim3((H + CV_THREADS - 1) / CV_THREADS), dim3(CV_THREADS), 0, s, part, R, H, (double)N, mean);
    if (vec) hipLaunchKernelGGL(cv_partial_kernel<true>, grid, dim3(CV_THREADS), 0, s, x, N, H, rows, (const double*)mean, part);
    else hipLaunchKernelGGL(cv_partial_kernel<false>, grid, dim3(CV_THREADS), 0, s, x, N, H, rows, (const double*)mean, part);
    hipLaunchKernelGGL(cv_final_kernel, dim3(1), dim3(CV_THREADS), 0, s, part, R, H, (double)(N - 1), out);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}
