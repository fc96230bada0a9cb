// Forward noising of a training batch on the device (adsorbdiff_amd/noising.py: DeviceNoiser).
// Reference: adsorbdiff/trainers/sde_denoising_trainer.py:45-135 (pbc_correction, tr_so3_schedule), :138-177
// (ads_COM_gaussian_schedule) and utils/rot_utils.py:18-98, 226-264 (axis_angle_to_matrix, sample_vec, score_vec, score_norm).
//
// The random numbers are counter based: a system's row of draws is a function of (seed, step, key of the system) alone
// (Philox4x32-10, Salmon et al., SC'11), so a system receives the same noise alone, in any batch and on any rank.
// Row layout (double [B,8]): (u_t, n0, n1, n2, n3, n4, n5, u_om); n0..2 the COM noise, n3..5 the rotation axis before
// normalisation, u_t / u_om the uniforms of the diffusion time and of the rotation angle's CDF look-up.
//
// adf_noise_tr_so3 / adf_noise_com: one wave per system.  The adsorbate is found by scanning tags over the system's atom
// range (it need not be contiguous or last); sums are wave reductions in a fixed order; no float atomics, no host read.
#include <stdlib.h>
#include <string.h>

#include "base.h"
#include "lanes.h"

#define NZ_CHECK_LAUNCH() ADF_HIP_CHECK(hipGetLastError())

// eps grid of the IGSO(3) tables (rot_utils.py:9-10)
#define NZ_MIN_EPS 0.01
#define NZ_MAX_EPS 2.0

// ------------------------------------------------------------------------------------------------ generator
__device__ __forceinline__ void nz_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                 uint32_t* out) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ double nz_unit(uint32_t w) { return ((double)w + 0.5) * 2.3283064365386963e-10; }   // 2^-32

__global__ void nz_draws_kernel(uint32_t seed_lo, uint32_t seed_hi, uint32_t step, const int64_t* __restrict__ keys, int B,
                                double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint64_t key = (uint64_t)keys[b];
    uint32_t w[8];
    nz_philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), step, 0u, seed_lo, seed_hi, w);
    nz_philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), step, 1u, seed_lo, seed_hi, w + 4);
    double* row = out + 8 * (size_t)b;
    row[0] = nz_unit(w[0]);
    row[7] = nz_unit(w[1]);
    for (int p = 0; p < 3; ++p) {   // Box-Muller on (a0,a1), (a2,a3), (a4,a5)
        const double r = sqrt(-2.0 * log(nz_unit(w[2 + 2 * p]))), ph = 2.0 * 3.141592653589793 * nz_unit(w[3 + 2 * p]);
        row[1 + 2 * p] = r * cos(ph);
        row[2 + 2 * p] = r * sin(ph);
    }
}
extern "C" int32_t adf_noise_draws(int64_t seed, int32_t step, const int64_t* keys, int32_t B, double* out, void* stream) {
    if (!keys || !out || B <= 0) { adf_set_error("noise_draws: bad argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(nz_draws_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, (uint32_t)(uint64_t)seed,
                       (uint32_t)((uint64_t)seed >> 32), (uint32_t)step, keys, B, out);
    NZ_CHECK_LAUNCH();
    return ADF_OK;
}

// The placement stage's rows (placement.hip): eight plain uniforms per (key, index), from the counters
// (key lo, key hi, index, 2) and (key lo, key hi, index, 3): the last counter word keeps them apart from the rows above.
__global__ void nz_place_draws_kernel(uint32_t seed_lo, uint32_t seed_hi, const int64_t* __restrict__ keys,
                                      const int32_t* __restrict__ index, int n, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = (uint64_t)keys[i];
    const uint32_t idx = (uint32_t)index[i];
    uint32_t w[8];
    nz_philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), idx, 2u, seed_lo, seed_hi, w);
    nz_philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), idx, 3u, seed_lo, seed_hi, w + 4);
    for (int k = 0; k < 8; ++k) out[8 * (size_t)i + k] = nz_unit(w[k]);
}
extern "C" int32_t adf_place_draws(int64_t seed, const int64_t* keys, const int32_t* index, int32_t n, double* out,
                                   void* stream) {
    if (!keys || !index || !out || n <= 0) { adf_set_error("place_draws: bad argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(nz_place_draws_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (uint32_t)(uint64_t)seed, (uint32_t)((uint64_t)seed >> 32), keys, index, n, out);
    NZ_CHECK_LAUNCH();
    return ADF_OK;
}

// The sampler's rows (denoising_torch.py: noise_seed): counters (key lo, key hi, t, 4 + 2 site + j), j in {0, 1} - the last
// counter word keeps them apart from the rows above (words 0 to 3) and from each other across the sites of one slab.
// Step row t in [0, T): six normals by the Box-Muller of nz_draws_kernel on (w0,w1), (w2,w3), (w4,w5), cast to float32:
// z_a[t,b] = (n0, n1, n2), z_b[t,b] = (n3, n4, n5).  Placement row: t = 0xFFFFFFFF, j = 0, place[b,k] = (w_k >> 8) * 2^-24,
// in [0, 1) and exact in float32 as torch.rand is (nz_unit would round to 1.0f for the largest words).
// One thread per (row, system); row T is the placement row.
__global__ void nz_sampler_draws_kernel(uint32_t seed_lo, uint32_t seed_hi, const int64_t* __restrict__ keys,
                                        const int32_t* __restrict__ site, int B, int T, float* __restrict__ place,
                                        float* __restrict__ z_a, float* __restrict__ z_b) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)(T + 1) * B) return;
    const int t = (int)(i / B), b = (int)(i % B);
    const uint64_t key = (uint64_t)keys[b];
    const uint32_t last = 4u + 2u * (uint32_t)(site ? site[b] : 0);
    uint32_t w[8];
    if (t == T) {
        if (!place) return;
        nz_philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), 0xFFFFFFFFu, last, seed_lo, seed_hi, w);
        for (int k = 0; k < 3; ++k) place[3 * (size_t)b + k] = (float)(w[k] >> 8) * 5.9604644775390625e-08f;   // 2^-24
        return;
    }
    if (!z_a && !z_b) return;
    nz_philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)t, last, seed_lo, seed_hi, w);
    nz_philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)t, last + 1u, seed_lo, seed_hi, w + 4);
    double n[6];
    for (int p = 0; p < 3; ++p) {
        const double r = sqrt(-2.0 * log(nz_unit(w[2 * p]))), ph = 2.0 * 3.141592653589793 * nz_unit(w[2 * p + 1]);
        n[2 * p] = r * cos(ph);
        n[2 * p + 1] = r * sin(ph);
    }
    const size_t row = 3 * ((size_t)t * B + b);
    if (z_a) for (int k = 0; k < 3; ++k) z_a[row + k] = (float)n[k];
    if (z_b) for (int k = 0; k < 3; ++k) z_b[row + k] = (float)n[3 + k];
}
// a site outside [0, 2^30) is ADF_EINVAL: the table lives on the device, so one flag is read back before the draws
__global__ void nz_site_range_kernel(const int32_t* __restrict__ site, int B, int32_t* __restrict__ bad) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && (site[b] < 0 || site[b] >= (1 << 30))) *bad = 1;
}
extern "C" int32_t adf_sampler_draws(int64_t seed, const int64_t* keys, const int32_t* site, int32_t B, int32_t T, float* place,
                                     float* z_a, float* z_b, void* stream) {
    if (!keys || B <= 0 || T < 0 || (!place && !z_a && !z_b) || ((z_a || z_b) && T == 0)) {
        adf_set_error("sampler_draws: bad argument");
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    if (site) {
        // (not host_util.h's adf_errword: a failed allocation here reports through ADF_HIP_CHECK, and adf_pool words it otherwise)
        int32_t* bad = nullptr;
        int32_t host_bad = 0;
        ADF_HIP_CHECK(hipMalloc(&bad, sizeof(int32_t)));
        hipError_t e = hipMemsetAsync(bad, 0, sizeof(int32_t), s);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(nz_site_range_kernel, dim3((B + 255) / 256), dim3(256), 0, s, site, B, bad);
            e = hipMemcpyAsync(&host_bad, bad, sizeof(int32_t), hipMemcpyDeviceToHost, s);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        (void)hipFree(bad);
        ADF_HIP_CHECK(e);
        if (host_bad) { adf_set_error("sampler_draws: site outside [0, 2^30)"); return ADF_EINVAL; }
    }
    const long long n = (long long)(T + 1) * B;
    hipLaunchKernelGGL(nz_sampler_draws_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (uint32_t)(uint64_t)seed,
                       (uint32_t)((uint64_t)seed >> 32), keys, site, B, T, place, z_a, z_b);
    NZ_CHECK_LAUNCH();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ table look-ups
// Igso3Tables.eps_index: nearest row of the log-spaced eps grid, clipped (np.around rounds halves to even, as rint does)
__device__ __forceinline__ int nz_eps_index(double eps, int n_eps) {
    const double idx = (log10(eps) - log10(NZ_MIN_EPS)) / (log10(NZ_MAX_EPS) - log10(NZ_MIN_EPS)) * (double)n_eps;
    const double r = rint(idx);
    if (!(r > 0.0)) return 0;            // also NaN
    if (r > (double)(n_eps - 1)) return n_eps - 1;
    return (int)r;
}
// last k in [0, n) with a[k] <= x, -1 when there is none (np.searchsorted(a, x, side="right") - 1)
__device__ __forceinline__ int nz_last_le(const double* __restrict__ a, int n, double x) {
    int lo = 0, hi = n;   // first index with a[k] > x lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}
// np.interp(x, xp, fp): slope * (x - x0) + f0 inside, the end values outside
__device__ __forceinline__ double nz_interp(double x, const double* __restrict__ xp, const double* __restrict__ fp, int n) {
    const int j = nz_last_le(xp, n, x);
    if (j < 0) return fp[0];
    if (x >= xp[n - 1]) return fp[n - 1];
    const int jc = j > n - 2 ? n - 2 : j;
    return (fp[jc + 1] - fp[jc]) / (xp[jc + 1] - xp[jc]) * (x - xp[jc]) + fp[jc];
}

__global__ void nz_score_norm_kernel(const float* __restrict__ rot_sigma, const double* __restrict__ table, int n_eps, int B,
                                     float* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) out[b] = (float)table[nz_eps_index((double)rot_sigma[b], n_eps)];
}
extern "C" int32_t adf_igso3_score_norm(const float* rot_sigma, const double* table, int32_t n_eps, int32_t B, float* out,
                                        void* stream) {
    if (!rot_sigma || !table || !out || n_eps <= 0 || B <= 0) { adf_set_error("igso3_score_norm: bad argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(nz_score_norm_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, rot_sigma, table, n_eps, B,
                       out);
    NZ_CHECK_LAUNCH();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ shared pieces
// centre of mass of the adsorbate (tag 2) of atoms [a0, a1): every lane returns the same values
__device__ __forceinline__ void nz_ads_center(const float* __restrict__ pos, const int32_t* __restrict__ tags, int a0, int a1,
                                              int lane, float* c) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int a = a0 + lane; a < a1; a += 64)
        if (tags[a] == 2) {
            for (int k = 0; k < 3; ++k) s[k] += (double)pos[3 * a + k];
            s[3] += 1.0;
        }
    for (int i = 0; i < 4; ++i) s[i] = adf_wave_sum(s[i]);
    const double cnt = s[3] > 1.0 ? s[3] : 1.0;
    for (int k = 0; k < 3; ++k) c[k] = (float)(s[k] / cnt);
}
__device__ __forceinline__ double nz_mod1(double x) {   // torch.remainder(x, 1)
    double r = fmod(x, 1.0);
    if (r < 0.0) r += 1.0;
    return r;
}
__device__ __forceinline__ float nz_mod1f(float x) {
    float r = fmodf(x, 1.0f);
    if (r < 0.f) r += 1.0f;
    return r;
}
// A f = v in float32 with partial pivoting (what torch.linalg.solve does for a float32 system)
__device__ void nz_solve3f(const float* A, const float* v, float* f) {
    float m[3][4];
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) m[r][c] = A[3 * r + c]; m[r][3] = v[r]; }
    for (int col = 0; col < 3; ++col) {
        int piv = col;
        for (int r = col + 1; r < 3; ++r) if (fabsf(m[r][col]) > fabsf(m[piv][col])) piv = r;
        if (piv != col) for (int c = 0; c < 4; ++c) { float t = m[col][c]; m[col][c] = m[piv][c]; m[piv][c] = t; }
        for (int r = col + 1; r < 3; ++r) {
            const float l = m[r][col] / m[col][col];
            for (int c = col; c < 4; ++c) m[r][c] = m[r][c] - l * m[col][c];
        }
    }
    f[2] = m[2][3] / m[2][2];
    f[1] = (m[1][3] - m[1][2] * f[2]) / m[1][1];
    f[0] = (m[0][3] - m[0][1] * f[1] - m[0][2] * f[2]) / m[0][0];
}
// pbc_correction of one vector: fractional coordinates by solving cell^T f = v in double (explicit inverse), into
// (-0.5, 0.5], back with the ROWS of cell in float32
__device__ void nz_pbc_correction(const float* __restrict__ cl, const float* v, float* out) {
    double A[3][3];   // A = cell^T
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) A[i][j] = (double)cl[3 * j + i];
    const double c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2],
                 c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
    const double det = A[0][0] * c00 + A[0][1] * c01 + A[0][2] * c02;
    const double inv[3][3] = {
        {c00 / det, (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det, (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det},
        {c01 / det, (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det, (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det},
        {c02 / det, (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det, (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det}};
    float fr[3];
    for (int i = 0; i < 3; ++i) {
        double f = inv[i][0] * (double)v[0] + inv[i][1] * (double)v[1] + inv[i][2] * (double)v[2];
        f = nz_mod1(nz_mod1(f));
        if (f > 0.5) f -= 1.0;
        fr[i] = (float)f;
    }
    for (int j = 0; j < 3; ++j) out[j] = fr[0] * cl[j] + fr[1] * cl[3 + j] + fr[2] * cl[6 + j];
}

// ------------------------------------------------------------------------------------------------ tr_so3_schedule
__global__ __launch_bounds__(64) void nz_tr_so3_kernel(
    const float* __restrict__ pos, const float* __restrict__ cell, const int32_t* __restrict__ tags,
    const int32_t* __restrict__ atom_offset, int B, int N, const double* __restrict__ draws, float ads_lo, float ads_hi,
    float rot_lo, float rot_hi, const double* __restrict__ omegas, const double* __restrict__ cdf,
    const double* __restrict__ score, const double* __restrict__ esn, int n_eps, int n_om, float* __restrict__ pos_out,
    float* __restrict__ tr_sigma, float* __restrict__ rot_sigma, float* __restrict__ tr_score, float* __restrict__ rot_score,
    float* __restrict__ noise_vec, float* __restrict__ rot_norm) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int a0 = atom_offset[b], a1 = atom_offset[b + 1];
    if (a0 < 0) a0 = 0;
    if (a1 > N) a1 = N;
    float center[3];
    nz_ads_center(pos, tags, a0, a1, lane, center);
    // the per-system scalars are computed by every lane alike (uniform reads of the row and of the tables)
    const double* row = draws + 8 * (size_t)b;
    const float t = (float)row[0];
    const float st = powf(ads_lo, 1.0f - t) * powf(ads_hi, t);
    const float sr = powf(rot_lo, 1.0f - t) * powf(rot_hi, t);
    float nv[3] = {(float)row[1] * st, (float)row[2] * st, (float)row[3] * st}, noise[3];
    nz_pbc_correction(cell + 9 * (size_t)b, nv, noise);
    noise[2] = 0.f;
    // rotation: axis / |axis| * omega(u_om), omega by inverting the CDF of row eps_index(sigma_rot)
    const int idx = nz_eps_index((double)sr, n_eps);
    const double* cdf_row = cdf + (size_t)idx * n_om;
    const double* score_row = score + (size_t)idx * n_om;
    const double x0 = row[4], x1 = row[5], x2 = row[6], u = row[7];
    const double nrm = sqrt(x0 * x0 + x1 * x1 + x2 * x2);
    const double omega = nz_interp(u, cdf_row, omegas, n_om);
    const double v[3] = {x0 / nrm * omega, x1 / nrm * omega, x2 / nrm * omega};
    const double om = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double sc = nz_interp(om, omegas, score_row, n_om);
    // rotation matrix through the unit quaternion (rot_utils.py:18-98; series below 1e-6), double, applied in float32
    const double half = 0.5 * om;
    const double kq = fabs(om) < 1e-6 ? 0.5 - om * om / 48.0 : sin(half) / om;
    const double qr = cos(half), qi = v[0] * kq, qj = v[1] * kq, qk = v[2] * kq;
    const double two_s = 2.0 / (qr * qr + qi * qi + qj * qj + qk * qk);
    const float R[9] = {(float)(1 - two_s * (qj * qj + qk * qk)), (float)(two_s * (qi * qj - qk * qr)),
                        (float)(two_s * (qi * qk + qj * qr)), (float)(two_s * (qi * qj + qk * qr)),
                        (float)(1 - two_s * (qi * qi + qk * qk)), (float)(two_s * (qj * qk - qi * qr)),
                        (float)(two_s * (qi * qk - qj * qr)), (float)(two_s * (qj * qk + qi * qr)),
                        (float)(1 - two_s * (qi * qi + qj * qj))};
    if (lane == 0) {
        tr_sigma[b] = st;
        rot_sigma[b] = sr;
        rot_norm[b] = (float)esn[idx];
        for (int k = 0; k < 3; ++k) {
            noise_vec[3 * b + k] = noise[k];
            tr_score[3 * b + k] = -noise[k] / (st * st);
            rot_score[3 * b + k] = (float)(sc * v[k] / om);
        }
    }
    for (int a = a0 + lane; a < a1; a += 64) {
        const float p[3] = {pos[3 * a], pos[3 * a + 1], pos[3 * a + 2]};
        if (tags[a] == 2) {
            const float r[3] = {p[0] - center[0], p[1] - center[1], p[2] - center[2]};
            for (int i = 0; i < 3; ++i) {
                float q = (r[0] * R[3 * i] + r[1] * R[3 * i + 1] + r[2] * R[3 * i + 2]) + noise[i] + center[i];
                if (i == 2) q += 1.0f;   // the reference lifts the noised adsorbate by 1 A
                pos_out[3 * a + i] = q;
            }
        } else {
            for (int i = 0; i < 3; ++i) pos_out[3 * a + i] = p[i];
        }
    }
}
extern "C" int32_t adf_noise_tr_so3(const float* pos, const float* cell, const int32_t* tags, const int32_t* atom_offset,
                                    int32_t B, int32_t N, const double* draws, float ads_std_low, float ads_std_high,
                                    float rot_std_low, float rot_std_high, const double* omegas, const double* cdf,
                                    const double* score, const double* exp_score_norm, int32_t n_eps, int32_t n_omega,
                                    float* pos_out, float* tr_sigma, float* rot_sigma, float* tr_score, float* rot_score,
                                    float* noise_vec, float* rot_norm, void* stream) {
    if (!pos || !cell || !tags || !atom_offset || !draws || !omegas || !cdf || !score || !exp_score_norm || !pos_out ||
        !tr_sigma || !rot_sigma || !tr_score || !rot_score || !noise_vec || !rot_norm || B <= 0 || N <= 0 || n_eps <= 0 ||
        n_omega < 2 || pos_out == pos) {
        adf_set_error("noise_tr_so3: bad argument");
        return ADF_EINVAL;
    }
    hipLaunchKernelGGL(nz_tr_so3_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, pos, cell, tags, atom_offset, B, N, draws,
                       ads_std_low, ads_std_high, rot_std_low, rot_std_high, omegas, cdf, score, exp_score_norm, n_eps, n_omega,
                       pos_out, tr_sigma, rot_sigma, tr_score, rot_score, noise_vec, rot_norm);
    NZ_CHECK_LAUNCH();
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------------ ads_COM_gaussian_schedule
__global__ __launch_bounds__(64) void nz_com_kernel(const float* __restrict__ pos, const float* __restrict__ cell,
                                                    const int32_t* __restrict__ tags, const int32_t* __restrict__ atom_offset,
                                                    int B, int N, const double* __restrict__ draws, float ads_lo, float ads_hi,
                                                    float* __restrict__ pos_out, float* __restrict__ tr_sigma,
                                                    float* __restrict__ tr_score, float* __restrict__ noise_vec) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int a0 = atom_offset[b], a1 = atom_offset[b + 1];
    if (a0 < 0) a0 = 0;
    if (a1 > N) a1 = N;
    float center[3];
    nz_ads_center(pos, tags, a0, a1, lane, center);
    const double* row = draws + 8 * (size_t)b;
    const float t = (float)row[0];
    const float st = powf(ads_lo, 1.0f - t) * powf(ads_hi, t);
    const float noise[3] = {(float)row[1] * st, (float)row[2] * st, 0.f};   // noise only in x, y
    const float* cl = cell + 9 * (size_t)b;
    const float tgt[3] = {center[0] + noise[0], center[1] + noise[1], center[2] + noise[2]};
    // the sampler's wrap: solve(cell, c) in float32, % 1 twice on all three components, back with cell . f
    float fr[3];
    nz_solve3f(cl, tgt, fr);
    for (int i = 0; i < 3; ++i) fr[i] = nz_mod1f(nz_mod1f(fr[i]));
    float c[3];
    for (int i = 0; i < 3; ++i) c[i] = cl[3 * i] * fr[0] + cl[3 * i + 1] * fr[1] + cl[3 * i + 2] * fr[2];
    c[2] += 1.0f;   // the reference lifts the noised adsorbate by 1 A
    if (lane == 0) {
        tr_sigma[b] = st;
        for (int k = 0; k < 3; ++k) {
            noise_vec[3 * b + k] = noise[k];
            tr_score[3 * b + k] = -noise[k] / (st * st);
        }
    }
    for (int a = a0 + lane; a < a1; a += 64) {
        const bool ads = tags[a] == 2;
        for (int i = 0; i < 3; ++i) pos_out[3 * a + i] = ads ? c[i] : pos[3 * a + i];   // the adsorbate collapses to its COM
    }
}
extern "C" int32_t adf_noise_com(const float* pos, const float* cell, const int32_t* tags, const int32_t* atom_offset, int32_t B,
                                 int32_t N, const double* draws, float ads_std_low, float ads_std_high, float* pos_out,
                                 float* tr_sigma, float* tr_score, float* noise_vec, void* stream) {
    if (!pos || !cell || !tags || !atom_offset || !draws || !pos_out || !tr_sigma || !tr_score || !noise_vec || B <= 0 ||
        N <= 0 || pos_out == pos) {
        adf_set_error("noise_com: bad argument");
        return ADF_EINVAL;
    }
    hipLaunchKernelGGL(nz_com_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, pos, cell, tags, atom_offset, B, N, draws,
                       ads_std_low, ads_std_high, pos_out, tr_sigma, tr_score, noise_vec);
    NZ_CHECK_LAUNCH();
    return ADF_OK;
}
