// Batched L-BFGS of ml_relax on the device (adsorbdiff/relaxation/optimizers/lbfgs_torch.py:22-213).
//
// State (all fp64, as the reference keeps it): the s / y history rings [memory, 3N], rho and alpha [memory], r0 / f0 [3N],
// the two-loop work vector q (z overwrites it) and the scaled step dr [3N].  The history bookkeeping (how many entries were
// appended, which ring slot holds logical entry i of the deque) lives on the host: it depends on the iteration numbers
// alone.  Every value decision (rho, alpha, the skip of a near-zero step) is taken on the device, so a step enqueues its
// kernels without a host synchronisation.
//
// Reductions.  The reference's dot products run over the whole flattened batch (systems are coupled through them).  An
// element kernel covers the 3N entries with G workgroups, each owning a contiguous chunk; a workgroup writes one partial
// sum (per-thread strided sums, then a fixed LDS tree).  The next launch finishes the dot: every workgroup sums the same G
// partials in the same fixed order, so all of them hold the same bits, and no atomics are involved anywhere.  One launch per
// history entry finishes the previous dot, applies the axpy of that entry and emits the partials of the next dot.
// Arithmetic that the reference performs as separate tensor ops (q - alpha * y, z + s * (alpha - beta), ...) is separately
// rounded.  The __dadd_rn / __dmul_rn spelling marks those places but does not do it: hipcc defines them as plain + and *,
// which the device default -ffp-contract=fast fuses into FMAs once inlined.  This file is therefore compiled with
// -ffp-contract=off (build.py, EXTRA_FLAGS); tests/test_gpu_relax_coupled.py checks z bit for bit against the float64
// statement of the step with this file's summation order.
//
// Per-system mode (adf_lbfgs_set_per_system).  Every system keeps its own step counter, its slice of the rings and its own
// rho / alpha [memory]; one workgroup per system walks a whole step in ONE launch (lb_per_system_kernel).  Thread t owns
// elements t, t + LB_THREADS, ... of its system's q / z; a dot product is the per-thread strided sum followed by the fixed
// LDS tree, so its summation order is a function of the system's atom count alone and a system's relaxation has the same
// bits alone, in any batch and on any shard.  The ring slot of a logical entry follows from the system's own counter and
// is computed on the device.
//
// The active set (adf_lbfgs_active_build): the list of the systems whose update mask is set, for a relaxation that leaves
// the converged ones out of the model forward; csrc/active.hip gathers and scatters over it.
#include <string.h>

#include <new>

#include "common.h"

#define LB_THREADS 256
#define LB_MAX_G 1024

struct adf_lbfgs {
    int64_t N, n;   // atoms, 3N
    int B, M;
    double maxstep, damping, H0;
    int early_stop_batch;
    int G;          // workgroups of the element kernels
    int64_t chunk;  // entries per workgroup
    double *s, *y;  // [M, n]
    double *rho, *alpha;  // [M]
    double *r0, *f0, *q, *dr;  // [n]
    double *part_a, *part_b, *part_rho;  // [G]
    double* sys_absmax;  // [B] max |dr| of the system
    int32_t* mask;       // [B] update mask of the last adf_lbfgs_converge
    int64_t total;       // entries appended since create / reset
    int64_t calls;       // adf_lbfgs_step calls since create / reset
    int per_system;      // every system keeps its own history and decisions (lb_per_system_kernel)
    double *rho_ps, *alpha_ps;  // [B, M], per-system mode
    int32_t* steps;             // [B] steps a system attempted (its own iteration number), per-system mode
    int32_t* prev_mask;         // [B] the mask the last adf_lbfgs_active_build saw (allocated by the first build)
    int converged;              // adf_lbfgs_converge has run since create / reset
    int built;                  // adf_lbfgs_active_build has run since create / reset
    adf_pool mem;        // owns every device buffer above
};

extern "C" int32_t adf_lbfgs_destroy(adf_lbfgs_t h) {
    delete h;
    return ADF_OK;
}

extern "C" int32_t adf_lbfgs_create(int64_t num_atoms, int32_t num_systems, int32_t memory, double maxstep,
                                    double damping, double alpha, int32_t early_stop_batch, adf_lbfgs_t* out) {
    if (!out) { adf_set_error("null argument"); return ADF_EINVAL; }
    *out = nullptr;
    if (num_atoms <= 0 || num_systems <= 0 || memory < 1 || !(alpha != 0.0)) {
        adf_set_error("lbfgs: num_atoms, num_systems and memory must be positive and alpha non-zero");
        return ADF_EINVAL;
    }
    if (3 * num_atoms > (int64_t)1 << 40 || (int64_t)memory * 3 * num_atoms > ((int64_t)1 << 40)) {
        adf_set_error("lbfgs: history of %lld entries too large", (long long)memory * 3 * num_atoms);
        return ADF_EINVAL;
    }
    adf_lbfgs* h = new (std::nothrow) adf_lbfgs();
    if (!h) { adf_set_error("host allocation failed"); return ADF_EOOM; }
    h->N = num_atoms; h->n = 3 * num_atoms; h->B = num_systems; h->M = memory;
    h->maxstep = maxstep; h->damping = damping; h->H0 = 1.0 / alpha; h->early_stop_batch = early_stop_batch != 0;
    // about 4 entries per thread, at most LB_MAX_G workgroups
    int64_t g = (h->n + 4 * LB_THREADS - 1) / (4 * LB_THREADS);
    h->G = (int)(g < 1 ? 1 : (g > LB_MAX_G ? LB_MAX_G : g));
    h->chunk = (h->n + h->G - 1) / h->G;
    const size_t n = (size_t)h->n, M = (size_t)memory;
    int32_t st = ADF_OK;
#define LB_ALLOC(field, count) if (st == ADF_OK) st = h->mem.alloc(&h->field, (count))
    LB_ALLOC(s, M * n);
    LB_ALLOC(y, M * n);
    LB_ALLOC(rho, M);
    LB_ALLOC(alpha, M);
    LB_ALLOC(r0, n);
    LB_ALLOC(f0, n);
    LB_ALLOC(q, n);
    LB_ALLOC(dr, n);
    LB_ALLOC(part_a, LB_MAX_G);
    LB_ALLOC(part_b, LB_MAX_G);
    LB_ALLOC(part_rho, LB_MAX_G);
    LB_ALLOC(sys_absmax, (size_t)num_systems);
    LB_ALLOC(mask, (size_t)num_systems);
#undef LB_ALLOC
    if (st == ADF_OK && hipMemset(h->r0, 0, n * sizeof(double)) != hipSuccess) st = ADF_EHIP;
    if (st == ADF_OK && hipMemset(h->f0, 0, n * sizeof(double)) != hipSuccess) st = ADF_EHIP;
    if (st == ADF_OK && hipMemset(h->mask, 0, (size_t)num_systems * sizeof(int32_t)) != hipSuccess) st = ADF_EHIP;
    if (st != ADF_OK) { adf_lbfgs_destroy(h); return st; }
    *out = h;
    return ADF_OK;
}

// A new run on the same batch shape: history, r0 / f0 and the update mask back to the state of a fresh handle.
extern "C" int32_t adf_lbfgs_reset(adf_lbfgs_t h, void* stream) {
    if (!h) { adf_set_error("null handle"); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)h->n;
    ADF_HIP_CHECK(hipMemsetAsync(h->r0, 0, n * sizeof(double), s));
    ADF_HIP_CHECK(hipMemsetAsync(h->f0, 0, n * sizeof(double), s));
    ADF_HIP_CHECK(hipMemsetAsync(h->mask, 0, (size_t)h->B * sizeof(int32_t), s));
    if (h->steps) {
        ADF_HIP_CHECK(hipMemsetAsync(h->steps, 0, (size_t)h->B * sizeof(int32_t), s));
        ADF_HIP_CHECK(hipMemsetAsync(h->sys_absmax, 0, (size_t)h->B * sizeof(double), s));
    }
    h->total = 0;
    h->calls = 0;
    h->converged = 0;
    h->built = 0;
    return ADF_OK;
}

// Per-system mode on / off, on a handle that has not stepped since create / reset.
extern "C" int32_t adf_lbfgs_set_per_system(adf_lbfgs_t h, int32_t on) {
    if (!h) { adf_set_error("null handle"); return ADF_EINVAL; }
    if (h->calls != 0) {
        adf_set_error("lbfgs_set_per_system: the handle has stepped %lld times (fresh or reset handles only)",
                      (long long)h->calls);
        return ADF_EINVAL;
    }
    if (on && h->early_stop_batch) {
        adf_set_error("lbfgs_set_per_system: early_stop_batch moves converged systems while others run, so a system alone "
                      "and in a batch would differ; the two cannot be combined");
        return ADF_EINVAL;
    }
    if (on && !h->steps) {
        const size_t B = (size_t)h->B, M = (size_t)h->M;
        int32_t st = h->mem.alloc(&h->rho_ps, B * M);
        if (st == ADF_OK) st = h->mem.alloc(&h->alpha_ps, B * M);
        if (st == ADF_OK) st = h->mem.alloc(&h->steps, B);
        if (st == ADF_OK && hipMemset(h->steps, 0, B * sizeof(int32_t)) != hipSuccess) st = ADF_EHIP;
        if (st == ADF_OK && hipMemset(h->sys_absmax, 0, B * sizeof(double)) != hipSuccess) st = ADF_EHIP;
        if (st != ADF_OK) return st;
    }
    h->per_system = on != 0;
    return ADF_OK;
}

// ---------------------------------------------------------------------------------------------------------- reductions
// Fixed-order block sum of one value per thread (LB_THREADS threads); the result is returned to every thread.
__device__ __forceinline__ double lb_block_sum(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int w = LB_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) red[t] = __dadd_rn(red[t], red[t + w]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// max that propagates NaN, like torch's max / amax reductions (fmax would drop it): a NaN force then gives the reference's
// decisions - the system's mask is clear (NaN >= fmax is false) and the step is not skipped (NaN < 1e-7 is false)
__device__ __forceinline__ double lb_max(double a, double b) { return (a != a || b != b) ? __longlong_as_double(0x7ff8000000000000ll) : fmax(a, b); }

__device__ __forceinline__ double lb_block_max(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int w = LB_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) red[t] = lb_max(red[t], red[t + w]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// sum of the G partials of the previous launch: the same order in every workgroup
__device__ __forceinline__ double lb_finish(const double* __restrict__ part, int G, double* red) {
    double a = 0.0;
    for (int i = threadIdx.x; i < G; i += LB_THREADS) a = __dadd_rn(a, part[i]);
    return lb_block_sum(a, red);
}

// ----------------------------------------------------------------------------------------------------------- kernels
// Start of a step: r = f64(pos); with append, s_new = r - r0 and y_new = -(f - f0) go to the ring slot and the partials of
// dot(y_new, s_new) to part_rho; q = -f.  loopmax > 0: partials of dot(s[loopmax-1], q) to part_out; loopmax == 0: z = H0 q.
__global__ __launch_bounds__(LB_THREADS) void lb_prep_kernel(const float* __restrict__ pos, const float* __restrict__ f,
                                                             const double* __restrict__ r0, const double* __restrict__ f0,
                                                             double* s_new, double* __restrict__ y_new,
                                                             const double* s_first, double* __restrict__ q,
                                                             double H0, int64_t n, int64_t chunk,
                                                             double* __restrict__ part_rho, double* __restrict__ part_out) {
    __shared__ double red[LB_THREADS];
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    double acc_rho = 0.0, acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += LB_THREADS) {
        const double fd = (double)f[i];
        const double qv = -fd;
        double sv = 0.0;
        if (s_new) {
            const double r = (double)pos[i];
            sv = __dsub_rn(r, r0[i]);
            const double yv = -__dsub_rn(fd, f0[i]);
            s_new[i] = sv;
            y_new[i] = yv;
            acc_rho = __dadd_rn(acc_rho, __dmul_rn(yv, sv));
        }
        if (s_first) {
            const double sf = s_first == s_new ? sv : s_first[i];
            acc = __dadd_rn(acc, __dmul_rn(sf, qv));
            q[i] = qv;
        } else {
            q[i] = __dmul_rn(H0, qv);
        }
    }
    if (s_new) {
        const double r = lb_block_sum(acc_rho, red);
        if (threadIdx.x == 0) part_rho[blockIdx.x] = r;
    }
    if (s_first) {
        const double r = lb_block_sum(acc, red);
        if (threadIdx.x == 0) part_out[blockIdx.x] = r;
    }
}

// First loop, entry i (descending): alpha_i = rho_i * dot(s_i, q) from part_in; q -= alpha_i * y_i; then the partials of
// dot(s_{i-1}, q), or (i == 0) z = H0 * q and the partials of dot(y_0, z).  new_rho: entry i is the one appended by this step,
// its rho = 1 / dot(y, s) is finished from part_rho and stored by workgroup 0.
__global__ __launch_bounds__(LB_THREADS) void lb_loop1_kernel(const double* __restrict__ part_in, const double* __restrict__ part_rho,
                                                              int new_rho, double* __restrict__ rho_slot,
                                                              double* __restrict__ alpha_i, const double* __restrict__ y_i,
                                                              const double* __restrict__ next, int last, double H0,
                                                              double* __restrict__ q, int64_t n, int64_t chunk, int G,
                                                              double* __restrict__ part_out) {
    __shared__ double red[LB_THREADS];
    double rho;
    if (new_rho) rho = __ddiv_rn(1.0, lb_finish(part_rho, G, red));
    else rho = *rho_slot;
    const double a = __dmul_rn(rho, lb_finish(part_in, G, red));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (new_rho) *rho_slot = rho;
        *alpha_i = a;
    }
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    double acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += LB_THREADS) {
        double qv = __dsub_rn(q[i], __dmul_rn(a, y_i[i]));
        if (last) qv = __dmul_rn(H0, qv);
        q[i] = qv;
        acc = __dadd_rn(acc, __dmul_rn(next[i], qv));
    }
    const double r = lb_block_sum(acc, red);
    if (threadIdx.x == 0) part_out[blockIdx.x] = r;
}

// Second loop, entry i (ascending): beta = rho_i * dot(y_i, z) from part_in; z += s_i * (alpha_i - beta); partials of
// dot(y_{i+1}, z) unless next == null.
__global__ __launch_bounds__(LB_THREADS) void lb_loop2_kernel(const double* __restrict__ part_in, const double* __restrict__ rho_slot,
                                                              const double* __restrict__ alpha_i, const double* __restrict__ s_i,
                                                              const double* __restrict__ next, double* __restrict__ z,
                                                              int64_t n, int64_t chunk, int G, double* __restrict__ part_out) {
    __shared__ double red[LB_THREADS];
    const double beta = __dmul_rn(*rho_slot, lb_finish(part_in, G, red));
    const double c = __dsub_rn(*alpha_i, beta);
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    double acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += LB_THREADS) {
        const double zv = __dadd_rn(z[i], __dmul_rn(s_i[i], c));
        z[i] = zv;
        if (next) acc = __dadd_rn(acc, __dmul_rn(next[i], zv));
    }
    if (next) {
        const double r = lb_block_sum(acc, red);
        if (threadIdx.x == 0) part_out[blockIdx.x] = r;
    }
}

// determine_step, one workgroup per system: p = -z; longest = max_atoms |p_atom|; dr = p * (1 / (longest + 1e-7) *
// min(longest, maxstep)) * damping; sys_absmax = max |dr|.
__global__ __launch_bounds__(LB_THREADS) void lb_step_kernel(const int32_t* __restrict__ atom_offset, const double* __restrict__ z,
                                                             double maxstep, double damping, double* __restrict__ dr,
                                                             double* __restrict__ sys_absmax) {
    __shared__ double red[LB_THREADS];
    const int b = blockIdx.x;
    const int a0 = atom_offset[b], a1 = atom_offset[b + 1];
    double m = 0.0;
    for (int a = a0 + threadIdx.x; a < a1; a += LB_THREADS) {
        const double px = -z[3 * (int64_t)a], py = -z[3 * (int64_t)a + 1], pz = -z[3 * (int64_t)a + 2];
        const double l = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(px, px), __dmul_rn(py, py)), __dmul_rn(pz, pz)));
        m = lb_max(m, l);
    }
    const double longest = lb_block_max(m, red);
    const double scale = __dmul_rn(__ddiv_rn(1.0, __dadd_rn(longest, 1e-7)), fmin(longest, maxstep));
    double am = 0.0;
    for (int64_t i = 3 * (int64_t)a0 + threadIdx.x; i < 3 * (int64_t)a1; i += LB_THREADS) {
        const double d = __dmul_rn(__dmul_rn(-z[i], scale), damping);
        dr[i] = d;
        am = lb_max(am, fabs(d));
    }
    const double r = lb_block_max(am, red);
    if (threadIdx.x == 0) sys_absmax[b] = r;
}

// set_positions, one workgroup per system, unless the step is skipped (max |dr| over the whole batch < 1e-7): then
// nothing is written and r0 / f0 stay.  pos += f32(dr) where the system's mask is set (every system with early_stop_batch);
// r0 = f64(old pos), f0 = f64(f).
__global__ __launch_bounds__(LB_THREADS) void lb_apply_kernel(const int32_t* __restrict__ atom_offset, int B,
                                                              const double* __restrict__ sys_absmax,
                                                              const int32_t* __restrict__ mask, int early,
                                                              const double* __restrict__ dr, const float* __restrict__ f,
                                                              float* __restrict__ pos, double* __restrict__ r0,
                                                              double* __restrict__ f0) {
    __shared__ double red[LB_THREADS];
    double m = 0.0;
    for (int i = threadIdx.x; i < B; i += LB_THREADS) m = lb_max(m, sys_absmax[i]);
    if (lb_block_max(m, red) < 1e-7) return;
    const int b = blockIdx.x;
    const bool on = early || mask[b] != 0;
    const int64_t lo = 3 * (int64_t)atom_offset[b], hi = 3 * (int64_t)atom_offset[b + 1];
    for (int64_t i = lo + threadIdx.x; i < hi; i += LB_THREADS) {
        const float p = pos[i];
        r0[i] = (double)p;
        f0[i] = (double)f[i];
        pos[i] = __fadd_rn(p, on ? (float)dr[i] : 0.0f);
    }
}

// One whole step of the per-system mode; workgroup b walks system b (elements lo .. lo + nb of the flattened batch).
//   mask clear: nothing is touched (last_absmax[b] = -1: no step attempted).
//   mask set, t = steps[b]: (1) t > 0: s = r - r0, y = -(f - f0) into ring slot (t - 1) % M, rho = 1 / dot(y, s);
//   (2) two loops over L = min(M, t) entries, logical entry i in slot (t - L + i) % M; (3) determine_step; (4) the skip of
//   a step whose max |dr| over THIS system is below 1e-7 (NaN does not skip); (5) pos += f32(dr), r0 = r, f0 = f unless
//   skipped; steps[b] = t + 1 either way.
// Thread t reads and writes only its own elements t, t + LB_THREADS, ... of q / z up to determine_step, which reads whole
// atoms after a barrier.  alpha is written by thread 0 and read by every thread after the barriers of the next reduction.
__global__ __launch_bounds__(LB_THREADS) void lb_per_system_kernel(const int32_t* __restrict__ atom_offset,
                                                                   const int32_t* __restrict__ mask, int32_t* steps,
                                                                   float* pos, const float* __restrict__ f, double* r0,
                                                                   double* f0, double* s, double* y, double* rho,
                                                                   double* alpha, double* q, int64_t n, int M, double H0,
                                                                   double maxstep, double damping, double* last_absmax) {
    __shared__ double red[LB_THREADS];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    if (mask[b] == 0) {
        if (tid == 0) last_absmax[b] = -1.0;
        return;
    }
    const int a0 = atom_offset[b], a1 = atom_offset[b + 1];
    const int64_t lo = 3 * (int64_t)a0;
    const int nb = 3 * (a1 - a0);
    const int t = steps[b];
    const int L = t < M ? t : M;
    pos += lo; f += lo; r0 += lo; f0 += lo; q += lo;
    s += lo; y += lo;
    rho += (size_t)b * M;
    alpha += (size_t)b * M;
    // ring slot of logical deque entry i (0 = oldest kept) and the offset of that entry in the rings
    auto slot = [&](int i) -> int { return (t - L + i) % M; };
    auto entry = [&](int i) -> size_t { return (size_t)slot(i) * (size_t)n; };

    // (1) history append and rho; q = -f, with the partial of dot(s[L-1], q), or z = H0 q without a history
    double rho_new = 0.0, acc = 0.0;
    if (t > 0) {
        double* s_new = s + entry(L - 1);
        double* y_new = y + entry(L - 1);
        double acc_rho = 0.0;
        for (int i = tid; i < nb; i += LB_THREADS) {
            const double fd = (double)f[i];
            const double qv = -fd;
            const double sv = __dsub_rn((double)pos[i], r0[i]);
            const double yv = -__dsub_rn(fd, f0[i]);
            s_new[i] = sv;
            y_new[i] = yv;
            acc_rho = __dadd_rn(acc_rho, __dmul_rn(yv, sv));
            acc = __dadd_rn(acc, __dmul_rn(sv, qv));
            q[i] = qv;
        }
        rho_new = __ddiv_rn(1.0, lb_block_sum(acc_rho, red));
        if (tid == 0) rho[slot(L - 1)] = rho_new;
    } else {
        for (int i = tid; i < nb; i += LB_THREADS) q[i] = __dmul_rn(H0, -(double)f[i]);
    }

    // (2) first loop, descending: alpha_i = rho_i dot(s_i, q); q -= alpha_i y_i; the last entry leaves z = H0 q
    for (int i = L - 1; i >= 0; --i) {
        const double rho_i = i == L - 1 ? rho_new : rho[slot(i)];
        const double a = __dmul_rn(rho_i, lb_block_sum(acc, red));
        if (tid == 0) alpha[i] = a;
        const double* y_i = y + entry(i);
        const double* next = i > 0 ? s + entry(i - 1) : y + entry(0);
        acc = 0.0;
        for (int j = tid; j < nb; j += LB_THREADS) {
            double qv = __dsub_rn(q[j], __dmul_rn(a, y_i[j]));
            if (i == 0) qv = __dmul_rn(H0, qv);
            q[j] = qv;
            acc = __dadd_rn(acc, __dmul_rn(next[j], qv));
        }
    }
    // second loop, ascending: beta = rho_i dot(y_i, z); z += s_i (alpha_i - beta)
    for (int i = 0; i < L; ++i) {
        const double rho_i = i == L - 1 ? rho_new : rho[slot(i)];
        const double beta = __dmul_rn(rho_i, lb_block_sum(acc, red));
        const double c = __dsub_rn(alpha[i], beta);
        const double* s_i = s + entry(i);
        const double* next = i + 1 < L ? y + entry(i + 1) : nullptr;
        acc = 0.0;
        for (int j = tid; j < nb; j += LB_THREADS) {
            const double zv = __dadd_rn(q[j], __dmul_rn(s_i[j], c));
            q[j] = zv;
            if (next) acc = __dadd_rn(acc, __dmul_rn(next[j], zv));
        }
    }
    __syncthreads();   // z is complete: determine_step reads whole atoms

    // (3) determine_step
    double m = 0.0;
    for (int a = tid; a < a1 - a0; a += LB_THREADS) {
        const double px = -q[3 * a], py = -q[3 * a + 1], pz = -q[3 * a + 2];
        const double l = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(px, px), __dmul_rn(py, py)), __dmul_rn(pz, pz)));
        m = lb_max(m, l);
    }
    const double longest = lb_block_max(m, red);
    const double scale = __dmul_rn(__ddiv_rn(1.0, __dadd_rn(longest, 1e-7)), fmin(longest, maxstep));
    double am = 0.0;
    for (int i = tid; i < nb; i += LB_THREADS) am = lb_max(am, fabs(__dmul_rn(__dmul_rn(-q[i], scale), damping)));
    // (4) the system's own skip decision
    const double absmax = lb_block_max(am, red);
    // (5) masked update
    if (!(absmax < 1e-7)) {
        for (int i = tid; i < nb; i += LB_THREADS) {
            const float p = pos[i];
            r0[i] = (double)p;
            f0[i] = (double)f[i];
            pos[i] = __fadd_rn(p, (float)__dmul_rn(__dmul_rn(-q[i], scale), damping));
        }
    }
    if (tid == 0) {
        steps[b] = t + 1;
        last_absmax[b] = absmax;
    }
}

// check_convergence: max over the system's atoms of sqrt(fx^2 + fy^2 + fz^2) in f64; mask = max >= fmax
__global__ __launch_bounds__(LB_THREADS) void lb_converge_kernel(const int32_t* __restrict__ atom_offset, const float* __restrict__ f,
                                                                 double fmax_, double* __restrict__ max_force,
                                                                 int32_t* __restrict__ mask) {
    __shared__ double red[LB_THREADS];
    const int b = blockIdx.x;
    const int a0 = atom_offset[b], a1 = atom_offset[b + 1];
    double m = 0.0;
    for (int a = a0 + threadIdx.x; a < a1; a += LB_THREADS) {
        const double fx = f[3 * (int64_t)a], fy = f[3 * (int64_t)a + 1], fz = f[3 * (int64_t)a + 2];
        m = lb_max(m, __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(fx, fx), __dmul_rn(fy, fy)), __dmul_rn(fz, fz))));
    }
    const double r = lb_block_max(m, red);
    if (threadIdx.x == 0) {
        if (max_force) max_force[b] = r;
        mask[b] = r >= fmax_ ? 1 : 0;
    }
}

__global__ __launch_bounds__(LB_THREADS) void lb_all_converged_kernel(const int32_t* __restrict__ mask, int B,
                                                                      int32_t* __restrict__ out) {
    __shared__ double red[LB_THREADS];
    double any = 0.0;
    for (int i = threadIdx.x; i < B; i += LB_THREADS) any = fmax(any, mask[i] ? 1.0 : 0.0);
    const double r = lb_block_max(any, red);
    if (threadIdx.x == 0) *out = r == 0.0 ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ entries
extern "C" int32_t adf_lbfgs_converge(adf_lbfgs_t h, const int32_t* atom_offset, const float* forces, double fmax_,
                                      double* max_force, int32_t* all_converged, void* stream) {
    if (!h || !atom_offset || !forces) { adf_set_error("lbfgs_converge: null argument"); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lb_converge_kernel, dim3(h->B), dim3(LB_THREADS), 0, s, atom_offset, forces, fmax_, max_force,
                       h->mask);
    if (all_converged)
        hipLaunchKernelGGL(lb_all_converged_kernel, dim3(1), dim3(LB_THREADS), 0, s, h->mask, h->B, all_converged);
    ADF_HIP_CHECK(hipGetLastError());
    h->converged = 1;
    return ADF_OK;
}

// The active set of the last converge's mask, one workgroup.  The B systems are walked in chunks of LB_THREADS; inside a
// chunk an inclusive integer scan in LDS (count of set masks, sum of their atom counts) gives every set system its place
// k in the list and the first compact row of its atoms, and the totals of the chunks before it are carried in registers
// (the same value in every thread).  Integer sums in a fixed order, no atomics.  changed: any mask that differs from the
// one the previous build saw (the list is a function of the mask), or `first`.
__global__ __launch_bounds__(LB_THREADS) void lb_active_build_kernel(const int32_t* __restrict__ mask,
                                                                     int32_t* __restrict__ prev_mask,
                                                                     const int32_t* __restrict__ atom_offset, int B,
                                                                     int first, int32_t* __restrict__ act_sys,
                                                                     int32_t* __restrict__ act_offset,
                                                                     int32_t* __restrict__ info) {
    __shared__ int32_t sc[LB_THREADS], sa[LB_THREADS];
    const int t = threadIdx.x;
    int carry_c = 0, carry_a = 0, diff = first;
    for (int base = 0; base < B; base += LB_THREADS) {
        const int i = base + t;
        int flag = 0, n = 0;
        if (i < B) {
            flag = mask[i] != 0;
            if (flag) n = atom_offset[i + 1] - atom_offset[i];
            diff |= flag != (prev_mask[i] != 0);
            prev_mask[i] = flag;
        }
        sc[t] = flag;
        sa[t] = n;
        __syncthreads();
        for (int d = 1; d < LB_THREADS; d <<= 1) {
            const int vc = t >= d ? sc[t - d] : 0, va = t >= d ? sa[t - d] : 0;
            __syncthreads();
            sc[t] += vc;
            sa[t] += va;
            __syncthreads();
        }
        if (flag) {
            const int k = carry_c + sc[t] - 1;
            act_sys[k] = i;
            act_offset[k] = carry_a + sa[t] - n;
        }
        carry_c += sc[LB_THREADS - 1];
        carry_a += sa[LB_THREADS - 1];
        __syncthreads();   // the totals are read before the next chunk overwrites them
    }
    sc[t] = diff;
    __syncthreads();
    for (int w = LB_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) sc[t] |= sc[t + w];
        __syncthreads();
    }
    for (int k = carry_c + t; k <= B; k += LB_THREADS) {
        if (k < B) act_sys[k] = -1;
        act_offset[k] = carry_a;
    }
    if (t == 0) {
        info[0] = carry_c;
        info[1] = carry_a;
        info[2] = sc[0] != 0;
        info[3] = 0;
    }
}

extern "C" int32_t adf_lbfgs_active_build(adf_lbfgs_t h, const int32_t* atom_offset, int32_t* act_sys, int32_t* act_offset,
                                          int32_t* info, void* stream) {
    if (!h || !atom_offset || !act_sys || !act_offset || !info) {
        adf_set_error("lbfgs_active_build: null argument");
        return ADF_EINVAL;
    }
    if (!h->converged) {
        adf_set_error("lbfgs_active_build: no adf_lbfgs_converge since create / reset (the list is built from its mask)");
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    if (!h->prev_mask) {
        const int32_t st = h->mem.alloc(&h->prev_mask, (size_t)h->B);
        if (st != ADF_OK) return st;
    }
    // the first build after create / reset compares with nothing: an all-clear previous mask and changed forced to 1
    if (!h->built) ADF_HIP_CHECK(hipMemsetAsync(h->prev_mask, 0, (size_t)h->B * sizeof(int32_t), s));
    hipLaunchKernelGGL(lb_active_build_kernel, dim3(1), dim3(LB_THREADS), 0, s, h->mask, h->prev_mask, atom_offset, h->B,
                       h->built ? 0 : 1, act_sys, act_offset, info);
    ADF_HIP_CHECK(hipGetLastError());
    h->built = 1;
    return ADF_OK;
}

extern "C" int32_t adf_lbfgs_step(adf_lbfgs_t h, const int32_t* atom_offset, float* pos, const float* forces,
                                  int64_t iteration, void* stream) {
    if (!h || !atom_offset || !pos || !forces || iteration < 0) { adf_set_error("lbfgs_step: bad argument"); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const int M = h->M, G = h->G;
    const size_t n = (size_t)h->n;
    const bool append = iteration > 0;
    // the reference appends one entry per step from iteration 1 on, so iteration k > 0 follows exactly k - 1 appends
    // (repeating or skipping an iteration number would leave an entry without its rho)
    if (iteration != (append ? h->total + 1 : 0) || (!append && h->total != 0)) {
        adf_set_error("lbfgs_step: iteration %lld after %lld recorded steps (iterations run 0, 1, 2, ... from a fresh or "
                      "reset handle)", (long long)iteration, (long long)h->total);
        return ADF_EINVAL;
    }
    const int64_t total = h->total + (append ? 1 : 0);
    const int len = (int)(total < M ? total : M);
    const int L = (int)(iteration < M ? iteration : M);
    h->total = total;
    h->calls += 1;
    if (h->per_system) {
        hipLaunchKernelGGL(lb_per_system_kernel, dim3(h->B), dim3(LB_THREADS), 0, s, atom_offset, h->mask, h->steps, pos,
                           forces, h->r0, h->f0, h->s, h->y, h->rho_ps, h->alpha_ps, h->q, (int64_t)h->n, M, h->H0,
                           h->maxstep, h->damping, h->sys_absmax);
        ADF_HIP_CHECK(hipGetLastError());
        return ADF_OK;
    }
    // ring slot of logical deque entry i (0 = oldest kept)
    auto slot = [&](int i) -> int { return (int)((total - len + i) % M); };
    double* s_new = append ? h->s + (size_t)slot(len - 1) * n : nullptr;
    double* y_new = append ? h->y + (size_t)slot(len - 1) * n : nullptr;
    const int new_idx = append ? len - 1 : -1;  // logical index of the entry appended now
    const dim3 grid(G), blk(LB_THREADS);
    double* pin = h->part_a;
    double* pout = h->part_b;
    hipLaunchKernelGGL(lb_prep_kernel, grid, blk, 0, s, pos, forces, h->r0, h->f0, s_new, y_new,
                       L > 0 ? h->s + (size_t)slot(L - 1) * n : nullptr, h->q, h->H0, (int64_t)n, h->chunk, h->part_rho,
                       pin);
    for (int i = L - 1; i >= 0; --i) {
        const int si = slot(i);
        const double* next = i > 0 ? h->s + (size_t)slot(i - 1) * n : h->y + (size_t)slot(0) * n;
        hipLaunchKernelGGL(lb_loop1_kernel, grid, blk, 0, s, pin, h->part_rho, i == new_idx ? 1 : 0, h->rho + si,
                           h->alpha + i, h->y + (size_t)si * n, next, i == 0 ? 1 : 0, h->H0, h->q, (int64_t)n, h->chunk, G,
                           pout);
        double* t = pin; pin = pout; pout = t;
    }
    for (int i = 0; i < L; ++i) {
        const int si = slot(i);
        const double* next = i + 1 < L ? h->y + (size_t)slot(i + 1) * n : nullptr;
        hipLaunchKernelGGL(lb_loop2_kernel, grid, blk, 0, s, pin, h->rho + si, h->alpha + i, h->s + (size_t)si * n, next,
                           h->q, (int64_t)n, h->chunk, G, pout);
        double* t = pin; pin = pout; pout = t;
    }
    hipLaunchKernelGGL(lb_step_kernel, dim3(h->B), blk, 0, s, atom_offset, h->q, h->maxstep, h->damping, h->dr,
                       h->sys_absmax);
    hipLaunchKernelGGL(lb_apply_kernel, dim3(h->B), blk, 0, s, atom_offset, h->B, h->sys_absmax, h->mask,
                       h->early_stop_batch, h->dr, forces, pos, h->r0, h->f0);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}

// The update mask of the last adf_lbfgs_converge ([B] int32, device).
extern "C" int32_t adf_lbfgs_get_mask(adf_lbfgs_t h, int32_t* out, void* stream) {
    if (!h || !out) { adf_set_error("null argument"); return ADF_EINVAL; }
    ADF_HIP_CHECK(hipMemcpyAsync(out, h->mask, sizeof(int32_t) * h->B, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ADF_OK;
}

// The search direction z of the last adf_lbfgs_step ([3N] f64, device): q holds it after the second loop in both modes.
// The rows of a system whose mask was clear in a per-system step are the ones of its own last step (undefined before it).
extern "C" int32_t adf_lbfgs_get_direction(adf_lbfgs_t h, double* z_out, void* stream) {
    if (!h || !z_out) { adf_set_error("null argument"); return ADF_EINVAL; }
    if (h->calls == 0) {
        adf_set_error("lbfgs_get_direction: no adf_lbfgs_step since create / reset (there is no direction yet)");
        return ADF_EINVAL;
    }
    ADF_HIP_CHECK(hipMemcpyAsync(z_out, h->q, sizeof(double) * (size_t)h->n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ADF_OK;
}

// Per-system mode: the steps every system has attempted and the max |dr| of its last attempt (-1: the last
// adf_lbfgs_step did not attempt one); either output may be null.
extern "C" int32_t adf_lbfgs_get_step_state(adf_lbfgs_t h, int32_t* steps_taken, double* last_absmax, void* stream) {
    if (!h) { adf_set_error("null handle"); return ADF_EINVAL; }
    if (!h->per_system) { adf_set_error("lbfgs_get_step_state: the handle is not in per-system mode"); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    if (steps_taken)
        ADF_HIP_CHECK(hipMemcpyAsync(steps_taken, h->steps, sizeof(int32_t) * h->B, hipMemcpyDeviceToDevice, s));
    if (last_absmax)
        ADF_HIP_CHECK(hipMemcpyAsync(last_absmax, h->sys_absmax, sizeof(double) * h->B, hipMemcpyDeviceToDevice, s));
    return ADF_OK;
}

// max |dr| over the batch of the last adf_lbfgs_step (< 1e-7: the step was skipped); device scalar out.  Per-system mode:
// over the systems that attempted a step (the others hold -1, below the 0 the maximum starts from).
__global__ void lb_last_absmax_kernel(const double* __restrict__ sys_absmax, int B, double* out) {
    __shared__ double red[LB_THREADS];
    double m = 0.0;
    for (int i = threadIdx.x; i < B; i += LB_THREADS) m = lb_max(m, sys_absmax[i]);
    const double r = lb_block_max(m, red);
    if (threadIdx.x == 0) *out = r;
}

extern "C" int32_t adf_lbfgs_last_step_max(adf_lbfgs_t h, double* out, void* stream) {
    if (!h || !out) { adf_set_error("null argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(lb_last_absmax_kernel, dim3(1), dim3(LB_THREADS), 0, (hipStream_t)stream, h->sys_absmax, h->B, out);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}
