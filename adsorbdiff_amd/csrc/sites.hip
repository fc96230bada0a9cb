// Heuristic adsorption sites: the ontop, bridge and hollow candidates of every slab of a batch from its
// tag-1 atoms and its surface triangles, and their reduction - near-duplicates first, symmetry-equivalent sites second - to
// one representative each.  The contract of both entries is in include/adsorbdiff_hip.h.  The reference leaves this to
// pymatgen's AdsorbateSiteFinder on the host (placement/adsorbate_slab_config.py:113-116, 185-194).
//
// All arithmetic is float64 on float32 inputs (as placement.hip); a candidate is rounded to float32 once, when it is
// stored, and the reduction reads those float32 rows, so it computes the same on candidates it is handed from elsewhere.
// No float atomics; the integer atomics are the OR on the error word.  Every output has one writer per launch phase and
// is written with an ordinary vector store: two calls give the same bits.
//
// Mapping.  ss_offsets_kernel: one workgroup; a thread counts the tag-1 atoms of its slab and the workgroup scans the
// segment sizes (three per slab: ontop, bridge, hollow) into seg_offset.  ss_candidates_kernel: one workgroup per (slab,
// kind) segment, threads over its candidates; the ontop segment compacts the tag-1 atoms in atom order with a ballot
// prefix.  ss_reduce_kernel: one workgroup per segment and the round structure of uq_cluster_kernel (unique.hip): the
// unassigned candidate of least index becomes a representative (a workgroup minimum), its coordinates go through LDS to
// every thread, and every thread tests its own unassigned candidates against it - under each operation of the slab, which
// are staged in LDS SS_OP_TILE at a time and read at one address by all lanes (a broadcast).  A thread reads and writes the
// state words of its own candidates only.  Candidates (strided), representatives (one per round) and operations (tiled)
// are all looped: nothing is capped.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "host_util.h"
#include "cell3.h"
#include "lanes.h"

#define SS_THREADS 256
#define SS_OP_TILE 128      // operations staged in LDS at a time: 12 doubles each, 12 KiB
#define SS_COS_MIN 1e-5     // a corner whose cosine is not at least this makes the triangle "obtuse"

enum { SS_ERR_RANGE = 1, SS_ERR_CELL = 2 };

// M = [a b n] as columns (row-major here), n = a x b / |a x b|, and its inverse
struct ss_frame {
    double M[9], Mi[9];
    bool ok;
};

__device__ __forceinline__ void ss_load_frame(const float* __restrict__ cell, ss_frame& F) {
    double a[3], b[3], n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { a[k] = (double)cell[k]; b[k] = (double)cell[3 + k]; }
    adf_cross3(a, b, n);
    const double nn = sqrt(adf_dot3(n, n));
    F.ok = nn > 0.0 && nn < INFINITY;
    const double in = F.ok ? 1.0 / nn : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] *= in;
#pragma unroll
    for (int k = 0; k < 3; ++k) { F.M[3 * k] = a[k]; F.M[3 * k + 1] = b[k]; F.M[3 * k + 2] = n[k]; }
    // rows of the inverse: b x n, n x a, a x b over det = a . (b x n)
    double r0[3], r1[3], r2[3];
    adf_cross3(b, n, r0);
    adf_cross3(n, a, r1);
    adf_cross3(a, b, r2);
    const double det = adf_dot3(a, r0);
    const double id = F.ok && det != 0.0 ? 1.0 / det : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { F.Mi[k] = r0[k] * id; F.Mi[3 + k] = r1[k] * id; F.Mi[6 + k] = r2[k] * id; }
}

// |reduce(d)| of section 4j: in-plane fractional components minus their nearest integer, the normal component kept
__device__ __forceinline__ double ss_reduce_norm(const ss_frame& F, double dx, double dy, double dz) {
    double f0 = F.Mi[0] * dx + F.Mi[1] * dy + F.Mi[2] * dz;
    double f1 = F.Mi[3] * dx + F.Mi[4] * dy + F.Mi[5] * dz;
    const double f2 = F.Mi[6] * dx + F.Mi[7] * dy + F.Mi[8] * dz;
    f0 -= rint(f0);
    f1 -= rint(f1);
    const double x = F.M[0] * f0 + F.M[1] * f1 + F.M[2] * f2;
    const double y = F.M[3] * f0 + F.M[4] * f1 + F.M[5] * f2;
    const double z = F.M[6] * f0 + F.M[7] * f1 + F.M[8] * f2;
    return sqrt(x * x + y * y + z * z);
}

// f -> (f + eps) mod 1 - eps along a and b, the height kept; stored as float32
__device__ __forceinline__ void ss_store_inside(const ss_frame& F, const double (&x)[3], float* __restrict__ out) {
    double f[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) f[k] = F.Mi[3 * k] * x[0] + F.Mi[3 * k + 1] * x[1] + F.Mi[3 * k + 2] * x[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) f[k] = adf_mod1_eps(f[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (float)(F.M[3 * k] * f[0] + F.M[3 * k + 1] * f[1] + F.M[3 * k + 2] * f[2]);
}

// workgroup sum of an int, left in every thread; red: SS_THREADS / 64 words of LDS.  Kept beside lanes.h's adf_block_reduce:
// through it the combine of ss_reduce_kernel compiles to other instructions (tools/device_asm_diff.py)
__device__ __forceinline__ int ss_block_sum(int v, int* red) {
    v = adf_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int w = 1; w < SS_THREADS / 64; ++w) v += red[w];
    return v;
}

// ------------------------------------------------------------------------------------------------ segment offsets
__global__ __launch_bounds__(SS_THREADS) void ss_offsets_kernel(const int32_t* __restrict__ tags,
                                                                const int32_t* __restrict__ atom_offset,
                                                                const int32_t* __restrict__ tri_offset, int N, int T, int B,
                                                                int capacity, int32_t* __restrict__ seg_offset,
                                                                int32_t* err) {
    // on an error (reported through err) the offsets written are within [0, capacity] and otherwise meaningless
    __shared__ int red[SS_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0;
    bool bad = false;
    for (int base = 0; base < B; base += SS_THREADS) {
        const int b = base + tid;
        int top = 0, nt = 0;
        if (b < B) {
            const int a0 = atom_offset[b], a1 = atom_offset[b + 1], t0 = tri_offset[b], t1 = tri_offset[b + 1];
            if (a0 < 0 || a1 < a0 || a1 > N || t0 < 0 || t1 < t0 || t1 > T) {
                bad = true;
            } else {
                for (int i = a0; i < a1; ++i) top += tags[i] == 1 ? 1 : 0;
                nt = t1 - t0;
            }
        }
        const long long total = (long long)top + 4ll * nt;
        // exclusive scan of `total` over the workgroup (every total and their sum fit an int: N + 4 T does, checked on the host)
        int incl = (int)total;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        __syncthreads();                                // the previous round's reads of red are done
        if (lane == 63) red[wave] = incl;
        __syncthreads();
        long long before = carry, all = 0;
#pragma unroll
        for (int w = 0; w < SS_THREADS / 64; ++w) {
            if (w < wave) before += red[w];
            all += red[w];
        }
        const long long start = before + incl - total;
        if (b < B) {
            if (start + total > capacity) {
                bad = true;                             // the tables are too small: the slab's segments stay empty
                seg_offset[3 * b] = seg_offset[3 * b + 1] = seg_offset[3 * b + 2] = (int32_t)min(start, (long long)capacity);
            } else {
                seg_offset[3 * b] = (int32_t)start;
                seg_offset[3 * b + 1] = (int32_t)(start + top);
                seg_offset[3 * b + 2] = (int32_t)(start + top + 3ll * nt);
            }
        }
        carry += all;
    }
    if (tid == 0) seg_offset[3 * B] = (int32_t)min(carry, (long long)capacity);
    if (bad) atomicOr(err, SS_ERR_RANGE);
}

// ------------------------------------------------------------------------------------------------ candidates
__global__ __launch_bounds__(SS_THREADS) void ss_candidates_kernel(
    const float* __restrict__ pos, const int32_t* __restrict__ tags, const int32_t* __restrict__ atom_offset,
    const float* __restrict__ cell, const float* __restrict__ tri, const int32_t* __restrict__ tri_offset,
    const int32_t* __restrict__ seg_offset, int N, int T, int capacity, float* __restrict__ cand,
    int32_t* __restrict__ valid, int32_t* err) {
    __shared__ int red[SS_THREADS / 64];
    const int b = blockIdx.x, kind = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((*err & SS_ERR_RANGE) != 0) return;             // ss_offsets_kernel refused an offset: no candidate is written
    const int s0 = seg_offset[3 * b + kind], s1 = seg_offset[3 * b + kind + 1];
    const int a0 = atom_offset[b], a1 = atom_offset[b + 1], t0 = tri_offset[b], t1 = tri_offset[b + 1];
    if (s0 < 0 || s1 <= s0 || s1 > capacity || a0 < 0 || a1 < a0 || a1 > N || t0 < 0 || t1 < t0 || t1 > T) return;
    ss_frame F;
    ss_load_frame(cell + 9 * (size_t)b, F);
    if (!F.ok) {
        if (tid == 0) atomicOr(err, SS_ERR_CELL);
        return;
    }
    const int n = s1 - s0;
    if (kind == 0) {
        // the k-th tag-1 atom, in atom order, is candidate k
        int running = 0;
        for (int base = a0; base < a1; base += SS_THREADS) {
            const int i = base + tid;
            const bool mine = i < a1 && tags[i] == 1;
            const unsigned long long m = __ballot(mine);
            __syncthreads();                            // the previous round's reads of red are done
            if (lane == 0) red[wave] = __popcll(m);
            __syncthreads();
            int before = running, all = 0;
#pragma unroll
            for (int w = 0; w < SS_THREADS / 64; ++w) {
                if (w < wave) before += red[w];
                all += red[w];
            }
            const int slot = before + __popcll(m & ((1ull << lane) - 1ull));
            if (mine && slot < n) {
                const double x[3] = {(double)pos[3 * (size_t)i], (double)pos[3 * (size_t)i + 1], (double)pos[3 * (size_t)i + 2]};
                ss_store_inside(F, x, cand + 3 * (size_t)(s0 + slot));
                valid[s0 + slot] = 1;
            }
            running += all;
        }
        return;
    }
    const int nt = t1 - t0;
    if (kind == 1) {
        // edge e of triangle t: the one opposite corner e, so (v1,v2), (v0,v2), (v0,v1)
        for (int c = tid; c < n && c < 3 * nt; c += SS_THREADS) {
            const int t = c / 3, e = c - 3 * t;
            const float* v = tri + 9 * (size_t)(t0 + t);
            const int i1 = e == 0 ? 1 : 0, i2 = e == 2 ? 1 : 2;
            double x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = 0.5 * ((double)v[3 * i1 + k] + (double)v[3 * i2 + k]);
            ss_store_inside(F, x, cand + 3 * (size_t)(s0 + c));
            valid[s0 + c] = 1;
        }
        return;
    }
    for (int c = tid; c < n && c < nt; c += SS_THREADS) {
        const float* vf = tri + 9 * (size_t)(t0 + c);
        double v[9], x[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) v[k] = (double)vf[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = (v[k] + v[3 + k] + v[6 + k]) / 3.0;
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int j = (i + 1) % 3, l = (i + 2) % 3;
            double e1[3], e2[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { e1[k] = v[3 * j + k] - v[3 * i + k]; e2[k] = v[3 * l + k] - v[3 * i + k]; }
            const double n1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
            const double n2 = sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
            const double cs = (e1[0] / n1) * (e2[0] / n2) + (e1[1] / n1) * (e2[1] / n2) + (e1[2] / n1) * (e2[2] / n2);
            ok = ok && cs >= SS_COS_MIN;                // NaN (an edge of no length) is not >=: invalid
        }
        ss_store_inside(F, x, cand + 3 * (size_t)(s0 + c));
        valid[s0 + c] = ok ? 1 : 0;
    }
}

static const adf_errrow SS_ERRORS[] = {
    {SS_ERR_RANGE, ADF_EINVAL, "%s: malformed offsets (not ascending, outside their arrays, a slab or operation index out of range, or "
                               "more candidates than the tables hold)"},
    {SS_ERR_CELL, ADF_EINVAL, "%s: the first two rows of a cell span no finite area"}};

extern "C" int32_t adf_surface_site_candidates(const float* pos, const int32_t* tags, const int32_t* atom_offset,
                                               const float* cell, const float* tri, const int32_t* tri_offset,
                                               int32_t num_atoms, int32_t num_triangles, int32_t num_slabs,
                                               int32_t capacity, int32_t* seg_offset, float* cand, int32_t* valid,
                                               void* stream) {
    if (!pos || !tags || !atom_offset || !cell || !tri || !tri_offset || !seg_offset || !cand || !valid) {
        adf_set_error("surface_site_candidates: null argument");
        return ADF_EINVAL;
    }
    if (num_atoms < 0 || num_triangles < 0 || num_slabs <= 0 || capacity < 0 ||
        (long long)num_atoms + 4ll * num_triangles > (long long)INT_MAX) {
        adf_set_error("surface_site_candidates: %d atoms, %d triangles, %d slabs, tables of %d rows", num_atoms, num_triangles,
                      num_slabs, capacity);
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    adf_errword err;   // freed on every return (after the synchronisation in finish)
    ADF_TRY(err.create(s));
    hipLaunchKernelGGL(ss_offsets_kernel, dim3(1), dim3(SS_THREADS), 0, s, tags, atom_offset, tri_offset, num_atoms,
                       num_triangles, num_slabs, capacity, seg_offset, err.dev);
    ADF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ss_candidates_kernel, dim3(num_slabs, 3), dim3(SS_THREADS), 0, s, pos, tags, atom_offset, cell, tri,
                       tri_offset, seg_offset, num_atoms, num_triangles, capacity, cand, valid, err.dev);
    ADF_HIP_CHECK(hipGetLastError());
    return err.finish(s, "surface_site_candidates", SS_ERRORS);
}

// ------------------------------------------------------------------------------------------------ reduction
struct ss_reduce_params {
    const float* cand; const int32_t* valid; const int32_t* seg_offset; const int32_t* seg_slab; const float* cell;
    const int32_t* op_offset; const double* rot; const double* trans;
    int32_t C, G, B, K;
    double tol;
    int32_t* first; int32_t* rep; int32_t* mult; int32_t* counts; int32_t* err;
};

// The greedy pass over the candidates whose state word is -2, in rounds; returns the representatives made.  OPS: the
// distance is the minimum over the operations o0 .. o0 + nops (else the identity alone); mult: receives, per
// representative, the candidates that joined it (itself included), or null.
template <bool OPS>
__device__ __forceinline__ int ss_rounds(const ss_reduce_params& q, const ss_frame& F, int s0, int n, int32_t* state,
                                         int32_t* mult, int o0, int nops, double* ops, double* rx, int* red) {
    const int tid = threadIdx.x;
    int staged = -1, count = 0;
    for (;;) {
        int key = INT_MAX;
        for (int c = tid; c < n; c += SS_THREADS)
            if (state[s0 + c] == -2) { key = c; break; }
        key = adf_block_min<SS_THREADS / 64>(key, red);
        if (key == INT_MAX) break;
        const int r = key;
        if (tid < 3) rx[tid] = (double)q.cand[3 * (size_t)(s0 + r) + tid];
        __syncthreads();
        const double xr = rx[0], yr = rx[1], zr = rx[2];    // one address in every lane: a broadcast
        int joined = 0;
        if (!OPS) {
            for (int c = tid; c < n; c += SS_THREADS) {
                if (state[s0 + c] != -2) continue;
                bool join = c == r;
                if (!join) {
                    const float* p = q.cand + 3 * (size_t)(s0 + c);
                    join = ss_reduce_norm(F, (double)p[0] - xr, (double)p[1] - yr, (double)p[2] - zr) <= q.tol;
                }
                if (join) { state[s0 + c] = s0 + r; ++joined; }
            }
        } else {
            for (int k0 = 0; k0 < nops; k0 += SS_OP_TILE) {
                const int kn = min(SS_OP_TILE, nops - k0);
                if (staged != k0) {                          // (with one tile the operations are staged once for all rounds)
                    __syncthreads();                         // the reads of the tile in place are done
                    for (int e = tid; e < 12 * kn; e += SS_THREADS) {
                        const int k = e / 12, j = e - 12 * k;
                        const size_t o = (size_t)(o0 + k0 + k);
                        ops[e] = j < 9 ? q.rot[9 * o + j] : q.trans[3 * o + (j - 9)];
                    }
                    __syncthreads();
                    staged = k0;
                }
                for (int c = tid; c < n; c += SS_THREADS) {
                    if (state[s0 + c] != -2) continue;
                    bool join = c == r;
                    const float* p = q.cand + 3 * (size_t)(s0 + c);
                    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
                    for (int k = 0; k < kn && !join; ++k) {
                        const double* R = ops + 12 * k;
                        const double ix = R[0] * x + R[1] * y + R[2] * z + R[9];
                        const double iy = R[3] * x + R[4] * y + R[5] * z + R[10];
                        const double iz = R[6] * x + R[7] * y + R[8] * z + R[11];
                        join = ss_reduce_norm(F, ix - xr, iy - yr, iz - zr) <= q.tol;
                    }
                    if (join) { state[s0 + c] = s0 + r; ++joined; }
                }
            }
        }
        if (mult) {
            joined = ss_block_sum(joined, red);
            if (tid == 0) mult[s0 + r] = joined;
        }
        ++count;
    }
    return count;
}

__global__ __launch_bounds__(SS_THREADS) void ss_reduce_kernel(ss_reduce_params q) {
    __shared__ double ops[12 * SS_OP_TILE];
    __shared__ double rx[3];
    __shared__ int red[SS_THREADS / 64];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int s0 = q.seg_offset[g], s1 = q.seg_offset[g + 1];
    const int b = q.seg_slab ? q.seg_slab[g] : g;
    bool bad = s0 < 0 || s1 < s0 || s1 > q.C || b < 0 || b >= q.B;
    int o0 = 0, nops = 1;
    if (!bad && q.op_offset) {
        o0 = q.op_offset[b];
        const long long end = q.op_offset[b + 1];
        bad = o0 < 0 || end <= o0 || end > q.K;
        nops = (int)(end - o0);
    }
    if (bad) {                                               // nothing of the segment is read or written
        if (tid == 0) { atomicOr(q.err, SS_ERR_RANGE); q.counts[2 * g] = 0; q.counts[2 * g + 1] = 0; }
        return;
    }
    const int n = s1 - s0;
    if (n == 0) {
        if (tid == 0) { q.counts[2 * g] = 0; q.counts[2 * g + 1] = 0; }
        return;
    }
    ss_frame F;
    ss_load_frame(q.cell + 9 * (size_t)b, F);
    if (!F.ok) {
        if (tid == 0) { atomicOr(q.err, SS_ERR_CELL); q.counts[2 * g] = 0; q.counts[2 * g + 1] = 0; }
        return;
    }
    // first pass: near-duplicates, the identity alone
    for (int c = tid; c < n; c += SS_THREADS) q.first[s0 + c] = (!q.valid || q.valid[s0 + c] != 0) ? -2 : -1;
    const int n1 = ss_rounds<false>(q, F, s0, n, q.first, nullptr, 0, 1, ops, rx, red);
    // second pass: its survivors, under the slab's operations
    for (int c = tid; c < n; c += SS_THREADS) {
        q.rep[s0 + c] = q.first[s0 + c] == s0 + c ? -2 : -1;
        q.mult[s0 + c] = 0;
    }
    const int n2 = q.op_offset ? ss_rounds<true>(q, F, s0, n, q.rep, q.mult, o0, nops, ops, rx, red)
                               : ss_rounds<false>(q, F, s0, n, q.rep, q.mult, 0, 1, ops, rx, red);
    __syncthreads();                                         // every survivor's rep is written
    for (int c = tid; c < n; c += SS_THREADS) {
        const int v = q.first[s0 + c];
        if (v >= 0 && v != s0 + c) q.rep[s0 + c] = q.rep[v];   // rep[v] belongs to a survivor: nobody writes it here
    }
    if (tid == 0) { q.counts[2 * g] = n1; q.counts[2 * g + 1] = n2; }
}

extern "C" int32_t adf_reduce_sites(const float* cand, const int32_t* valid, const int32_t* seg_offset,
                                    const int32_t* seg_slab, const float* cell, int32_t num_candidates,
                                    int32_t num_segments, int32_t num_slabs, const int32_t* op_offset, const double* rot,
                                    const double* trans, int32_t num_ops, double tol, int32_t* first, int32_t* rep,
                                    int32_t* multiplicity, int32_t* counts, void* stream) {
    if (!cand || !seg_offset || !cell || !first || !rep || !multiplicity || !counts) {
        adf_set_error("reduce_sites: null argument");
        return ADF_EINVAL;
    }
    if (op_offset && (!rot || !trans || num_ops <= 0)) {
        adf_set_error("reduce_sites: op_offset without rot / trans, or %d operations", num_ops);
        return ADF_EINVAL;
    }
    if (num_candidates < 0 || num_segments <= 0 || num_slabs <= 0) {
        adf_set_error("reduce_sites: %d candidates, %d segments, %d slabs", num_candidates, num_segments, num_slabs);
        return ADF_EINVAL;
    }
    if (!(tol >= 0.0) || !(tol < (double)INFINITY)) {
        adf_set_error("reduce_sites: tol must be finite and not negative");
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    adf_errword err;   // freed on every return (after the synchronisation in finish)
    ADF_TRY(err.create(s));
    ss_reduce_params q = {};
    q.cand = cand; q.valid = valid; q.seg_offset = seg_offset; q.seg_slab = seg_slab; q.cell = cell;
    q.op_offset = op_offset; q.rot = rot; q.trans = trans;
    q.C = num_candidates; q.G = num_segments; q.B = num_slabs; q.K = op_offset ? num_ops : 0;
    q.tol = tol;
    q.first = first; q.rep = rep; q.mult = multiplicity; q.counts = counts; q.err = err.dev;
    hipLaunchKernelGGL(ss_reduce_kernel, dim3(num_segments), dim3(SS_THREADS), 0, s, q);
    ADF_HIP_CHECK(hipGetLastError());
    return err.finish(s, "reduce_sites", SS_ERRORS);
}
