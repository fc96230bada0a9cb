// Surface triangles: the Delaunay triangulation of the 3 x 3 tiled tag-1 atoms of every slab of a batch,
// pruned to the triangles with a vertex in the central tile - what placement.surface_triangles does on the host with
// scipy.spatial.Delaunay [the reference's placement/adsorbate_slab_config.py:117-142, 479-508].  The contract is in
// include/adsorbdiff_hip.h.
//
// All arithmetic is float64 on float32 inputs; a vertex is rounded to float32 once, when it is stored.  No float atomics;
// the integer atomics are the OR on the error word.  Every output row has one writer and is written with an ordinary
// vector store: two calls give the same bits, and nothing a slab gets depends on its batch-mates.
//
// Formulation: the star of every central-tile point, one wave per point.  The nearest tiled point is a Delaunay neighbour
// (its diametral disc is empty).  From a star edge i -> j the face to its left is found by gift wrapping: among the points
// left of i -> j the one whose circle through i and j has its centre furthest to the right (least t, centre = midpoint +
// t * left normal) has no point inside; every point within circle_tol of that circle belongs to the face, a convex
// polygon.  The polygon is split as a fan from its canonical vertex (least x up to circle_tol, then least y), so every
// vertex that finds it splits it alike; the walk goes on from the polygon's other side at i and closes where it began.
// Each lane proposes over its slice of the points and one wave reduction decides: O(faces * points) per star.
//
// Mapping.  tg_prepare_kernel: one workgroup; a thread counts the tag-1 atoms of its slab, picks its tiling vectors, and
// the workgroup scans the counts.  tg_tile_kernel: one workgroup per slab compacts the tag-1 atoms in atom order (ballot
// prefix) and writes the 9 n_top tiled x, y as doubles.  tg_walk_kernel<false>: workgroups (slab, part), one wave per
// central point, the slab's points staged in LDS where they fit; counts the triangles each star owns - those whose least
// index is the star's centre.  tg_scan_kernel: one workgroup, exclusive scan of the counts: row of every star, tri_offset.
// tg_walk_kernel<true>: the same walk writes the (b, c) of its triangles, then sorts them by rank and stores the rows.
// Slabs, points, faces, polygon vertices and triangles per star are all looped: nothing is capped.
#include <float.h>
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "host_util.h"
#include "cell3.h"
#include "lanes.h"

#define TG_THREADS 256
#define TG_WAVES (TG_THREADS / 64)
#define TG_LDS_POINTS 4000      // tiled points (two doubles each) staged in LDS: 62.5 KiB
#define TG_LEFT_SIN 1e-10       // a point is left of an edge when the sine of the angle it makes exceeds this

enum { TG_ERR_RANGE = 1, TG_ERR_NOTOP = 2, TG_ERR_CELL = 4, TG_ERR_DEGENERATE = 8, TG_ERR_CAPACITY = 16 };

// tile t of surface_triangles' order - the central one first, then (i, j) for i, j in (-1, 0, 1) - as (i, j)
__device__ __forceinline__ void tg_tile_ij(int t, int& i, int& j) {
    const int m = t == 0 ? 4 : (t <= 4 ? t - 1 : t);
    i = m / 3 - 1;
    j = m % 3 - 1;
}

// (p + i v0) + j v1 in float64: i, j are 0 or +-1, the products are exact and a contraction changes nothing
__device__ __forceinline__ double tg_tiled(double p, double v0, double v1, int i, int j) {
    return (p + (double)i * v0) + (double)j * v1;
}

// ------------------------------------------------------------------------------------------------ per-slab preparation
__global__ __launch_bounds__(TG_THREADS) void tg_prepare_kernel(const int32_t* __restrict__ tags,
                                                                const int32_t* __restrict__ atom_offset,
                                                                const float* __restrict__ cell, int N, int B,
                                                                int32_t* __restrict__ top_off, double* __restrict__ tv,
                                                                int32_t* err) {
    __shared__ int red[TG_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0, bad = 0;
    for (int base = 0; base < B; base += TG_THREADS) {
        const int b = base + tid;
        int top = 0;
        if (b < B) {
            const int a0 = atom_offset[b], a1 = atom_offset[b + 1];
            if (a0 < 0 || a1 < a0 || a1 > N) {
                bad |= TG_ERR_RANGE;
            } else {
                for (int i = a0; i < a1; ++i) top += tags[i] == 1 ? 1 : 0;
                if (top == 0) bad |= TG_ERR_NOTOP;
                // tiling_vectors: the first two rows with round(v[0], 3) != 0 or round(v[1], 1) != 0
                int found = 0;
                bool finite = true;
                for (int r = 0; r < 3; ++r) {
                    const double x = (double)cell[9 * (size_t)b + 3 * r], y = (double)cell[9 * (size_t)b + 3 * r + 1],
                                 z = (double)cell[9 * (size_t)b + 3 * r + 2];
                    if (!(fabs(x) >= 0.0005 || fabs(y) >= 0.05) || found == 2) continue;   // (a NaN row does not pass)
                    finite = finite && fabs(x) < INFINITY && fabs(y) < INFINITY && fabs(z) < INFINITY;
                    tv[6 * (size_t)b + 3 * found] = x;
                    tv[6 * (size_t)b + 3 * found + 1] = y;
                    tv[6 * (size_t)b + 3 * found + 2] = z;
                    ++found;
                }
                if (found < 2 || !finite) { bad |= TG_ERR_CELL; top = 0; }
            }
        }
        // exclusive scan of `top` over the workgroup (the sum is at most N)
        int incl = top;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        __syncthreads();                                // the previous round's reads of red are done
        if (lane == 63) red[wave] = incl;
        __syncthreads();
        int before = carry, all = 0;
#pragma unroll
        for (int w = 0; w < TG_WAVES; ++w) {
            if (w < wave) before += red[w];
            all += red[w];
        }
        if (b < B) top_off[b] = before + incl - top;
        carry += all;
    }
    if (tid == 0) top_off[B] = carry;
    if (bad) atomicOr(err, bad);
}

// ------------------------------------------------------------------------------------------------ tiled points
__global__ __launch_bounds__(TG_THREADS) void tg_tile_kernel(const float* __restrict__ pos, const int32_t* __restrict__ tags,
                                                             const int32_t* __restrict__ atom_offset,
                                                             const int32_t* __restrict__ top_off,
                                                             const double* __restrict__ tv, int N,
                                                             int32_t* __restrict__ top_atom, double2* __restrict__ pts,
                                                             const int32_t* err) {
    __shared__ int red[TG_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (*err != 0) return;                              // written by the kernel before this one: the same in every thread
    const int a0 = atom_offset[b], a1 = atom_offset[b + 1], t0 = top_off[b], n_top = top_off[b + 1] - t0;
    if (a0 < 0 || a1 < a0 || a1 > N || t0 < 0 || n_top <= 0 || t0 + n_top > N) return;
    const double v0x = tv[6 * (size_t)b], v0y = tv[6 * (size_t)b + 1], v1x = tv[6 * (size_t)b + 3], v1y = tv[6 * (size_t)b + 4];
    double2* P = pts + 9 * (size_t)t0;
    int running = 0;
    for (int base = a0; base < a1; base += TG_THREADS) {
        const int i = base + tid;
        const bool mine = i < a1 && tags[i] == 1;
        const unsigned long long m = __ballot(mine);
        __syncthreads();                                // the previous round's reads of red are done
        if (lane == 0) red[wave] = __popcll(m);
        __syncthreads();
        int before = running, all = 0;
#pragma unroll
        for (int w = 0; w < TG_WAVES; ++w) {
            if (w < wave) before += red[w];
            all += red[w];
        }
        const int slot = before + __popcll(m & ((1ull << lane) - 1ull));
        if (mine && slot < n_top) {
            top_atom[t0 + slot] = i;
            const double x = (double)pos[3 * (size_t)i], y = (double)pos[3 * (size_t)i + 1];
            for (int t = 0; t < 9; ++t) {
                int ti, tj;
                tg_tile_ij(t, ti, tj);
                P[(size_t)t * n_top + slot] = make_double2(tg_tiled(x, v0x, v1x, ti, tj), tg_tiled(y, v0y, v1y, ti, tj));
            }
        }
        running += all;
    }
}

// ------------------------------------------------------------------------------------------------ the star walk
// (key, index) of the least key over the wave, ties to the least index; left in every lane
// One triangle (i, x, y), counter-clockwise, of the star of i: owned, and counted, where i is its least index.  Emitting:
// lane 0 notes (x, y) in row base + count of bc (rows up to `room` only: what the counting walk found).
template <bool EMIT>
__device__ __forceinline__ void tg_triangle(int i, int x, int y, int& count, int2* bc, int room) {
    if (i >= x || i >= y) return;
    if (EMIT && (threadIdx.x & 63) == 0 && count < room) bc[count] = make_int2(x, y);
    ++count;
}

// The star of central point i of a slab of n tiled points P (LDS or global).  Every decision is made on values a wave
// reduction left in all lanes: the control flow is the same in every lane.  Returns the triangles owned, or -1: the walk
// found no point to the left of an edge or did not close (collinear points, a lattice that does not surround i).
template <bool EMIT>
__device__ __forceinline__ int tg_star(const double2* P, int n, int i, double tol, int2* bc, int room) {
    const int lane = threadIdx.x & 63;
    const double2 pi = P[i];
    // the nearest point: a Delaunay neighbour
    double key = INFINITY;
    int j0 = INT_MAX;
    for (int q = lane; q < n; q += 64) {
        if (q == i) continue;
        const double2 p = P[q];
        const double ux = p.x - pi.x, uy = p.y - pi.y, d2 = ux * ux + uy * uy;
        if (d2 < key) { key = d2; j0 = q; }
    }
    adf_wave_argmin(key, j0);
    if (j0 == INT_MAX || !(key > 0.0)) return -1;
    int count = 0, j = j0;
    for (int step = 0;; ++step) {
        if (step >= n) return -1;
        const double2 pj = P[j];
        const double dx = pj.x - pi.x, dy = pj.y - pi.y, dd = dx * dx + dy * dy;
        // pass A: the left point whose circle through i and j has the least t
        double tk = INFINITY;
        int ks = INT_MAX;
        for (int q = lane; q < n; q += 64) {
            if (q == i || q == j) continue;
            const double2 p = P[q];
            const double ux = p.x - pi.x, uy = p.y - pi.y, uu = ux * ux + uy * uy;
            const double cr = dx * uy - dy * ux;
            if (!(cr > 0.0) || !(cr * cr > (TG_LEFT_SIN * TG_LEFT_SIN) * dd * uu)) continue;
            const double t = (ux * (ux - dx) + uy * (uy - dy)) / (2.0 * cr);
            if (t < tk) { tk = t; ks = q; }
        }
        adf_wave_argmin(tk, ks);
        if (ks == INT_MAX || !(fabs(tk) < INFINITY)) return -1;
        const double cx = pi.x + 0.5 * dx - tk * dy, cy = pi.y + 0.5 * dy + tk * dx;
        const double r = sqrt(dd * (0.25 + tk * tk));
        // pass B: the face - every point on that circle - its least x and its last vertex as seen from i
        int on_count = 0, qs = INT_MAX;
        double xmin = INFINITY, cmin = INFINITY;           // cmin: least cosine of the angle from i -> j, the largest angle
        for (int q = lane; q < n; q += 64) {
            if (q == i) continue;
            const double2 p = P[q];
            const double ex = p.x - cx, ey = p.y - cy;
            const bool on = q == j || q == ks || fabs(sqrt(ex * ex + ey * ey) - r) <= tol;
            if (!on) continue;
            ++on_count;
            xmin = fmin(xmin, p.x);
            if (q == j) continue;
            const double ux = p.x - pi.x, uy = p.y - pi.y;
            const double c = (dx * ux + dy * uy) / sqrt(ux * ux + uy * uy);
            if (c < cmin) { cmin = c; qs = q; }
        }
        on_count = adf_wave_sum(on_count);
        adf_wave_argmin(cmin, qs);
        if (qs == INT_MAX) return -1;
        if (on_count <= 2) {
            tg_triangle<EMIT>(i, j, qs, count, bc, room);   // a triangle: the generic case
        } else {
            xmin = fmin(adf_wave_min(xmin), pi.x);
            // pass C: the canonical vertex - least y among the vertices whose x is within tol of the least
            double ymin = INFINITY;
            int v = INT_MAX;
            if (lane == 0 && pi.x <= xmin + tol) { ymin = pi.y; v = i; }
            for (int q = lane; q < n; q += 64) {
                if (q == i) continue;
                const double2 p = P[q];
                const double ex = p.x - cx, ey = p.y - cy;
                const bool on = q == j || q == ks || fabs(sqrt(ex * ex + ey * ey) - r) <= tol;
                if (!on || !(p.x <= xmin + tol)) continue;
                if (p.y < ymin || (p.y == ymin && q < v)) { ymin = p.y; v = q; }
            }
            adf_wave_argmin(ymin, v);
            if (v == i) {
                // the fan is i's own: the polygon's vertices in the order of their angle from i -> j
                int cur = j;
                double ccur = INFINITY;                     // cosine of the current vertex (j: angle 0, above every cosine)
                for (int m = 0; cur != qs; ++m) {
                    if (m >= on_count) return -1;
                    double best = INFINITY;                 // -cosine: the least angle beyond the current vertex's
                    int nx = INT_MAX;
                    for (int q = lane; q < n; q += 64) {
                        if (q == i || q == j || q == cur) continue;
                        const double2 p = P[q];
                        const double ex = p.x - cx, ey = p.y - cy;
                        const bool on = q == ks || fabs(sqrt(ex * ex + ey * ey) - r) <= tol;
                        if (!on) continue;
                        const double ux = p.x - pi.x, uy = p.y - pi.y;
                        const double c = (dx * ux + dy * uy) / sqrt(ux * ux + uy * uy);
                        if (c < ccur && -c < best) { best = -c; nx = q; }
                    }
                    adf_wave_argmin(best, nx);
                    if (nx == INT_MAX) return -1;
                    tg_triangle<EMIT>(i, cur, nx, count, bc, room);
                    cur = nx;
                    ccur = -best;
                }
            } else if (v == j || v == qs) {
                tg_triangle<EMIT>(i, j, qs, count, bc, room);
            } else {
                tg_triangle<EMIT>(i, j, v, count, bc, room);
                tg_triangle<EMIT>(i, v, qs, count, bc, room);
            }
        }
        j = qs;
        if (j == j0) break;
    }
    return count;
}

struct tg_walk_params {
    const float* pos; const int32_t* top_off; const int32_t* top_atom; const double* tv;
    const double2* pts; const int32_t* start;
    int32_t N, lds_points, capacity;
    double tol;
    int32_t* cnt; int2* bc; int32_t* tri_offset; float* tri; int32_t* tri_index; int32_t* err;
};

template <bool EMIT>
__global__ __launch_bounds__(TG_THREADS) void tg_walk_kernel(tg_walk_params q) {
    extern __shared__ double2 tg_sm[];
    __shared__ int err_seen;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) err_seen = *q.err;                        // one read for the workgroup: other walkers may be setting bits
    __syncthreads();
    if (err_seen != 0) return;
    const int t0 = q.top_off[b], n_top = q.top_off[b + 1] - t0;
    if (t0 < 0 || n_top <= 0 || t0 + n_top > q.N) return;
    const int n = 9 * n_top;
    const double2* G = q.pts + 9 * (size_t)t0;
    const bool staged = n <= q.lds_points;
    if (staged) {
        for (int e = tid; e < n; e += TG_THREADS) tg_sm[e] = G[e];
        __syncthreads();
    }
    if (EMIT && tid == 0 && blockIdx.y == 0) {
        q.tri_offset[b] = q.start[t0];
        if (b == (int)gridDim.x - 1) q.tri_offset[b + 1] = q.start[t0 + n_top];
    }
    for (int k = blockIdx.y * TG_WAVES + wave; k < n_top; k += gridDim.y * TG_WAVES) {
        const int row = EMIT ? q.start[t0 + k] : 0, room = EMIT ? q.start[t0 + k + 1] - row : 0;
        if (EMIT && (row < 0 || room < 0 || row + room > q.capacity)) continue;
        int2* bc = EMIT ? q.bc + row : nullptr;
        const int count = staged ? tg_star<EMIT>(tg_sm, n, k, q.tol, bc, room) : tg_star<EMIT>(G, n, k, q.tol, bc, room);
        if (!EMIT) {
            if (lane == 0) {
                q.cnt[t0 + k] = count < 0 ? 0 : count;
                if (count < 0) atomicOr(q.err, TG_ERR_DEGENERATE);
            }
            continue;
        }
        if (count != room) continue;                        // (the two walks are the same computation)
        __threadfence_block();                              // lane 0's rows of bc are written before the wave reads them
        const double v0[3] = {q.tv[6 * (size_t)b], q.tv[6 * (size_t)b + 1], q.tv[6 * (size_t)b + 2]};
        const double v1[3] = {q.tv[6 * (size_t)b + 3], q.tv[6 * (size_t)b + 4], q.tv[6 * (size_t)b + 5]};
        for (int t = lane; t < count; t += 64) {
            const int2 me = bc[t];
            int rank = 0;
            for (int u = 0; u < count; ++u) {
                const int2 o = bc[u];
                rank += (o.x < me.x || (o.x == me.x && o.y < me.y)) ? 1 : 0;
            }
            const size_t out = (size_t)row + rank;
            const int idx[3] = {k, me.x, me.y};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                q.tri_index[3 * out + c] = idx[c];
                int ti, tj;
                tg_tile_ij(idx[c] / n_top, ti, tj);
                const float* p = q.pos + 3 * (size_t)q.top_atom[t0 + idx[c] % n_top];
#pragma unroll
                for (int a = 0; a < 3; ++a) q.tri[9 * out + 3 * c + a] = (float)tg_tiled((double)p[a], v0[a], v1[a], ti, tj);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ rows of the stars
__global__ __launch_bounds__(TG_THREADS) void tg_scan_kernel(const int32_t* __restrict__ cnt,
                                                             const int32_t* __restrict__ top_off, int B, int N, int capacity,
                                                             int32_t* __restrict__ start, int32_t* err) {
    __shared__ int red[TG_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (*err != 0) return;
    const int S = min(max(top_off[B], 0), N);
    long long carry = 0;
    for (int base = 0; base < S; base += TG_THREADS) {
        const int e = base + tid;
        const int mine = e < S ? cnt[e] : 0;
        int incl = mine;                                    // a round's sum is below 18 * 256
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        __syncthreads();                                    // the previous round's reads of red are done
        if (lane == 63) red[wave] = incl;
        __syncthreads();
        long long before = carry, all = 0;
#pragma unroll
        for (int w = 0; w < TG_WAVES; ++w) {
            if (w < wave) before += red[w];
            all += red[w];
        }
        if (e < S) start[e] = (int32_t)min(before + incl - mine, (long long)capacity);
        carry += all;
    }
    if (tid == 0) {
        start[S] = (int32_t)min(carry, (long long)capacity);
        if (carry > (long long)capacity) atomicOr(err, TG_ERR_CAPACITY);
    }
}

extern "C" int32_t adf_surface_triangles(const float* pos, const int32_t* tags, const int32_t* atom_offset, const float* cell,
                                         int32_t num_atoms, int32_t num_slabs, double circle_tol, int32_t capacity,
                                         int32_t* tri_offset, float* tri, int32_t* tri_index, void* stream) {
    if (!pos || !tags || !atom_offset || !cell || !tri_offset || !tri || !tri_index) {
        adf_set_error("surface_triangles: null argument");
        return ADF_EINVAL;
    }
    if (num_atoms < 0 || num_slabs <= 0 || capacity < 0 || 18ll * num_atoms > (long long)INT_MAX) {
        adf_set_error("surface_triangles: %d atoms, %d slabs, tables of %d rows", num_atoms, num_slabs, capacity);
        return ADF_EINVAL;
    }
    if (!(circle_tol >= 0.0) || !(circle_tol < (double)INFINITY)) {
        adf_set_error("surface_triangles: circle_tol must be finite and not negative");
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)num_atoms, B = (size_t)num_slabs;
    const size_t rows = (size_t)std::min((long long)capacity, 18ll * num_atoms);     // more rows than that are never owned
    // one scratch block, freed on every return (after the synchronisation in finish): laid out by the same code twice
    double* tv;
    double2* pts;
    int32_t *err_dev, *top_off, *top_atom, *cnt, *start;
    int2* bc;
    auto lay = [&](adf_carver c) {
        tv = c.take<double>(6 * B); pts = c.take<double2>(9 * N);
        err_dev = c.take<int32_t>(1); top_off = c.take<int32_t>(B + 1); top_atom = c.take<int32_t>(N); cnt = c.take<int32_t>(N);
        start = c.take<int32_t>(N + 1); bc = c.take<int2>(rows);
        return c.bytes();
    };
    adf_pool tmp;
    void* block = nullptr;
    ADF_TRY(tmp.alloc(&block, lay(adf_carver())));
    lay(adf_carver(block));
    adf_errword err;
    ADF_TRY(err.adopt(err_dev, s));
    ADF_HIP_CHECK(hipMemsetAsync(tri_offset, 0, (B + 1) * sizeof(int32_t), s));
    hipLaunchKernelGGL(tg_prepare_kernel, dim3(1), dim3(TG_THREADS), 0, s, tags, atom_offset, cell, num_atoms, num_slabs,
                       top_off, tv, err.dev);
    ADF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(tg_tile_kernel, dim3(num_slabs), dim3(TG_THREADS), 0, s, pos, tags, atom_offset, top_off, tv, num_atoms,
                       top_atom, pts, err.dev);
    ADF_HIP_CHECK(hipGetLastError());
    tg_walk_params q = {};
    q.pos = pos; q.top_off = top_off; q.top_atom = top_atom; q.tv = tv; q.pts = pts; q.start = start;
    q.N = num_atoms; q.capacity = (int32_t)rows; q.tol = circle_tol;
    q.lds_points = (int32_t)std::min((long long)TG_LDS_POINTS, 9ll * num_atoms);
    q.cnt = cnt; q.bc = bc; q.tri_offset = tri_offset; q.tri = tri; q.tri_index = tri_index; q.err = err.dev;
    // workgroups per slab: a wave per star, sized by the mean slab (a slab's rows do not depend on it)
    const int parts = (int)std::min(64ll, std::max(1ll, ((long long)num_atoms / num_slabs + 31) / 32));
    const size_t lds = (size_t)q.lds_points * sizeof(double2);
    hipLaunchKernelGGL(tg_walk_kernel<false>, dim3(num_slabs, parts), dim3(TG_THREADS), lds, s, q);
    ADF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(tg_scan_kernel, dim3(1), dim3(TG_THREADS), 0, s, cnt, top_off, num_slabs, num_atoms, (int32_t)rows, start,
                       err.dev);
    ADF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(tg_walk_kernel<true>, dim3(num_slabs, parts), dim3(TG_THREADS), lds, s, q);
    ADF_HIP_CHECK(hipGetLastError());
    const adf_errrow errors[] = {
        {TG_ERR_RANGE, ADF_EINVAL, "%s: atom offsets not ascending or outside [0, N]"},
        {TG_ERR_NOTOP, ADF_EINVAL, "%s: a slab has no atom of tag 1"},
        {TG_ERR_CELL, ADF_EINVAL, "%s: a cell has fewer than two in-plane lattice vectors (or a non-finite one)"},
        {TG_ERR_DEGENERATE, ADF_EINVAL, "%s: a slab cannot be triangulated (its tiled points are collinear, coincide, or its "
                                        "tiling vectors do not surround the central tile)"},
        {TG_ERR_CAPACITY, ADF_EINVAL, "%s: more triangles than the tables hold (%d rows; 18 * num_atoms always suffices)", capacity}};
    return err.finish(s, "surface_triangles", errors);
}
