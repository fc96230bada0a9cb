// Duplicate sites: a per-slab pairwise site distance, a deterministic greedy clustering on top of it and a
// top-k ranking of the distinct valid sites.  The contract is in include/adsorbdiff_hip.h.  An extension: the reference has
// no counterpart (its write_vasp_inputs_nsite.py takes the best N relaxed sites per slab on the host, duplicates included).
//
// Distances.  One wave per ordered pair (i <= j) of sites of one group, lanes over the atoms of the two sites, which are
// read straight from global memory (a lane reads its atom's three floats of both sites; a wave reads two contiguous
// ranges).  Nothing of a group is staged in LDS: 100 sites x 200 atoms would be 240 KB.  The displacement is the IS2RS
// metric's (evaluate.hip, ev_is2rs_part_kernel): fractional coordinates through a float32 explicit inverse of site i's
// cell, % 1 twice, minus 1 above 0.5, times the cell.  The wave's maximum is a butterfly of fmaxf: any order gives the
// same bits.  The permutation-invariant adsorbate distance walks the other site's atoms 64 at a time: every lane holds
// one, the adsorbate ones are handed round with a lane read, so an adsorbate of any size needs no scratch.  The pair's
// value goes to (i, j) and (j, i) with plain stores; (i, i) is written as 0.
//
// Clustering.  One workgroup per group.  The visiting order is a rank sort inside the workgroup (energies staged through
// LDS in tiles, so a group may hold any number of sites); a site's rank lives in its own `rep` word, as -2 - rank, until
// the site is assigned, so no scratch is needed.  Then, repeatedly: the unassigned site of least rank becomes a
// representative (a workgroup minimum), and every unassigned site within both tolerances of it joins it.  That is the
// contract's "join the first representative in visiting order that fits": representatives are made in visiting order, and
// a site is taken by the first one made that fits it.  Every thread reads and writes the `rep` words of its own sites only.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "base.h"
#include "cell3.h"
#include "lanes.h"

#define UQ_THREADS 256

// numpy's x %= 1.0 on a float32 (evaluate.hip: ev_mod1).  x - trunc(x) is fmodf(x, 1) exactly.
__device__ __forceinline__ float uq_mod1(float x) {
    float r = x - truncf(x);
    if (r < 0.f) r = r + 1.0f;
    return r;
}

// |min_diff(d, cell)| of scripts/eval.py:765-777; c: rows = lattice vectors, inv: its inverse
__device__ __forceinline__ float uq_disp(float dx, float dy, float dz, const float (&c)[9], const float (&inv)[9]) {
    float f[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float x = dx * inv[j] + dy * inv[3 + j] + dz * inv[6 + j];
        x = uq_mod1(uq_mod1(x));
        f[j] = x > 0.5f ? x - 1.0f : x;
    }
    const float mx = f[0] * c[0] + f[1] * c[3] + f[2] * c[6];
    const float my = f[0] * c[1] + f[1] * c[4] + f[2] * c[7];
    const float mz = f[0] * c[2] + f[1] * c[5] + f[2] * c[8];
    return sqrtf(fmaf(mz, mz, fmaf(my, my, mx * mx)));
}

// R x + tau of a symmetry operation (T: R row-major, then tau), formed in double and rounded to float32 once
__device__ __forceinline__ void uq_apply(const double (&T)[12], float& x, float& y, float& z) {
    const double dx = x, dy = y, dz = z;
    x = (float)(T[0] * dx + T[1] * dy + T[2] * dz + T[9]);
    y = (float)(T[3] * dx + T[4] * dy + T[5] * dz + T[10]);
    z = (float)(T[6] * dx + T[7] * dy + T[8] * dz + T[11]);
}

// max over the adsorbate atoms of site X of the least displacement to an adsorbate atom of site Y of the same element;
// flip: the displacement is taken from Y's atom to X's (so that both directions evaluate the same vectors b - a).
// XF (the symmetry-aware entry): 1 - the atoms of X go through T first, 2 - the atoms of Y do; 0 - T is not read.
__device__ const double UQ_NO_OP[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};   // never read (XF = 0)

// the cell of site s (rows = lattice vectors) and its float32 explicit inverse
__device__ __forceinline__ void uq_cell(const float* __restrict__ cell, int s, float (&c)[9], float (&inv)[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) c[k] = cell[9 * (size_t)s + k];
    // (not cell3.h's adf_inv3: unguarded, and assigned row by row)
    const float m00 = c[4] * c[8] - c[5] * c[7], m01 = c[5] * c[6] - c[3] * c[8], m02 = c[3] * c[7] - c[4] * c[6];
    const float r = 1.0f / (c[0] * m00 + c[1] * m01 + c[2] * m02);
    inv[0] = m00 * r; inv[1] = (c[2] * c[7] - c[1] * c[8]) * r; inv[2] = (c[1] * c[5] - c[2] * c[4]) * r;
    inv[3] = m01 * r; inv[4] = (c[0] * c[8] - c[2] * c[6]) * r; inv[5] = (c[2] * c[3] - c[0] * c[5]) * r;
    inv[6] = m02 * r; inv[7] = (c[1] * c[6] - c[0] * c[7]) * r; inv[8] = (c[0] * c[4] - c[1] * c[3]) * r;
}

template <int XF>
__device__ __forceinline__ float uq_one_sided(const float* __restrict__ pos, const int32_t* __restrict__ tags,
                                              const int32_t* __restrict__ Z, int x0, int y0, int n, bool flip,
                                              const float (&c)[9], const float (&inv)[9], int lane, bool& nan,
                                              const double (&T)[12]) {
    float worst = 0.f;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const bool mine = k < n && tags[x0 + min(k, n - 1)] == 2;
        if (__ballot(mine) == 0ull) continue;           // a round of slab atoms
        const int ax = x0 + min(k, n - 1);
        float px = pos[3 * (size_t)ax], py = pos[3 * (size_t)ax + 1], pz = pos[3 * (size_t)ax + 2];
        if (XF == 1) uq_apply(T, px, py, pz);
        const int zx = Z[ax];
        float least = INFINITY;
        for (int m0 = 0; m0 < n; m0 += 64) {
            const int m = m0 + lane;
            const int ay = y0 + min(m, n - 1);
            unsigned long long ads = __ballot(m < n && tags[ay] == 2);
            if (ads == 0ull) continue;
            float qx = pos[3 * (size_t)ay], qy = pos[3 * (size_t)ay + 1], qz = pos[3 * (size_t)ay + 2];
            if (XF == 2) uq_apply(T, qx, qy, qz);
            const int zy = Z[ay];
            while (ads != 0ull) {
                const int l = __ffsll((long long)ads) - 1;
                ads &= ads - 1ull;
                const float ox = __shfl(qx, l, 64), oy = __shfl(qy, l, 64), oz = __shfl(qz, l, 64);
                const int oZ = __shfl(zy, l, 64);
                const float d = flip ? uq_disp(px - ox, py - oy, pz - oz, c, inv) : uq_disp(ox - px, oy - py, oz - pz, c, inv);
                if (d != d) nan = nan || mine;
                if (mine && oZ == zx) least = fminf(least, d);
            }
        }
        if (mine && least < INFINITY) worst = fmaxf(worst, least);
    }
    return worst;
}

__global__ __launch_bounds__(UQ_THREADS) void uq_pair_kernel(
    const float* __restrict__ pos, const float* __restrict__ cell, const int32_t* __restrict__ tags,
    const int32_t* __restrict__ Z, const int32_t* __restrict__ atom_offset, const int32_t* __restrict__ group_offset,
    const int64_t* __restrict__ pair_offset, int num_atoms, int num_sites, long long out_len, int include_slab,
    int permutation_invariant, float* __restrict__ out) {
    const int g = blockIdx.x, lane = threadIdx.x & 63;
    const int s0 = min(max(group_offset[g], 0), num_sites), s1 = min(max(group_offset[g + 1], s0), num_sites);
    const long long n = s1 - s0;
    const long long po = pair_offset[g];
    if (n <= 0 || po < 0 || po + n * n > out_len) return;
    const long long wave0 = (long long)blockIdx.y * (UQ_THREADS / 64) + (threadIdx.x >> 6);
    const long long stride = (long long)gridDim.y * (UQ_THREADS / 64);
    for (long long p = wave0; p < n * n; p += stride) {
        const int i = (int)(p / n), j = (int)(p - (long long)i * n);
        if (i > j) continue;
        if (i == j) {
            if (lane == 0) out[po + p] = 0.f;
            continue;
        }
        const int sa = s0 + i, sb = s0 + j;
        const int a0 = min(max(atom_offset[sa], 0), num_atoms), a1 = min(max(atom_offset[sa + 1], a0), num_atoms);
        const int b0 = min(max(atom_offset[sb], 0), num_atoms), b1 = min(max(atom_offset[sb + 1], b0), num_atoms);
        const int na = a1 - a0;
        float d = 0.f;
        bool differ = na != b1 - b0, nan = false;
        if (!differ && na > 0) {
            float c[9], inv[9];
            uq_cell(cell, sa, c, inv);
            // the ordered part: slab atoms, and the adsorbate atoms when the adsorbate is compared in order
            bool any_ads = false;
            for (int k = lane; k < na; k += 64) {
                const int ta = tags[a0 + k], tb = tags[b0 + k];
                if (ta != tb || Z[a0 + k] != Z[b0 + k]) differ = true;
                const bool ads = ta == 2;
                any_ads = any_ads || ads;
                if (ads ? permutation_invariant != 0 : include_slab == 0) continue;
                const size_t ra = 3 * (size_t)(a0 + k), rb = 3 * (size_t)(b0 + k);
                const float v = uq_disp(pos[rb] - pos[ra], pos[rb + 1] - pos[ra + 1], pos[rb + 2] - pos[ra + 2], c, inv);
                if (v != v) nan = true;
                d = fmaxf(d, v);
            }
            differ = __ballot(differ) != 0ull;
            if (!differ && permutation_invariant && __ballot(any_ads) != 0ull) {
                d = fmaxf(d, uq_one_sided<0>(pos, tags, Z, a0, b0, na, false, c, inv, lane, nan, UQ_NO_OP));
                d = fmaxf(d, uq_one_sided<0>(pos, tags, Z, b0, a0, na, true, c, inv, lane, nan, UQ_NO_OP));
            }
            d = adf_wave_max(d);
            nan = __ballot(nan) != 0ull;
        }
        if (nan) d = NAN;               // a non-finite coordinate: the pair is within no tolerance
        if (differ) d = INFINITY;
        if (lane == 0) {
            out[po + p] = d;
            out[po + (long long)j * n + i] = d;
        }
    }
}

static int uq_pair_slots(int32_t num_sites, int32_t num_groups) {
    const long long avg = (num_sites + num_groups - 1) / num_groups;
    const long long blocks = (avg * avg + (UQ_THREADS / 64) - 1) / (UQ_THREADS / 64);
    return (int)(blocks > 4096 ? 4096 : blocks < 1 ? 1 : blocks);
}

extern "C" int32_t adf_site_pair_distances(const float* pos, const float* cell, const int32_t* tags,
                                           const int32_t* atomic_numbers, const int32_t* atom_offset,
                                           const int32_t* group_offset, const int64_t* pair_offset, int32_t num_atoms,
                                           int32_t num_sites, int32_t num_groups, int64_t out_len, int32_t include_slab,
                                           int32_t permutation_invariant, float* out, void* stream) {
    if (!pos || !cell || !tags || !atomic_numbers || !atom_offset || !group_offset || !pair_offset || !out) {
        adf_set_error("site_pair_distances: null argument");
        return ADF_EINVAL;
    }
    if (num_atoms < 0 || num_sites <= 0 || num_groups <= 0 || num_groups > num_sites || out_len < num_sites) {
        adf_set_error("site_pair_distances: %d atoms, %d sites, %d groups, %lld output elements", num_atoms, num_sites,
                      num_groups, (long long)out_len);
        return ADF_EINVAL;
    }
    // waves per group: one per matrix entry of the average group (the lower triangle's leave at once), so that the common
    // group has a wave per pair; a larger group strides over its pairs, a smaller one leaves its spare waves at once
    const int slots = uq_pair_slots(num_sites, num_groups);
    hipLaunchKernelGGL(uq_pair_kernel, dim3(num_groups, slots), dim3(UQ_THREADS), 0, (hipStream_t)stream, pos, cell, tags,
                       atomic_numbers, atom_offset, group_offset, pair_offset, num_atoms, num_sites, (long long)out_len,
                       include_slab, permutation_invariant, out);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}

// ---- the symmetry-aware distance: d_sym(i, j) = min over the operations g of the group's slab of
// d(g . site i, site j), i the earlier site.  One wave per pair, the operations one after the other; per operation the
// adsorbate part first, and the slab part only while the operation can still win.  Operation 0 of every group is the
// identity and is not applied, so a group with that one operation evaluates the expressions of uq_pair_kernel.
__global__ __launch_bounds__(UQ_THREADS) void uq_pair_sym_kernel(
    const float* __restrict__ pos, const float* __restrict__ cell, const int32_t* __restrict__ tags,
    const int32_t* __restrict__ Z, const int32_t* __restrict__ atom_offset, const int32_t* __restrict__ group_offset,
    const int64_t* __restrict__ pair_offset, const int32_t* __restrict__ op_offset, const double* __restrict__ rot,
    const double* __restrict__ trans, const int32_t* __restrict__ perm, const int64_t* __restrict__ perm_offset,
    int num_atoms, int num_sites, long long out_len, int num_ops, long long perm_len, int include_slab,
    int permutation_invariant, float* __restrict__ out, int32_t* __restrict__ best_op) {
    const int g = blockIdx.x, lane = threadIdx.x & 63;
    const int s0 = min(max(group_offset[g], 0), num_sites), s1 = min(max(group_offset[g + 1], s0), num_sites);
    const long long n = s1 - s0;
    const long long po = pair_offset[g];
    if (n <= 0 || po < 0 || po + n * n > out_len) return;
    // the group's operations: [o0, o0 + nops), each with a permutation of nb slab atoms
    const int o0 = op_offset[g];
    int nops = op_offset[g + 1] - o0;
    const long long pp = perm_offset[g];
    long long nb = -1;
    if (o0 >= 0 && nops > 0 && o0 + (long long)nops <= num_ops && pp >= 0 && perm_offset[g + 1] <= perm_len &&
        perm_offset[g + 1] >= pp && (perm_offset[g + 1] - pp) % nops == 0)
        nb = (perm_offset[g + 1] - pp) / nops;
    const long long wave0 = (long long)blockIdx.y * (UQ_THREADS / 64) + (threadIdx.x >> 6);
    const long long stride = (long long)gridDim.y * (UQ_THREADS / 64);
    for (long long p = wave0; p < n * n; p += stride) {
        const int i = (int)(p / n), j = (int)(p - (long long)i * n);
        if (i > j) continue;
        if (i == j) {
            if (lane == 0) { out[po + p] = 0.f; best_op[po + p] = 0; }
            continue;
        }
        const int sa = s0 + i, sb = s0 + j;
        const int a0 = min(max(atom_offset[sa], 0), num_atoms), a1 = min(max(atom_offset[sa + 1], a0), num_atoms);
        const int b0 = min(max(atom_offset[sb], 0), num_atoms), b1 = min(max(atom_offset[sb + 1], b0), num_atoms);
        const int na = a1 - a0;
        float best = INFINITY;
        int bop = 0;
        bool differ = na != b1 - b0, nan = false;
        if (!differ && na > 0) {
            float c[9], inv[9];
            uq_cell(cell, sa, c, inv);
            // the layout: equal tags and elements, the adsorbate one contiguous block [q0, q0 + nads)
            int q0 = INT_MAX, q1 = -1, cnt = 0;
            for (int k = lane; k < na; k += 64) {
                const int ta = tags[a0 + k];
                if (ta != tags[b0 + k] || Z[a0 + k] != Z[b0 + k]) differ = true;
                if (ta == 2) { q0 = min(q0, k); q1 = max(q1, k); ++cnt; }
            }
            differ = __ballot(differ) != 0ull;
            q0 = adf_wave_min(q0);
            q1 = -adf_wave_min(-q1);
            int nads = cnt;
            // kept inline: as a call to lanes.h this butterfly reorders the kernel's instructions (tools/device_asm_diff.py)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) nads += __shfl_xor(nads, o, 64);
            if (nads == 0) q0 = na;
            const int nslab = na - nads;
            if ((nads > 0 && q1 - q0 + 1 != nads) || nslab != nb) differ = true;
            for (int op = 0; op < nops && !differ; ++op) {
                double T[12];
#pragma unroll
                for (int k = 0; k < 9; ++k) T[k] = rot[9 * (size_t)(o0 + op) + k];
#pragma unroll
                for (int k = 0; k < 3; ++k) T[9 + k] = trans[3 * (size_t)(o0 + op) + k];
                float d = 0.f;
                bool bad = false;
                if (nads > 0 && permutation_invariant) {
                    if (op == 0) {
                        d = fmaxf(d, uq_one_sided<0>(pos, tags, Z, a0, b0, na, false, c, inv, lane, bad, T));
                        d = fmaxf(d, uq_one_sided<0>(pos, tags, Z, b0, a0, na, true, c, inv, lane, bad, T));
                    } else {
                        d = fmaxf(d, uq_one_sided<1>(pos, tags, Z, a0, b0, na, false, c, inv, lane, bad, T));
                        d = fmaxf(d, uq_one_sided<2>(pos, tags, Z, b0, a0, na, true, c, inv, lane, bad, T));
                    }
                } else if (nads > 0) {
                    for (int k = q0 + lane; k < q0 + nads; k += 64) {
                        const size_t ra = 3 * (size_t)(a0 + k), rb = 3 * (size_t)(b0 + k);
                        float x = pos[ra], y = pos[ra + 1], z = pos[ra + 2];
                        if (op != 0) uq_apply(T, x, y, z);
                        const float v = uq_disp(pos[rb] - x, pos[rb + 1] - y, pos[rb + 2] - z, c, inv);
                        if (v != v) bad = true;
                        d = fmaxf(d, v);
                    }
                }
                d = adf_wave_max(d);
                if (__ballot(bad) != 0ull) { nan = true; continue; }
                if (!(d < best)) continue;                  // the slab part can only raise d: this operation cannot win
                if (include_slab) {
                    const int32_t* pm = perm + pp + (long long)op * nb;
                    for (int r = lane; r < nslab; r += 64) {
                        const int t = op == 0 ? r : pm[r];
                        if (t < 0 || t >= nslab) { bad = true; continue; }
                        const size_t ra = 3 * (size_t)(a0 + (r < q0 ? r : r + nads)), rb = 3 * (size_t)(b0 + (t < q0 ? t : t + nads));
                        float x = pos[ra], y = pos[ra + 1], z = pos[ra + 2];
                        if (op != 0) uq_apply(T, x, y, z);
                        const float v = uq_disp(pos[rb] - x, pos[rb + 1] - y, pos[rb + 2] - z, c, inv);
                        if (v != v) bad = true;
                        d = fmaxf(d, v);
                    }
                    d = adf_wave_max(d);
                    if (__ballot(bad) != 0ull) { nan = true; continue; }
                }
                if (d < best) { best = d; bop = op; }
            }
        } else if (!differ) {
            best = nb == 0 ? 0.f : INFINITY;               // two sites without atoms
        }
        if (nan) { best = NAN; bop = 0; }                   // a non-finite coordinate: the pair is within no tolerance
        if (differ) { best = INFINITY; bop = 0; }
        if (lane == 0) {
            out[po + p] = best;
            out[po + (long long)j * n + i] = best;
            best_op[po + p] = bop;
            best_op[po + (long long)j * n + i] = bop;
        }
    }
}

extern "C" int32_t adf_site_pair_distances_sym(const float* pos, const float* cell, const int32_t* tags,
                                               const int32_t* atomic_numbers, const int32_t* atom_offset,
                                               const int32_t* group_offset, const int64_t* pair_offset, int32_t num_atoms,
                                               int32_t num_sites, int32_t num_groups, int64_t out_len, int32_t include_slab,
                                               int32_t permutation_invariant, const int32_t* op_offset, const double* rot,
                                               const double* trans, const int32_t* perm, const int64_t* perm_offset,
                                               int32_t num_ops, int64_t perm_len, float* out, int32_t* best_op, void* stream) {
    if (!pos || !cell || !tags || !atomic_numbers || !atom_offset || !group_offset || !pair_offset || !op_offset || !rot ||
        !trans || !perm || !perm_offset || !out || !best_op) {
        adf_set_error("site_pair_distances_sym: null argument");
        return ADF_EINVAL;
    }
    if (num_atoms < 0 || num_sites <= 0 || num_groups <= 0 || num_groups > num_sites || out_len < num_sites || num_ops <= 0 ||
        perm_len < 0) {
        adf_set_error("site_pair_distances_sym: %d atoms, %d sites, %d groups, %lld output elements, %d operations, %lld "
                      "permutation entries", num_atoms, num_sites, num_groups, (long long)out_len, num_ops, (long long)perm_len);
        return ADF_EINVAL;
    }
    hipLaunchKernelGGL(uq_pair_sym_kernel, dim3(num_groups, uq_pair_slots(num_sites, num_groups)), dim3(UQ_THREADS), 0,
                       (hipStream_t)stream, pos, cell, tags, atomic_numbers, atom_offset, group_offset, pair_offset, op_offset,
                       rot, trans, perm, perm_offset, num_atoms, num_sites, (long long)out_len, num_ops, (long long)perm_len,
                       include_slab, permutation_invariant, out, best_op);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}

// ---- clustering
__device__ __forceinline__ bool uq_valid(const float* energy, const int32_t* flags, int s) {
    bool ok = true;
    if (energy) { const float e = energy[s]; ok = !(e != e); }
    if (flags) ok = ok && (flags[4 * (size_t)s] | flags[4 * (size_t)s + 1] | flags[4 * (size_t)s + 2] | flags[4 * (size_t)s + 3]) == 0;
    return ok;
}

__global__ __launch_bounds__(UQ_THREADS) void uq_cluster_kernel(
    const float* __restrict__ dist, const int32_t* __restrict__ group_offset, const int64_t* __restrict__ pair_offset,
    int num_sites, long long dist_len, const float* __restrict__ energy, const int32_t* __restrict__ flags, float tol,
    float energy_tol, int32_t* __restrict__ rep, int32_t* __restrict__ n_unique) {
    __shared__ float tile[UQ_THREADS];                   // keys of one tile of sites; NaN: not valid
    __shared__ unsigned long long red[UQ_THREADS / 64];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s0 = min(max(group_offset[g], 0), num_sites), s1 = min(max(group_offset[g + 1], s0), num_sites);
    const int n = s1 - s0;
    const long long po = pair_offset[g];
    if (po < 0 || po + (long long)n * n > dist_len) {    // the matrix is not there: nothing of the group is valid
        for (int s = tid; s < n; s += UQ_THREADS) rep[s0 + s] = -1;
        if (tid == 0) n_unique[g] = 0;
        return;
    }
    // rank of every valid site in (energy, position): valid sites that come before it
    for (int base = 0; base < n; base += UQ_THREADS) {   // the sites this round ranks: one per thread
        const int s = base + tid;
        const bool mine = s < n && uq_valid(energy, flags, s0 + min(s, n - 1));
        const float es = mine && energy ? energy[s0 + s] : 0.f;
        int before = 0;
        for (int q0 = 0; q0 < n; q0 += UQ_THREADS) {
            __syncthreads();
            {
                const int q = q0 + tid;
                const bool ok = q < n && uq_valid(energy, flags, s0 + min(q, n - 1));
                tile[tid] = ok ? (energy ? energy[s0 + q] : 0.f) : NAN;
            }
            __syncthreads();
            const int qn = min(UQ_THREADS, n - q0);
            for (int t = 0; t < qn; ++t) {
                const float eq = tile[t];                // the same address in every lane: a broadcast
                before += (eq < es || (eq == es && q0 + t < s)) ? 1 : 0;
            }
        }
        if (s < n) rep[s0 + s] = mine ? -2 - before : -1;
    }
    int count = 0;
    for (;;) {
        // the unassigned site of least rank
        unsigned long long key = ~0ull;
        for (int s = tid; s < n; s += UQ_THREADS) {
            const int v = rep[s0 + s];
            if (v <= -2) {
                const unsigned long long k = ((unsigned long long)(unsigned)(-2 - v) << 32) | (unsigned)s;
                key = k < key ? k : key;
            }
        }
        // kept inline: as a call to lanes.h this butterfly reorders the kernel's instructions (tools/device_asm_diff.py)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(key, o, 64);
            key = other < key ? other : key;
        }
        __syncthreads();                                 // the previous round's reads of red are done
        if (lane == 0) red[wave] = key;
        __syncthreads();
        key = red[0];
#pragma unroll
        for (int w = 1; w < UQ_THREADS / 64; ++w) key = red[w] < key ? red[w] : key;
        if (key == ~0ull) break;
        const int r = (int)(unsigned)(key & 0xffffffffull);
        const double er = energy ? (double)energy[s0 + r] : 0.0;
        const float* row = dist + po + (long long)r * n;
        for (int s = tid; s < n; s += UQ_THREADS) {
            if (rep[s0 + s] > -2) continue;
            bool join = s == r;
            if (!join) {
                join = row[s] <= tol;
                if (join && energy && energy_tol >= 0.f) join = fabs((double)energy[s0 + s] - er) <= (double)energy_tol;
            }
            if (join) rep[s0 + s] = s0 + r;
        }
        ++count;
    }
    if (tid == 0) n_unique[g] = count;
}

extern "C" int32_t adf_unique_sites(const float* dist, const int32_t* group_offset, const int64_t* pair_offset,
                                    int32_t num_sites, int32_t num_groups, int64_t dist_len, const float* energy,
                                    const int32_t* flags, float tol, float energy_tol, int32_t* rep, int32_t* n_unique,
                                    void* stream) {
    if (!dist || !group_offset || !pair_offset || !rep || !n_unique) { adf_set_error("unique_sites: null argument"); return ADF_EINVAL; }
    if (num_sites <= 0 || num_groups <= 0 || num_groups > num_sites || dist_len < num_sites) {
        adf_set_error("unique_sites: %d sites, %d groups, %lld distances", num_sites, num_groups, (long long)dist_len);
        return ADF_EINVAL;
    }
    if (!(tol >= 0.f) || !(tol < INFINITY) || energy_tol != energy_tol) {
        adf_set_error("unique_sites: tol must be finite and not negative (an infinite distance marks sites that cannot be "
                      "compared), energy_tol not NaN");
        return ADF_EINVAL;
    }
    hipLaunchKernelGGL(uq_cluster_kernel, dim3(num_groups), dim3(UQ_THREADS), 0, (hipStream_t)stream, dist, group_offset,
                       pair_offset, num_sites, (long long)dist_len, energy, flags, tol, energy_tol, rep, n_unique);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}

// ---- top-k: one wave per group, k selections; each takes the least (energy, index) above the previous one, with the
// comparison and the butterfly of an_best_sites_kernel (anomaly.hip), so that column 0 is adf_select_best_sites' answer
__global__ __launch_bounds__(256) void uq_top_sites_kernel(const float* __restrict__ energy, const int32_t* __restrict__ flags,
                                                            const int32_t* __restrict__ rep,
                                                            const int32_t* __restrict__ group_offset, int num_groups, int k,
                                                            int32_t* __restrict__ top, float* __restrict__ top_energy) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= num_groups) return;
    const int s0 = group_offset[g], s1 = group_offset[g + 1];
    float last_e = 0.f;
    int last_i = -1;
    int c = 0;
    for (; c < k; ++c) {
        float be = INFINITY;
        int bi = INT_MAX;
        for (int i = s0 + lane; i < s1; i += 64) {
            const float e = energy[i];
            bool ok = !(e != e);
            if (flags) ok = ok && (flags[4 * (size_t)i] | flags[4 * (size_t)i + 1] | flags[4 * (size_t)i + 2] | flags[4 * (size_t)i + 3]) == 0;
            if (rep) ok = ok && rep[i] == i;
            if (c > 0) ok = ok && (e > last_e || (e == last_e && i > last_i));
            if (ok && (e < be || (e == be && i < bi))) { be = e; bi = i; }
        }
        // kept inline: as a call to lanes.h this butterfly reorders the kernel's instructions (tools/device_asm_diff.py)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float oe = __shfl_xor(be, o);
            const int oi = __shfl_xor(bi, o);
            if (oe < be || (oe == be && oi < bi)) { be = oe; bi = oi; }
        }
        if (bi == INT_MAX) break;
        if (lane == 0) { top[(size_t)g * k + c] = bi; top_energy[(size_t)g * k + c] = be; }
        last_e = be; last_i = bi;
    }
    for (int m = c + lane; m < k; m += 64) { top[(size_t)g * k + m] = -1; top_energy[(size_t)g * k + m] = INFINITY; }
}

extern "C" int32_t adf_select_top_sites(const float* energy, const int32_t* flags, const int32_t* rep,
                                        const int32_t* group_offset, int32_t num_groups, int32_t k, int32_t* top,
                                        float* top_energy, void* stream) {
    if (!energy || !group_offset || !top || !top_energy || num_groups <= 0 || k <= 0) { adf_set_error("select_top_sites: bad argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(uq_top_sites_kernel, dim3((num_groups + 3) / 4), dim3(256), 0, (hipStream_t)stream, energy, flags, rep,
                       group_offset, num_groups, k, top, top_energy);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}
