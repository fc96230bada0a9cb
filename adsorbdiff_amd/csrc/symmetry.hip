// Slab symmetry search: the operations x -> R x + tau of a bare slab that keep its surface normal, with the
// permutation each induces on the slab's atoms, for a whole batch of slabs.  The contract is in include/adsorbdiff_hip.h.
// An extension: the reference has no counterpart (it leaves symmetry reduction to pymatgen's site finder,
// placement/adsorbate_slab_config.py:113-116).
//
// Lattice step (sy_lattice_kernel): one wave per slab.  Every lane works out the point operations in double (a 2 x 2
// Lagrange reduction and 81 integer matrices: nothing worth spreading), the lanes share the species count that names the
// rarest element, and the slab's atoms are packed as (x, y, z, Z) for the kernels that follow.
//
// Verification (sy_verify_kernel): candidates are (slab, point slot 0..11, atom j of the slab), one wave each.  A slab of
// at most SY_CAP atoms is staged in LDS, a larger one is read from the packed global copy.  Lanes stride over atoms i, every
// lane walks the atoms k (one address per step: a broadcast), and the wave leaves at the first round of 64 atoms in which a
// lane found no partner - most candidates die in round one.  A survivor's partners are kept (in LDS; for a slab beyond
// SY_CAP in a global scratch row of its point slot, which one wave then walks through alone) and a second pass over them
// refuses a partner taken twice.  One flag word per candidate, plain stores.
//
// Ranking (sy_rank_kernel): one wave per slab turns the flags into ranks (ballot prefix) and writes the count.
// Emission (sy_emit_kernel): after the host has read the counts and sized the outputs, one wave per accepted candidate
// repeats the match - the same instructions on the same data, so the same partners - and writes rot / trans / W / perm
// at the candidate's rank.  Op 0 is the identity, written exactly.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "host_util.h"
#include "cell3.h"
#include "lanes.h"

#define SY_THREADS 256
#define SY_WAVES (SY_THREADS / 64)
#define SY_CAP 1024             // atoms of a slab held in LDS (16 B each, and 4 B per wave for the partners)
#define SY_SLOTS 12             // a two-dimensional lattice has at most 12 point operations
#define SY_LATD 128             // doubles per slab: M [9], inverse [9], R [12][9]
#define SY_LATI 64              // ints per slab: point ops, i0, rarest Z, refused, identity slot, W [12][4]

// the lattice record of a slab, as the verifying and emitting kernels hold it in LDS
struct sy_lat {
    double d[SY_LATD];
    int32_t i[SY_LATI];
};
// d[0..9): M, columns a, b, n; d[9..18): its inverse
#define SY_R(l, s, k) ((l).d[18 + 9 * (s) + (k)])
#define SY_NW(l) ((l).i[0])
#define SY_I0(l) ((l).i[1])
#define SY_ZR(l) ((l).i[2])
#define SY_BAD(l) ((l).i[3])
#define SY_IDENT(l) ((l).i[4])
#define SY_W(l, s, k) ((l).i[8 + 4 * (s) + (k)])

__global__ __launch_bounds__(SY_THREADS) void sy_lattice_kernel(
    const float* __restrict__ pos, const float* __restrict__ cell, const int32_t* __restrict__ Z,
    const int32_t* __restrict__ atom_offset, int num_atoms, int num_slabs, double symprec, int proper_only,
    double* __restrict__ lat_d, int32_t* __restrict__ lat_i, float4* __restrict__ xz) {
    const int b = blockIdx.x * SY_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= num_slabs) return;
    int a0, n;
    adf_segment_clamp(atom_offset, b, num_atoms, a0, n);
    for (int k = lane; k < n; k += 64) {
        const size_t r = 3 * (size_t)(a0 + k);
        xz[a0 + k] = make_float4(pos[r], pos[r + 1], pos[r + 2], __int_as_float(Z[a0 + k]));
    }
    // the first atom of the rarest atomic number, ties to the smaller number: the least (count, Z, index)
    int bc = INT_MAX, bz = INT_MAX, bi = INT_MAX;
    for (int i = lane; i < n; i += 64) {
        const int zi = Z[a0 + i];
        int cnt = 0;
        for (int k = 0; k < n; ++k) cnt += Z[a0 + k] == zi ? 1 : 0;
        if (cnt < bc || (cnt == bc && (zi < bz || (zi == bz && i < bi)))) { bc = cnt; bz = zi; bi = i; }
    }
    // kept inline: as a call to lanes.h this butterfly reorders the kernel's instructions (tools/device_asm_diff.py)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int oc = __shfl_xor(bc, o, 64), oz = __shfl_xor(bz, o, 64), oi = __shfl_xor(bi, o, 64);
        if (oc < bc || (oc == bc && (oz < bz || (oz == bz && oi < bi)))) { bc = oc; bz = oz; bi = oi; }
    }
    // ---- point operations, every lane the same arithmetic
    double a[3], bv[3], nv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { a[k] = (double)cell[9 * (size_t)b + k]; bv[k] = (double)cell[9 * (size_t)b + 3 + k]; }
    nv[0] = a[1] * bv[2] - a[2] * bv[1];   // (not cell3.h's adf_cross3: the call reorders this kernel's instructions)
    nv[1] = a[2] * bv[0] - a[0] * bv[2];
    nv[2] = a[0] * bv[1] - a[1] * bv[0];
    const double area = sqrt(adf_dot3(nv, nv));
    const double la = sqrt(adf_dot3(a, a)), lb = sqrt(adf_dot3(bv, bv));
    // symprec below half the shortest in-plane height, a finite cell of non-zero area: else the slab is refused
    const bool ok = area > 0.0 && area < (double)FLT_MAX && symprec >= 0.0 && symprec < 0.5 * area / fmax(la, lb);
    double M[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Mi[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    int nW = 0, Ws[SY_SLOTS][4];
    if (ok) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { nv[k] /= area; M[3 * k] = a[k]; M[3 * k + 1] = bv[k]; M[3 * k + 2] = nv[k]; }
        {   // (not cell3.h's adf_inv3: unguarded, and assigned row by row)
            const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
            const double r = 1.0 / (M[0] * c00 + M[1] * c01 + M[2] * c02);
            Mi[0] = c00 * r; Mi[1] = (M[2] * M[7] - M[1] * M[8]) * r; Mi[2] = (M[1] * M[5] - M[2] * M[4]) * r;
            Mi[3] = c01 * r; Mi[4] = (M[0] * M[8] - M[2] * M[6]) * r; Mi[5] = (M[2] * M[3] - M[0] * M[5]) * r;
            Mi[6] = c02 * r; Mi[7] = (M[1] * M[6] - M[0] * M[7]) * r; Mi[8] = (M[0] * M[4] - M[1] * M[3]) * r;
        }
        // Lagrange reduction: A_r = A U, columns (ar, br)
        long long U[4] = {1, 0, 0, 1};
        double ar[3], br[3];
        for (int it = 0; it < 100; ++it) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { ar[k] = a[k] * (double)U[0] + bv[k] * (double)U[2]; br[k] = a[k] * (double)U[1] + bv[k] * (double)U[3]; }
            const double aa = ar[0] * ar[0] + ar[1] * ar[1] + ar[2] * ar[2], bb = br[0] * br[0] + br[1] * br[1] + br[2] * br[2];
            if (aa > bb) {
                long long t = U[0]; U[0] = U[1]; U[1] = t;
                t = U[2]; U[2] = U[3]; U[3] = t;
                continue;
            }
            const double q = rint((ar[0] * br[0] + ar[1] * br[1] + ar[2] * br[2]) / aa);
            if (q == 0.0 || !(fabs(q) < 1e15)) break;
            U[1] -= (long long)q * U[0];
            U[3] -= (long long)q * U[2];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) { ar[k] = a[k] * (double)U[0] + bv[k] * (double)U[2]; br[k] = a[k] * (double)U[1] + bv[k] * (double)U[3]; }
        const long long detU = U[0] * U[3] - U[1] * U[2];                  // +-1
        const long long Ui[4] = {detU * U[3], -detU * U[1], -detU * U[2], detU * U[0]};
        double l0 = 0, l1 = 0, l2 = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { l0 += ar[k] * ar[k]; l1 += br[k] * br[k]; l2 += (ar[k] + br[k]) * (ar[k] + br[k]); }
        l0 = sqrt(l0); l1 = sqrt(l1); l2 = sqrt(l2);
        for (int code = 0; code < 81; ++code) {
            const int w00 = code / 27 - 1, w01 = (code / 9) % 3 - 1, w10 = (code / 3) % 3 - 1, w11 = code % 3 - 1;
            const int det = w00 * w11 - w01 * w10;
            if (det != 1 && !(det == -1 && !proper_only)) continue;
            double m0 = 0, m1 = 0, m2 = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double c0 = ar[k] * w00 + br[k] * w10, c1 = ar[k] * w01 + br[k] * w11;
                m0 += c0 * c0; m1 += c1 * c1; m2 += (c0 + c1) * (c0 + c1);
            }
            const double err = fmax(fmax(fabs(sqrt(m0) - l0), fabs(sqrt(m1) - l1)), fabs(sqrt(m2) - l2));
            if (!(err <= symprec) || nW >= SY_SLOTS) continue;
            // W = U W_r U^-1
            const long long t00 = U[0] * w00 + U[1] * w10, t01 = U[0] * w01 + U[1] * w11;
            const long long t10 = U[2] * w00 + U[3] * w10, t11 = U[2] * w01 + U[3] * w11;
            const int W[4] = {(int)(t00 * Ui[0] + t01 * Ui[2]), (int)(t00 * Ui[1] + t01 * Ui[3]),
                              (int)(t10 * Ui[0] + t11 * Ui[2]), (int)(t10 * Ui[1] + t11 * Ui[3])};
            int at = nW;                                                   // insertion in ascending (W00, W01, W10, W11)
            while (at > 0) {
                const int* p = Ws[at - 1];
                const bool less = W[0] != p[0] ? W[0] < p[0] : W[1] != p[1] ? W[1] < p[1] : W[2] != p[2] ? W[2] < p[2] : W[3] < p[3];
                if (!less) break;
#pragma unroll
                for (int k = 0; k < 4; ++k) Ws[at][k] = p[k];
                --at;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) Ws[at][k] = W[k];
            ++nW;
        }
    }
    if (lane != 0) return;
    double* ld = lat_d + (size_t)b * SY_LATD;
    int32_t* li = lat_i + (size_t)b * SY_LATI;
    for (int k = 0; k < 9; ++k) { ld[k] = M[k]; ld[9 + k] = Mi[k]; }
    int ident = 0;
    for (int s = 0; s < SY_SLOTS; ++s) {
        const bool on = s < nW;
        const double w00 = on ? Ws[s][0] : 1, w01 = on ? Ws[s][1] : 0, w10 = on ? Ws[s][2] : 0, w11 = on ? Ws[s][3] : 1;
        if (on && Ws[s][0] == 1 && Ws[s][1] == 0 && Ws[s][2] == 0 && Ws[s][3] == 1) ident = s;
        // R = M [W 0; 0 1] M^-1
        double T[9];
        for (int c = 0; c < 3; ++c) { T[c] = w00 * Mi[c] + w01 * Mi[3 + c]; T[3 + c] = w10 * Mi[c] + w11 * Mi[3 + c]; T[6 + c] = Mi[6 + c]; }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) ld[18 + 9 * s + 3 * r + c] = M[3 * r] * T[c] + M[3 * r + 1] * T[3 + c] + M[3 * r + 2] * T[6 + c];
        for (int k = 0; k < 4; ++k) li[8 + 4 * s + k] = on ? Ws[s][k] : 0;
    }
    li[0] = nW; li[1] = n > 0 ? bi : 0; li[2] = n > 0 ? bz : 0; li[3] = ok ? 0 : 1; li[4] = ident;
    li[5] = li[6] = li[7] = 0;
    for (int k = 8 + 4 * SY_SLOTS; k < SY_LATI; ++k) li[k] = 0;
    for (int k = 18 + 9 * SY_SLOTS; k < SY_LATD; ++k) ld[k] = 0.0;
}

// Does x -> R x + tau take every atom of the slab onto an atom of its element within symprec?  partner[i] receives the
// nearest such atom (ties to the lower index) of every atom the wave got to; the wave leaves at the first round with an
// atom that has none.  src: the slab's n packed atoms (LDS or global), partner: n words (LDS or global).
__device__ __forceinline__ bool sy_match(const float4* src, int n, const sy_lat& L, const double (&R)[9], const double (&tau)[3],
                                         double symprec, int lane, int32_t* partner) {
    const double s2 = symprec * symprec;
    double m[9], mi[9];                                                 // registers: the inner loop reads nothing but src[k]
#pragma unroll
    for (int k = 0; k < 9; ++k) { m[k] = L.d[k]; mi[k] = L.d[9 + k]; }
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const float4 p = src[min(i, n - 1)];
        const double yx = R[0] * p.x + R[1] * p.y + R[2] * p.z + tau[0];
        const double yy = R[3] * p.x + R[4] * p.y + R[5] * p.z + tau[1];
        const double yz = R[6] * p.x + R[7] * p.y + R[8] * p.z + tau[2];
        const int zi = __float_as_int(p.w);
        double best = INFINITY;
        int bk = -1;
        for (int k = 0; k < n; ++k) {
            const float4 q = src[k];
            if (__float_as_int(q.w) != zi) continue;
            const double dx = yx - q.x, dy = yy - q.y, dz = yz - q.z;
            const double f2 = mi[6] * dx + mi[7] * dy + mi[8] * dz;      // along n: no wrap
            if (!(fabs(f2) <= symprec)) continue;                       // |reduce(d)| >= |f2|: n is a unit normal of a and b
            double f0 = mi[0] * dx + mi[1] * dy + mi[2] * dz;
            double f1 = mi[3] * dx + mi[4] * dy + mi[5] * dz;
            f0 -= rint(f0);
            f1 -= rint(f1);
            const double ex = m[0] * f0 + m[1] * f1 + m[2] * f2;
            const double ey = m[3] * f0 + m[4] * f1 + m[5] * f2;
            const double ez = m[6] * f0 + m[7] * f1 + m[8] * f2;
            const double d2 = ex * ex + ey * ey + ez * ez;
            if (d2 < best) { best = d2; bk = k; }
        }
        const bool found = best <= s2;
        if (__ballot(i < n && !found) != 0ull) return false;
        if (i < n) partner[i] = bk;
    }
    return true;
}

// R of slot `slot` and tau = x_j - R x_i0 of candidate (slot, j)
__device__ __forceinline__ void sy_candidate(const float4* src, const sy_lat& L, int slot, int j, double (&R)[9], double (&tau)[3]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = SY_R(L, slot, k);
    const float4 o = src[SY_I0(L)], t = src[j];
    tau[0] = (double)t.x - (R[0] * o.x + R[1] * o.y + R[2] * o.z);
    tau[1] = (double)t.y - (R[3] * o.x + R[4] * o.y + R[5] * o.z);
    tau[2] = (double)t.z - (R[6] * o.x + R[7] * o.y + R[8] * o.z);
}

// the slab's lattice record and, when it fits, its atoms into LDS; returns where the atoms are read from
__device__ __forceinline__ const float4* sy_stage(const double* __restrict__ lat_d, const int32_t* __restrict__ lat_i,
                                                  const float4* __restrict__ xz, int b, int a0, int n, sy_lat& L, float4* sh) {
    for (int k = threadIdx.x; k < SY_LATD; k += SY_THREADS) L.d[k] = lat_d[(size_t)b * SY_LATD + k];
    for (int k = threadIdx.x; k < SY_LATI; k += SY_THREADS) L.i[k] = lat_i[(size_t)b * SY_LATI + k];
    if (n <= SY_CAP)
        for (int k = threadIdx.x; k < n; k += SY_THREADS) sh[k] = xz[a0 + k];
    __syncthreads();
    return n <= SY_CAP ? (const float4*)sh : xz + a0;
}

__global__ __launch_bounds__(SY_THREADS) void sy_verify_kernel(
    const int32_t* __restrict__ atom_offset, int num_atoms, double symprec, const double* __restrict__ lat_d,
    const int32_t* __restrict__ lat_i, const float4* __restrict__ xz, int32_t* __restrict__ big_partner,
    int32_t* __restrict__ flags) {
    __shared__ sy_lat L;
    __shared__ float4 sh[SY_CAP];
    __shared__ int32_t sh_partner[SY_WAVES][SY_CAP];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int a0, n;
    adf_segment_clamp(atom_offset, b, num_atoms, a0, n);
    if (n == 0) return;
    const float4* src = sy_stage(lat_d, lat_i, xz, b, a0, n, L, sh);
    const bool big = n > SY_CAP;
    // a slab beyond the LDS: one wave per point slot walks the slot's candidates, the partners in the slot's global row
    if (big && (wave != 0 || blockIdx.y >= SY_SLOTS)) return;
    const long long total = (long long)SY_SLOTS * n;
    long long c = big ? (long long)blockIdx.y * n : (long long)blockIdx.y * SY_WAVES + wave;
    const long long end = big ? c + n : total, step = big ? 1 : (long long)gridDim.y * SY_WAVES;
    for (; c < end; c += step) {
        const int slot = (int)(c / n), j = (int)(c - (long long)slot * n);
        bool ok = SY_BAD(L) == 0 && slot < SY_NW(L) && __float_as_int(src[j].w) == SY_ZR(L);
        if (ok && !(slot == SY_IDENT(L) && j == SY_I0(L))) {                // the identity stands as it is
            int32_t* partner = big ? big_partner + (size_t)SY_SLOTS * a0 + (size_t)slot * n : sh_partner[wave];
            double R[9], tau[3];
            sy_candidate(src, L, slot, j, R, tau);
            ok = sy_match(src, n, L, R, tau, symprec, lane, partner);
            if (ok) {
                __threadfence();                                        // the partners other lanes wrote
                bool twice = false;
                for (int i = lane; i < n; i += 64) {
                    const int mine = partner[i];
                    for (int k = 0; k < n; ++k) twice = twice || (k != i && partner[k] == mine);
                }
                ok = __ballot(twice) == 0ull;
                __threadfence();                                        // read before the next candidate overwrites them
            }
        }
        if (lane == 0) flags[(size_t)SY_SLOTS * a0 + c] = ok ? 1 : 0;
    }
}

// flags -> 1 + rank among the slab's accepted candidates in (slot, j) order; n_ops[b] = their number, -1: slab refused;
// n_ops[B + b] = the slab's atoms
__global__ __launch_bounds__(SY_THREADS) void sy_rank_kernel(const int32_t* __restrict__ atom_offset, int num_atoms, int num_slabs,
                                                             const int32_t* __restrict__ lat_i, int32_t* __restrict__ flags,
                                                             int32_t* __restrict__ n_ops) {
    const int b = blockIdx.x * SY_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= num_slabs) return;
    int a0, n;
    adf_segment_clamp(atom_offset, b, num_atoms, a0, n);
    const long long total = (long long)SY_SLOTS * n;
    int base = 0;
    for (long long c0 = 0; c0 < total; c0 += 64) {
        const long long c = c0 + lane;
        const bool f = c < total && flags[(size_t)SY_SLOTS * a0 + c] != 0;
        const unsigned long long m = __ballot(f);
        if (f) flags[(size_t)SY_SLOTS * a0 + c] = base + __popcll(m & ((1ull << lane) - 1ull)) + 1;
        base += __popcll(m);
    }
    if (lane == 0) {
        n_ops[b] = lat_i[(size_t)b * SY_LATI + 3] != 0 ? -1 : base;
        n_ops[num_slabs + b] = n;                                       // the host sizes perm by it
    }
}

__global__ __launch_bounds__(SY_THREADS) void sy_emit_kernel(
    const int32_t* __restrict__ atom_offset, int num_atoms, double symprec, const double* __restrict__ lat_d,
    const int32_t* __restrict__ lat_i, const float4* __restrict__ xz, const int32_t* __restrict__ flags,
    const int32_t* __restrict__ op_offset, const int64_t* __restrict__ perm_offset, int num_ops, long long perm_len,
    double* __restrict__ rot, double* __restrict__ trans, int32_t* __restrict__ W, int32_t* __restrict__ perm) {
    __shared__ sy_lat L;
    __shared__ float4 sh[SY_CAP];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int a0, n;
    adf_segment_clamp(atom_offset, b, num_atoms, a0, n);
    if (n == 0) return;
    const float4* src = sy_stage(lat_d, lat_i, xz, b, a0, n, L, sh);
    const int o0 = op_offset[b], nops = op_offset[b + 1] - o0;
    const long long p0 = perm_offset[b];
    const long long total = (long long)SY_SLOTS * n, ident = (long long)SY_IDENT(L) * n + SY_I0(L);
    for (long long c = (long long)blockIdx.y * SY_WAVES + wave; c < total; c += (long long)gridDim.y * SY_WAVES) {
        const int f = flags[(size_t)SY_SLOTS * a0 + c];
        if (f == 0) continue;
        // the identity goes first, the others keep their order
        const int k = c == ident ? 0 : c < ident ? f : f - 1;
        if (o0 < 0 || k >= nops || o0 + k >= num_ops || p0 < 0 || p0 + ((long long)k + 1) * n > perm_len) continue;
        const int slot = (int)(c / n), j = (int)(c - (long long)slot * n);
        double R[9], tau[3];
        int32_t* out = perm + p0 + (long long)k * n;
        if (c == ident) {
#pragma unroll
            for (int q = 0; q < 9; ++q) R[q] = q % 4 == 0 ? 1.0 : 0.0;
            tau[0] = tau[1] = tau[2] = 0.0;
            for (int i = lane; i < n; i += 64) out[i] = i;
        } else {
            sy_candidate(src, L, slot, j, R, tau);
            (void)sy_match(src, n, L, R, tau, symprec, lane, out);
        }
        if (lane == 0) {
            const size_t g = (size_t)(o0 + k);
#pragma unroll
            for (int q = 0; q < 9; ++q) rot[9 * g + q] = R[q];
#pragma unroll
            for (int q = 0; q < 3; ++q) trans[3 * g + q] = tau[q];
#pragma unroll
            for (int q = 0; q < 4; ++q) W[4 * g + q] = SY_W(L, slot, q);
        }
    }
}

// ---- host side
struct sy_scratch {
    double* lat_d;
    int32_t* lat_i;
    float4* xz;
    int32_t* flags;
    int32_t* big_partner;
    size_t bytes;
};

// the layout of the caller's scratch, every region on a 256-byte boundary; a null scratch measures it (s.bytes)
static sy_scratch sy_carve(void* scratch, int32_t num_atoms, int32_t num_slabs) {
    adf_carver c(scratch, 256);
    sy_scratch s;
    s.lat_d = c.take<double>((size_t)num_slabs * SY_LATD);
    s.lat_i = c.take<int32_t>((size_t)num_slabs * SY_LATI);
    s.xz = c.take<float4>((size_t)num_atoms);
    s.flags = c.take<int32_t>((size_t)num_atoms * SY_SLOTS);
    s.big_partner = c.take<int32_t>((size_t)num_atoms * SY_SLOTS);
    s.bytes = c.bytes();
    return s;
}

extern "C" int64_t adf_slab_symmetry_scratch(int32_t num_atoms, int32_t num_slabs) {
    if (num_atoms < 0 || num_slabs < 0) return 0;
    return (int64_t)sy_carve(nullptr, num_atoms, num_slabs).bytes;
}

// blocks per slab: about four candidates per wave of the average slab; at least one block per point slot (large slabs)
static int sy_blocks_per_slab(int32_t num_atoms, int32_t num_slabs) {
    const long long avg = ((long long)num_atoms + num_slabs - 1) / num_slabs;
    const long long y = (SY_SLOTS * avg + 4 * SY_WAVES - 1) / (4 * SY_WAVES);
    return (int)(y < SY_SLOTS ? SY_SLOTS : y > 1024 ? 1024 : y);
}

extern "C" int32_t adf_slab_symmetry_search(const float* pos, const float* cell, const int32_t* atomic_numbers,
                                            const int32_t* atom_offset, int32_t num_atoms, int32_t num_slabs, double symprec,
                                            int32_t proper_only, void* scratch, int32_t* n_ops, int32_t* n_ops_host,
                                            void* stream) {
    if (!pos || !cell || !atomic_numbers || !atom_offset || !scratch || !n_ops || !n_ops_host) {
        adf_set_error("slab_symmetry_search: null argument");
        return ADF_EINVAL;
    }
    if (num_atoms <= 0 || num_slabs <= 0 || !(symprec >= 0.0) || !(symprec < 1e30)) {
        adf_set_error("slab_symmetry_search: %d atoms, %d slabs, symprec %g", num_atoms, num_slabs, symprec);
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const sy_scratch w = sy_carve(scratch, num_atoms, num_slabs);
    const int per_wave = (num_slabs + SY_WAVES - 1) / SY_WAVES;
    hipLaunchKernelGGL(sy_lattice_kernel, dim3(per_wave), dim3(SY_THREADS), 0, s, pos, cell, atomic_numbers, atom_offset,
                       num_atoms, num_slabs, symprec, proper_only, w.lat_d, w.lat_i, w.xz);
    ADF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sy_verify_kernel, dim3(num_slabs, sy_blocks_per_slab(num_atoms, num_slabs)), dim3(SY_THREADS), 0, s,
                       atom_offset, num_atoms, symprec, w.lat_d, w.lat_i, w.xz, w.big_partner, w.flags);
    ADF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sy_rank_kernel, dim3(per_wave), dim3(SY_THREADS), 0, s, atom_offset, num_atoms, num_slabs, w.lat_i,
                       w.flags, n_ops);
    ADF_HIP_CHECK(hipGetLastError());
    // the one read-back: the counts size the outputs
    ADF_HIP_CHECK(hipMemcpyAsync(n_ops_host, n_ops, 2 * (size_t)num_slabs * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ADF_HIP_CHECK(hipStreamSynchronize(s));
    for (int32_t b = 0; b < num_slabs; ++b)
        if (n_ops_host[b] < 0) {
            adf_set_error("slab_symmetry_search: slab %d: symprec %g is not below half the shortest in-plane lattice height "
                          "(or the cell's first two rows span no finite area)", b, symprec);
            return ADF_EINVAL;
        }
    return ADF_OK;
}

extern "C" int32_t adf_slab_symmetry_emit(const int32_t* atom_offset, int32_t num_atoms, int32_t num_slabs, double symprec,
                                          const void* scratch, const int32_t* op_offset, const int64_t* perm_offset,
                                          int32_t num_ops, int64_t perm_len, double* rot, double* trans, int32_t* W,
                                          int32_t* perm, void* stream) {
    if (!atom_offset || !scratch || !op_offset || !perm_offset || !rot || !trans || !W || !perm) {
        adf_set_error("slab_symmetry_emit: null argument");
        return ADF_EINVAL;
    }
    if (num_atoms <= 0 || num_slabs <= 0 || num_ops <= 0 || perm_len <= 0) {
        adf_set_error("slab_symmetry_emit: %d atoms, %d slabs, %d operations, %lld permutation entries", num_atoms, num_slabs,
                      num_ops, (long long)perm_len);
        return ADF_EINVAL;
    }
    const sy_scratch w = sy_carve(const_cast<void*>(scratch), num_atoms, num_slabs);
    hipLaunchKernelGGL(sy_emit_kernel, dim3(num_slabs, sy_blocks_per_slab(num_atoms, num_slabs)), dim3(SY_THREADS), 0,
                       (hipStream_t)stream, atom_offset, num_atoms, symprec, w.lat_d, w.lat_i, w.xz, w.flags, op_offset,
                       perm_offset, num_ops, (long long)perm_len, rot, trans, W, perm);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}
