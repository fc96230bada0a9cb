// Surface tags: Voronoi coordination numbers of the atoms of a batch - pymatgen's
// VoronoiNN(tol).get_cn(use_weights=True), a qhull call per atom in the reference - the bulk table made of them and the tags
// of tag_surface_atoms [the reference's placement/slab.py:284-482].  The contract is in include/adsorbdiff_hip.h.
//
// All arithmetic is float64 on float32 inputs.  No float atomics; the integer atomics are the OR on the error word and the
// MIN on the atom it names.  Every output row has one writer: two calls give the same bits, and nothing a system gets
// depends on its batch-mates.  Results go to scratch rows first and a last kernel copies them out where the error word is
// still zero, so an error leaves the outputs alone.
//
// vo_cell_kernel: workgroups (system, part) of ONE wave, a wave per selected atom.  The wave gathers the atom's candidates
// into LDS in (atom, image) order [ballot prefix], sorts (|d|^2, slot) with a bitonic network and puts the vectors in that
// order.  Then rounds over the K nearest: lane j clips the square on the bisector plane of candidate j by every other
// candidate [Sutherland-Hodgman], its vertices as in-plane (s, t) pairs in LDS, ping-pong, lane-minor so that the lanes of a
// wave touch consecutive words [a runtime-indexed register array would go to scratch]; 64 facets at a time, so the LDS holds
// 64 polygons whatever K is.  A clip that cuts nothing is skipped after one pass over the vertices, which leaves them bit for
// bit.  The wave maximum of the vertex radius decides whether candidate K can still cut [the security radius]; if so K
// doubles and the cell is built again.  LDS: 36 KiB of candidates, 8 KiB of solid angles, 64 KiB of polygons - one wave per CU
// at a time.
#include <float.h>
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "host_util.h"
#include "cell3.h"
#include "lanes.h"

#define VO_CAND 1024            // candidates of one atom held in LDS
#define VO_VERT 32              // vertices of a facet while it is clipped
#define VO_SQUARE 1e4           // half-width of the square a facet starts from [A]
#define VO_MAX_PAIRS (1 << 24)  // (atom, image) pairs one wave looks at
#define VO_Z 119                // atomic numbers 0 .. 118

enum {
    VO_ERR_RANGE = 1, VO_ERR_CELL = 2, VO_ERR_CAND = 4, VO_ERR_VERT = 8, VO_ERR_PAIRS = 16, VO_ERR_FLAGGED = 32,
    VO_ERR_Z = 64, VO_ERR_ELEMENT = 128, VO_ERR_MASS = 256
};

struct vo_cell3 { double a[3], b[3], c[3]; };

__device__ __forceinline__ vo_cell3 vo_load_cell(const float* cell, int b) {
    vo_cell3 q;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        q.a[k] = (double)cell[9 * (size_t)b + k];
        q.b[k] = (double)cell[9 * (size_t)b + 3 + k];
        q.c[k] = (double)cell[9 * (size_t)b + 6 + k];
    }
    return q;
}
__device__ __forceinline__ bool vo_finite(double v) { return fabs(v) < INFINITY; }

__device__ __forceinline__ void vo_fail(int32_t* err, int bit, int atom) {
    atomicOr(err, bit);
    atomicMin(err + 1, atom);
}

// ------------------------------------------------------------------------------------------------ per-system preparation
// reps [B,4]: the repeats along a, b, c and 1 where the system may be evaluated
__global__ void vo_prepare_kernel(const float* __restrict__ cell, const int32_t* __restrict__ pbc,
                                  const int32_t* __restrict__ atom_offset, int N, int B, double cutoff, int cell_always,
                                  int32_t* __restrict__ reps, int32_t* err) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int32_t r[4] = {0, 0, 0, 0};
    const int a0 = atom_offset[b], a1 = atom_offset[b + 1];
    if (a0 < 0 || a1 < a0 || a1 > N) {
        atomicOr(err, VO_ERR_RANGE);
    } else {
        const bool per[3] = {pbc[3 * (size_t)b] != 0, pbc[3 * (size_t)b + 1] != 0, pbc[3 * (size_t)b + 2] != 0};
        bool ok = true;
        if (per[0] || per[1] || per[2] || cell_always) {
            const vo_cell3 q = vo_load_cell(cell, b);
            double bc[3], ca[3], ab[3];
            adf_cross3(q.b, q.c, bc);
            adf_cross3(q.c, q.a, ca);
            adf_cross3(q.a, q.b, ab);
            const double vol = fabs(adf_dot3(q.a, bc));
            const double area[3] = {sqrt(adf_dot3(bc, bc)), sqrt(adf_dot3(ca, ca)), sqrt(adf_dot3(ab, ab))};
            if (!(vol > 0.0) || !vo_finite(vol) || !vo_finite(area[0]) || !vo_finite(area[1]) || !vo_finite(area[2])) {
                ok = false;
                vo_fail(err, VO_ERR_CELL, a0);
            } else {
                double pairs = (double)max(a1 - a0, 1);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double want = per[k] ? ceil(cutoff / (vol / area[k])) : 0.0;
                    pairs *= 2.0 * want + 1.0;
                    r[k] = want < 1e6 ? (int32_t)want : 0;
                }
                if (!(pairs <= (double)VO_MAX_PAIRS)) {
                    ok = false;
                    vo_fail(err, VO_ERR_PAIRS, a0);
                }
            }
        }
        r[3] = ok ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) reps[4 * (size_t)b + k] = r[k];
}

// ------------------------------------------------------------------------------------------------ the cell of one atom
struct vo_params {
    const float* pos; const float* cell; const int32_t* atom_offset; const int32_t* select; const int32_t* reps;
    int32_t N;
    double cutoff, weight_tol, far;
    double* cn; double* omega_max; int32_t* nn; int32_t* flags; int32_t* err;
};

__global__ __launch_bounds__(64) void vo_cell_kernel(vo_params q) {
    __shared__ double cx[VO_CAND], cy[VO_CAND], cz[VO_CAND], key[VO_CAND], om[VO_CAND];
    __shared__ int perm[VO_CAND];
    __shared__ double2 poly[2 * VO_VERT * 64];              // [buffer][vertex][lane]
    const int b = blockIdx.x, lane = threadIdx.x;
    if (q.reps[4 * (size_t)b + 3] == 0) return;             // refused by the preparation: the error word says why
    const int a0 = q.atom_offset[b], a1 = q.atom_offset[b + 1], n = a1 - a0;
    const int ra = q.reps[4 * (size_t)b], rb = q.reps[4 * (size_t)b + 1], rc = q.reps[4 * (size_t)b + 2];
    const int nb = 2 * rb + 1, nc = 2 * rc + 1, nimg = (2 * ra + 1) * nb * nc;
    const int total = n * nimg;                             // at most VO_MAX_PAIRS
    vo_cell3 L = {};
    if (nimg > 1) L = vo_load_cell(q.cell, b);
    double2* mine = poly + lane;
    for (int i = a0 + (int)blockIdx.y; i < a1; i += (int)gridDim.y) {
        if (q.select && q.select[i] == 0) continue;
        const double px = (double)q.pos[3 * (size_t)i], py = (double)q.pos[3 * (size_t)i + 1], pz = (double)q.pos[3 * (size_t)i + 2];
        __syncthreads();                                    // the previous atom's reads of the LDS are done
        // ---- candidates, in (atom, image) order
        int count = 0;
        for (int base = 0; base < total && count <= VO_CAND; base += 64) {
            const int e = base + lane;
            bool ok = false;
            double dx = 0.0, dy = 0.0, dz = 0.0, d2 = 0.0;
            if (e < total) {
                const int j = e / nimg, img = e - j * nimg;
                const double ia = (double)(img / (nb * nc) - ra), ib = (double)((img / nc) % nb - rb), ic = (double)(img % nc - rc);
                const float* pj = q.pos + 3 * (size_t)(a0 + j);
                dx = ((double)pj[0] + ((ia * L.a[0] + ib * L.b[0]) + ic * L.c[0])) - px;
                dy = ((double)pj[1] + ((ia * L.a[1] + ib * L.b[1]) + ic * L.c[1])) - py;
                dz = ((double)pj[2] + ((ia * L.a[2] + ib * L.b[2]) + ic * L.c[2])) - pz;
                d2 = dx * dx + dy * dy + dz * dz;
                ok = d2 > 1e-16 && sqrt(d2) <= q.cutoff;
            }
            const unsigned long long m = __ballot(ok);
            const int slot = count + __popcll(m & ((1ull << lane) - 1ull));
            if (ok && slot < VO_CAND) {
                cx[slot] = dx; cy[slot] = dy; cz[slot] = dz; key[slot] = d2; perm[slot] = slot;
            }
            count += __popcll(m);
        }
        if (count > VO_CAND) {
            if (lane == 0) vo_fail(q.err, VO_ERR_CAND, i);
            continue;
        }
        if (count == 0) {                                   // nothing closes the cell
            if (lane == 0) { q.cn[i] = NAN; q.omega_max[i] = NAN; q.nn[i] = 0; q.flags[i] = 1; }
            continue;
        }
        // ---- sort (|d|^2, slot): bitonic over the next power of two, padded with +inf
        int npad = 64;
        while (npad < count) npad <<= 1;
        for (int t = count + lane; t < npad; t += 64) { key[t] = INFINITY; perm[t] = t; }
        __syncthreads();
        for (int k = 2; k <= npad; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = lane; t < npad; t += 64) {
                    const int x = t ^ j;
                    if (x > t) {
                        const double ka = key[t], kb = key[x];
                        const int pa = perm[t], pb = perm[x];
                        const bool gt = ka > kb || (ka == kb && pa > pb);
                        if (gt == ((t & k) == 0)) { key[t] = kb; key[x] = ka; perm[t] = pb; perm[x] = pa; }
                    }
                }
                __syncthreads();
            }
        }
        // the vectors in that order [through the polygon buffers, which are free here]
        double* tmp = reinterpret_cast<double*>(poly);
        for (int t = lane; t < count; t += 64) {
            const int p = perm[t];
            tmp[3 * t] = cx[p]; tmp[3 * t + 1] = cy[p]; tmp[3 * t + 2] = cz[p];
        }
        __syncthreads();
        for (int t = lane; t < count; t += 64) { cx[t] = tmp[3 * t]; cy[t] = tmp[3 * t + 1]; cz[t] = tmp[3 * t + 2]; }
        __syncthreads();
        // ---- the cell from the K nearest, K doubled until the next candidate cannot cut it
        int K = min(count, 64);
        double R = 0.0;
        bool over = false;
        for (;;) {
            double rmax = 0.0;
            for (int chunk = 0; chunk < K; chunk += 64) {
                const int j = chunk + lane;
                double omega = 0.0;
                if (j < K) {
                    const double d[3] = {cx[j], cy[j], cz[j]};
                    const double r = sqrt(key[j]);
                    const double nrm[3] = {d[0] / r, d[1] / r, d[2] / r};
                    const double o[3] = {0.5 * d[0], 0.5 * d[1], 0.5 * d[2]};
                    const bool ex = fabs(nrm[0]) < 0.9;
                    const double e[3] = {ex ? 1.0 : 0.0, ex ? 0.0 : 1.0, 0.0};
                    double u[3], v[3];
                    adf_cross3(nrm, e, u);
                    const double ul = sqrt(adf_dot3(u, u));
                    u[0] /= ul; u[1] /= ul; u[2] /= ul;
                    adf_cross3(nrm, u, v);
                    int cur = 0, cnt = 4;
                    mine[0 * 64] = make_double2(-VO_SQUARE, -VO_SQUARE);
                    mine[1 * 64] = make_double2(VO_SQUARE, -VO_SQUARE);
                    mine[2 * 64] = make_double2(VO_SQUARE, VO_SQUARE);
                    mine[3 * 64] = make_double2(-VO_SQUARE, VO_SQUARE);
                    for (int k = 0; k < K && cnt >= 3; ++k) {
                        if (k == j) continue;
                        const double dk[3] = {cx[k], cy[k], cz[k]};
                        const double c0 = adf_dot3(o, dk) - 0.5 * key[k], cu = adf_dot3(u, dk), cv = adf_dot3(v, dk);
                        const double2* src = mine + cur * (VO_VERT * 64);
                        bool cuts = false;
                        for (int a = 0; a < cnt; ++a) {
                            const double2 p = src[a * 64];
                            cuts = cuts || !(c0 + cu * p.x + cv * p.y <= 0.0);
                        }
                        if (!cuts) continue;
                        double2* dst = mine + (cur ^ 1) * (VO_VERT * 64);
                        int out = 0;
                        double2 pa = src[0];
                        double sa = c0 + cu * pa.x + cv * pa.y;
                        for (int a = 0; a < cnt; ++a) {
                            const double2 pb = src[(a + 1 < cnt ? a + 1 : 0) * 64];
                            const double sb = c0 + cu * pb.x + cv * pb.y;
                            const bool ina = sa <= 0.0, inb = sb <= 0.0;
                            if (ina) {
                                if (out < VO_VERT) dst[out * 64] = pa;
                                ++out;
                            }
                            if (ina != inb) {
                                const double t = sa / (sa - sb);
                                if (out < VO_VERT) dst[out * 64] = make_double2(pa.x + t * (pb.x - pa.x), pa.y + t * (pb.y - pa.y));
                                ++out;
                            }
                            pa = pb;
                            sa = sb;
                        }
                        if (out > VO_VERT) { over = true; out = 0; }
                        cnt = out;
                        cur ^= 1;
                    }
                    if (cnt >= 3) {
                        const double2* src = mine + cur * (VO_VERT * 64);
                        double P0[3], Pb[3], lb = 0.0, l0 = 0.0, tot = 0.0;
                        for (int a = 0; a < cnt; ++a) {
                            const double2 p = src[a * 64];
                            const double Pc[3] = {o[0] + p.x * u[0] + p.y * v[0], o[1] + p.x * u[1] + p.y * v[1],
                                                  o[2] + p.x * u[2] + p.y * v[2]};
                            const double lc = sqrt(adf_dot3(Pc, Pc));
                            rmax = fmax(rmax, lc);
                            if (a == 0) {
                                P0[0] = Pc[0]; P0[1] = Pc[1]; P0[2] = Pc[2]; l0 = lc;
                            } else if (a >= 2) {
                                double bxc[3];
                                adf_cross3(Pb, Pc, bxc);
                                const double num = adf_dot3(P0, bxc);
                                const double den = l0 * lb * lc + adf_dot3(P0, Pb) * lc + adf_dot3(P0, Pc) * lb + adf_dot3(Pb, Pc) * l0;
                                tot += 2.0 * atan2(num, den);
                            }
                            Pb[0] = Pc[0]; Pb[1] = Pc[1]; Pb[2] = Pc[2]; lb = lc;
                        }
                        omega = fabs(tot);
                    }
                    om[j] = omega;
                }
            }
            R = adf_wave_max(rmax);
            if (__any(over)) break;
            if (K == count || sqrt(key[K]) > 2.0 * R) break;
            K = min(count, 2 * K);
        }
        if (__any(over)) {
            if (lane == 0) vo_fail(q.err, VO_ERR_VERT, i);
            continue;
        }
        __syncthreads();                                    // every lane's om is written
        double omax = 0.0;
        for (int j = lane; j < K; j += 64) omax = fmax(omax, om[j]);
        omax = adf_wave_max(omax);
        if (R > q.far || !(omax > 0.0)) {                   // open [no facet at all cannot happen: the nearest has one]
            if (lane == 0) { q.cn[i] = NAN; q.omega_max[i] = NAN; q.nn[i] = 0; q.flags[i] = 1; }
            continue;
        }
        double cn = 0.0;                                    // in candidate order, the same in every lane
        int nn = 0;
        for (int j = 0; j < K; ++j) {
            const double w = om[j] / omax;
            if (w > q.weight_tol) { cn += w; ++nn; }
        }
        if (lane == 0) { q.cn[i] = cn; q.omega_max[i] = omax; q.nn[i] = nn; q.flags[i] = 0; }
    }
}

// ------------------------------------------------------------------------------------------------ results -> outputs
__global__ void vo_commit_kernel(const int32_t* __restrict__ select, int N, const double* __restrict__ r_cn,
                                 const double* __restrict__ r_om, const int32_t* __restrict__ r_nn,
                                 const int32_t* __restrict__ r_fl, double* __restrict__ cn, double* __restrict__ omega_max,
                                 int32_t* __restrict__ nn, int32_t* __restrict__ flags, const int32_t* err) {
    if (*err != 0) return;                                  // written by the kernels before this one
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || (select && select[i] == 0)) return;
    cn[i] = r_cn[i];
    omega_max[i] = r_om[i];
    nn[i] = r_nn[i];
    flags[i] = r_fl[i];
}

// ------------------------------------------------------------------------------------------------ the bulk table
__global__ void vo_bulk_check_kernel(const double* __restrict__ cn, const int32_t* __restrict__ flags,
                                     const int32_t* __restrict__ Z, const int32_t* __restrict__ atom_offset, int N, int B,
                                     int32_t* err) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < B) {
        const int a0 = atom_offset[t], a1 = atom_offset[t + 1];
        if (a0 < 0 || a1 < a0 || a1 > N) atomicOr(err, VO_ERR_RANGE);
    }
    if (t < N) {
        if (flags[t] != 0 || !vo_finite(cn[t])) vo_fail(err, VO_ERR_FLAGGED, t);
        if (Z[t] < 0 || Z[t] >= VO_Z) vo_fail(err, VO_ERR_Z, t);
    }
}
// one workgroup of 128 per system: thread z takes element z, the atoms in order
__global__ void vo_bulk_min_kernel(const double* __restrict__ cn, const int32_t* __restrict__ Z,
                                   const int32_t* __restrict__ atom_offset, double* __restrict__ table, const int32_t* err) {
    if (*err != 0) return;
    const int b = blockIdx.x, z = threadIdx.x;
    if (z >= VO_Z) return;
    double least = INFINITY;
    for (int i = atom_offset[b]; i < atom_offset[b + 1]; ++i)
        if (Z[i] == z) least = fmin(least, cn[i]);
    table[VO_Z * (size_t)b + z] = least;
}

// ------------------------------------------------------------------------------------------------ the tagging rules
struct vo_tag_params {
    const float* pos; const float* cell; const int32_t* pbc; const int32_t* Z; const int32_t* atom_offset;
    const double* masses; const double* bulk; const int32_t* reps;
    double height;
    double* f; int32_t* tag0; int32_t* sel; int32_t* err;
};
// one wave per system: fractional heights, the height rule, the centre of mass, who is evaluated
__global__ __launch_bounds__(64) void vo_tag_prepare_kernel(vo_tag_params q) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (q.reps[4 * (size_t)b + 3] == 0) return;
    const int a0 = q.atom_offset[b], a1 = q.atom_offset[b + 1];
    const vo_cell3 L = vo_load_cell(q.cell, b);
    double axb[3];
    adf_cross3(L.a, L.b, axb);
    const double vol = adf_dot3(L.c, axb), clen = sqrt(adf_dot3(L.c, L.c));
    const bool wrap = q.pbc[3 * (size_t)b + 2] != 0;
    double fmx = -INFINITY;
    bool badz = false;
    for (int i = a0 + lane; i < a1; i += 64) {
        const double p[3] = {(double)q.pos[3 * (size_t)i], (double)q.pos[3 * (size_t)i + 1], (double)q.pos[3 * (size_t)i + 2]};
        double f = adf_dot3(p, axb) / vol;
        if (wrap) {
            f -= floor(f);
            f -= floor(f);
        }
        q.f[i] = f;
        fmx = fmax(fmx, f);
        if (q.Z[i] < 0 || q.Z[i] >= VO_Z) {
            badz = true;
            vo_fail(q.err, VO_ERR_Z, i);
        }
    }
    if (__any(badz)) return;
    fmx = adf_wave_max(fmx);
    __syncthreads();                                        // f of this system is written [one wave: its own stores]
    double sm = 0.0, smf = 0.0;                             // in atom order, the same in every lane
    for (int i = a0; i < a1; ++i) {
        const double m = q.masses[q.Z[i]];
        sm += m;
        smf += m * q.f[i];
    }
    if (a1 > a0 && !(sm > 0.0 && vo_finite(sm))) {
        if (lane == 0) vo_fail(q.err, VO_ERR_MASS, a0);
        return;
    }
    const double f_com = smf / sm, thr = fmx - q.height / clen;
    for (int i = a0 + lane; i < a1; i += 64) {
        const double f = q.f[i];
        const int t0 = !(f < thr) ? 1 : 0;
        q.tag0[i] = t0;
        int s = 0;
        if (q.bulk) {
            const double least = q.bulk[VO_Z * (size_t)b + q.Z[i]];
            if (!vo_finite(least)) vo_fail(q.err, VO_ERR_ELEMENT, i);
            s = (t0 == 0 && !(f < f_com)) ? 1 : 0;
        }
        q.sel[i] = s;
    }
}
__global__ void vo_tag_commit_kernel(const int32_t* __restrict__ tag0, const int32_t* __restrict__ sel,
                                     const double* __restrict__ r_cn, const int32_t* __restrict__ r_fl,
                                     const double* __restrict__ bulk, const int32_t* __restrict__ Z,
                                     const int32_t* __restrict__ atom_offset, int N, int B, double cn_tol,
                                     int32_t* __restrict__ tags, double* __restrict__ cn, int32_t* __restrict__ flags,
                                     const int32_t* err) {
    if (*err != 0) return;
    const int b = blockIdx.x;
    for (int i = atom_offset[b] + (int)threadIdx.x; i < atom_offset[b + 1]; i += (int)blockDim.x) {
        int t = tag0[i];
        double c = NAN;
        int fl = 0;
        if (sel[i]) {
            c = r_cn[i];
            fl = r_fl[i];
            if ((fl & 1) || c < bulk[VO_Z * (size_t)b + Z[i]] - cn_tol) t = 1;
        }
        tags[i] = t;
        cn[i] = c;
        flags[i] = fl;
    }
}

// ------------------------------------------------------------------------------------------------ host side
static bool vo_positive(double v) { return v > 0.0 && v < (double)INFINITY; }

static const adf_errrow VO_ERRORS[] = {
    {VO_ERR_RANGE, ADF_EINVAL, "%s: atom offsets not ascending or outside [0, N]"},
    {VO_ERR_CELL, ADF_EINVAL, "%s: the cell of the system of atom %d is singular or not finite", ADF_ERR_ATOM},
    {VO_ERR_Z, ADF_EINVAL, "%s: atom %d has an atomic number outside [0, 118]", ADF_ERR_ATOM},
    {VO_ERR_MASS, ADF_EINVAL, "%s: the masses of the system of atom %d do not sum to a positive number", ADF_ERR_ATOM},
    {VO_ERR_ELEMENT, ADF_EINVAL, "%s: the element of atom %d is absent from its slab's row of the bulk table", ADF_ERR_ATOM},
    {VO_ERR_FLAGGED, ADF_EINVAL, "%s: atom %d has an open cell or no coordination number (a bulk is periodic in three directions)",
     ADF_ERR_ATOM},
    {VO_ERR_PAIRS, ADF_EOVERFLOW, "%s: the system of atom %d has more than %d (atom, image) pairs within the cutoff's repeats",
     ADF_ERR_ATOM, VO_MAX_PAIRS},
    {VO_ERR_CAND, ADF_EOVERFLOW, "%s: atom %d has more than %d candidates within the cutoff", ADF_ERR_ATOM, VO_CAND},
    {VO_ERR_VERT, ADF_EOVERFLOW, "%s: a facet of atom %d needs more than %d vertices", ADF_ERR_ATOM, VO_VERT}};

static int32_t vo_launch_cells(vo_params q, int num_atoms, int num_systems, hipStream_t s) {
    // workgroups per system: a wave per atom, sized by the mean system (a system's rows do not depend on it)
    const int parts = (int)std::min(256ll, std::max(1ll, (long long)num_atoms / num_systems));
    hipLaunchKernelGGL(vo_cell_kernel, dim3(num_systems, parts), dim3(64), 0, s, q);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}

extern "C" int32_t adf_voronoi_coordination(const float* pos, const float* cell, const int32_t* pbc, const int32_t* atom_offset,
                                            int32_t num_atoms, int32_t num_systems, const int32_t* select, double cutoff,
                                            double weight_tol, double far, double* cn, double* omega_max, int32_t* nn,
                                            int32_t* flags, void* stream) {
    if (!pos || !cell || !pbc || !atom_offset || !cn || !omega_max || !nn || !flags) {
        adf_set_error("voronoi_coordination: null argument");
        return ADF_EINVAL;
    }
    if (num_atoms < 0 || num_systems <= 0) {
        adf_set_error("voronoi_coordination: %d atoms, %d systems", num_atoms, num_systems);
        return ADF_EINVAL;
    }
    if (!vo_positive(cutoff) || !vo_positive(weight_tol) || !vo_positive(far)) {
        adf_set_error("voronoi_coordination: cutoff, weight_tol and far must be finite and positive");
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)num_atoms, B = (size_t)num_systems;
    // one scratch block, freed on every return (after the synchronisation in finish): laid out by the same code twice
    double *r_cn, *r_om;
    int32_t *r_nn, *r_fl, *reps, *err_dev;
    auto lay = [&](adf_carver c) {
        r_cn = c.take<double>(N); r_om = c.take<double>(N);
        r_nn = c.take<int32_t>(N); r_fl = c.take<int32_t>(N); reps = c.take<int32_t>(4 * B); err_dev = c.take<int32_t>(2);
        return c.bytes();
    };
    adf_pool tmp;
    void* block = nullptr;
    ADF_TRY(tmp.alloc(&block, lay(adf_carver())));
    lay(adf_carver(block));
    adf_errword err;
    ADF_TRY(err.adopt(err_dev, s, 2));
    hipLaunchKernelGGL(vo_prepare_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, cell, pbc, atom_offset, num_atoms,
                       num_systems, cutoff, 0, reps, err.dev);
    ADF_HIP_CHECK(hipGetLastError());
    vo_params q = {};
    q.pos = pos; q.cell = cell; q.atom_offset = atom_offset; q.select = select; q.reps = reps; q.N = num_atoms;
    q.cutoff = cutoff; q.weight_tol = weight_tol; q.far = far;
    q.cn = r_cn; q.omega_max = r_om; q.nn = r_nn; q.flags = r_fl; q.err = err.dev;
    if (num_atoms > 0) {
        ADF_TRY(vo_launch_cells(q, num_atoms, num_systems, s));
        hipLaunchKernelGGL(vo_commit_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, select, num_atoms, r_cn, r_om,
                           r_nn, r_fl, cn, omega_max, nn, flags, err.dev);
        ADF_HIP_CHECK(hipGetLastError());
    }
    return err.finish(s, "voronoi_coordination", VO_ERRORS);
}

extern "C" int32_t adf_bulk_coordination_min(const double* cn, const int32_t* flags, const int32_t* atomic_numbers,
                                             const int32_t* atom_offset, int32_t num_atoms, int32_t num_systems, double* table,
                                             void* stream) {
    if (!cn || !flags || !atomic_numbers || !atom_offset || !table) {
        adf_set_error("bulk_coordination_min: null argument");
        return ADF_EINVAL;
    }
    if (num_atoms < 0 || num_systems <= 0) {
        adf_set_error("bulk_coordination_min: %d atoms, %d systems", num_atoms, num_systems);
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    adf_errword err;   // freed on every return (after the synchronisation in finish)
    ADF_TRY(err.create(s, 2));
    const int most = std::max(num_atoms, num_systems);
    hipLaunchKernelGGL(vo_bulk_check_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, s, cn, flags, atomic_numbers,
                       atom_offset, num_atoms, num_systems, err.dev);
    ADF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(vo_bulk_min_kernel, dim3(num_systems), dim3(128), 0, s, cn, atomic_numbers, atom_offset, table, err.dev);
    ADF_HIP_CHECK(hipGetLastError());
    return err.finish(s, "bulk_coordination_min", VO_ERRORS);
}

extern "C" int32_t adf_tag_surface_atoms(const float* pos, const float* cell, const int32_t* pbc, const int32_t* atomic_numbers,
                                         const int32_t* atom_offset, int32_t num_atoms, int32_t num_systems,
                                         const double* masses, const double* bulk_cn_min, double height, double cutoff,
                                         double weight_tol, double far, double cn_tol, int32_t* tags, double* cn,
                                         int32_t* flags, void* stream) {
    if (!pos || !cell || !pbc || !atomic_numbers || !atom_offset || !masses || !tags || !cn || !flags) {
        adf_set_error("tag_surface_atoms: null argument");
        return ADF_EINVAL;
    }
    if (num_atoms < 0 || num_systems <= 0) {
        adf_set_error("tag_surface_atoms: %d atoms, %d systems", num_atoms, num_systems);
        return ADF_EINVAL;
    }
    if (!vo_positive(cutoff) || !vo_positive(weight_tol) || !vo_positive(far)) {
        adf_set_error("tag_surface_atoms: cutoff, weight_tol and far must be finite and positive");
        return ADF_EINVAL;
    }
    if (!(height >= 0.0) || !(height < (double)INFINITY) || !(cn_tol >= 0.0) || !(cn_tol < (double)INFINITY)) {
        adf_set_error("tag_surface_atoms: height and cn_tol must be finite and not negative");
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)num_atoms, B = (size_t)num_systems;
    double *r_cn, *r_om, *f;
    int32_t *r_nn, *r_fl, *tag0, *sel, *reps, *err_dev;
    auto lay = [&](adf_carver c) {
        r_cn = c.take<double>(N); r_om = c.take<double>(N); f = c.take<double>(N);
        r_nn = c.take<int32_t>(N); r_fl = c.take<int32_t>(N); tag0 = c.take<int32_t>(N); sel = c.take<int32_t>(N);
        reps = c.take<int32_t>(4 * B); err_dev = c.take<int32_t>(2);
        return c.bytes();
    };
    adf_pool tmp;
    void* block = nullptr;
    ADF_TRY(tmp.alloc(&block, lay(adf_carver())));
    lay(adf_carver(block));
    adf_errword err;
    ADF_TRY(err.adopt(err_dev, s, 2));
    hipLaunchKernelGGL(vo_prepare_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, cell, pbc, atom_offset, num_atoms,
                       num_systems, cutoff, 1, reps, err.dev);
    ADF_HIP_CHECK(hipGetLastError());
    vo_tag_params t = {};
    t.pos = pos; t.cell = cell; t.pbc = pbc; t.Z = atomic_numbers; t.atom_offset = atom_offset; t.masses = masses;
    t.bulk = bulk_cn_min; t.reps = reps; t.height = height; t.f = f; t.tag0 = tag0; t.sel = sel; t.err = err.dev;
    hipLaunchKernelGGL(vo_tag_prepare_kernel, dim3(num_systems), dim3(64), 0, s, t);
    ADF_HIP_CHECK(hipGetLastError());
    if (bulk_cn_min && num_atoms > 0) {
        vo_params q = {};
        q.pos = pos; q.cell = cell; q.atom_offset = atom_offset; q.select = sel; q.reps = reps; q.N = num_atoms;
        q.cutoff = cutoff; q.weight_tol = weight_tol; q.far = far;
        q.cn = r_cn; q.omega_max = r_om; q.nn = r_nn; q.flags = r_fl; q.err = err.dev;
        ADF_TRY(vo_launch_cells(q, num_atoms, num_systems, s));
    }
    hipLaunchKernelGGL(vo_tag_commit_kernel, dim3(num_systems), dim3(64), 0, s, tag0, sel, r_cn, r_fl, bulk_cn_min,
                       atomic_numbers, atom_offset, num_atoms, num_systems, cn_tol, tags, cn, flags, err.dev);
    ADF_HIP_CHECK(hipGetLastError());
    return err.finish(s, "tag_surface_atoms", VO_ERRORS);
}
