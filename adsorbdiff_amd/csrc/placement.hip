// Adsorbate placement on slabs: the reference's AdsorbateSlabConfig (adsorbdiff/placement/
// adsorbate_slab_config.py:99-439, 460-575 with adsorbate.py:122-169) for a whole batch of slabs, modes "random" and
// "random_site_heuristic_placement".  The contract of every entry is in include/adsorbdiff_hip.h.
//
// All arithmetic is float64 on float32 inputs (as noising.hip): the work is a few hundred pairs per placement, and this
// leaves the rounding of the float32 outputs as the only float32 effect.  Reductions are wave butterflies of max / min /
// integer sum, whose results do not depend on the order: every output is bit-reproducible.  No float atomics; the one
// integer atomic is the OR on the error word.
//
// Mapping.  pl_place_kernel / pl_gap_kernel: one wave per placement / system.  The lanes stride over the slab atoms (64
// per step); a lane wraps its slab atom once and loops over the adsorbate atoms, whose rotated positions are recomputed
// from the 3 x 3 rotation (nine multiply-adds, cheaper than staging them and no cap on the adsorbate's size).
// pl_candidates_kernel: one thread per candidate site.
#include <float.h>
#include <math.h>

#include "host_util.h"
#include "cell3.h"
#include "lanes.h"

enum { PL_ERR_Z = 1, PL_ERR_BINDING = 2, PL_ERR_RANGE = 4 };

struct pl_frame {
    double c[9];     // lattice, rows = vectors
    double inv[9];   // f_k = d . inv[:,k]
    double n[3];     // (a x b) / |a x b|, sign as it comes
    double cc[3];    // cell centre 0.5 (a + b + c)
};

__device__ __forceinline__ void pl_load_frame(const float* __restrict__ cell, pl_frame& F) {
#pragma unroll
    for (int k = 0; k < 9; ++k) F.c[k] = (double)cell[k];
    const double* c = F.c;
    adf_inv3(c, F.inv);
    // a x b (not cell3.h's adf_cross3: the call reorders the kernels' instructions)
    const double nx = c[1] * c[5] - c[2] * c[4], ny = c[2] * c[3] - c[0] * c[5], nz = c[0] * c[4] - c[1] * c[3];
    const double nn = sqrt(nx * nx + ny * ny + nz * nz);
    F.n[0] = nx / nn; F.n[1] = ny / nn; F.n[2] = nz / nn;
#pragma unroll
    for (int k = 0; k < 3; ++k) F.cc[k] = 0.5 * (c[k] + c[3 + k] + c[6 + k]);
}
// ase.geometry.wrap_positions about the cell centre: fractional coordinates, the periodic ones into [-eps, 1 - eps), back
__device__ __forceinline__ void pl_wrap(const pl_frame& F, const int32_t* __restrict__ pbc, double* p) {
    double f[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f[k] = p[0] * F.inv[k] + p[1] * F.inv[3 + k] + p[2] * F.inv[6 + k];
        if (pbc[k]) f[k] = adf_mod1_eps(f[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = f[0] * F.c[k] + f[1] * F.c[3 + k] + f[2] * F.c[6 + k];
}
// ------------------------------------------------------------------------------------------------ placements
struct pl_place_params {
    const float* slab_pos; const float* cell; const int32_t* slab_Z; const int32_t* slab_offset;
    int32_t B, N;
    const int32_t* slab_of; const float* site; const double* draws;
    const int32_t* ads_offset; const float* ads_pos; const int32_t* ads_Z;
    const float* radii; int32_t num_radii; const float* masses; int32_t num_masses;
    double gap; int32_t mode; const int32_t* binding_idx; const int32_t* pbc;
    int32_t P; const int32_t* out_row; int64_t out_rows;
    float* out_pos; double* scaled_normal; int32_t* n_combos; double* rot_meta; int32_t* err;
};

__global__ __launch_bounds__(64) void pl_place_kernel(pl_place_params q) {
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= q.P) return;
    const int b = q.slab_of[p];
    if (b < 0 || b >= q.B) { if (lane == 0) atomicOr(q.err, PL_ERR_RANGE); return; }
    int s0 = q.slab_offset[b], s1 = q.slab_offset[b + 1];
    const int a0 = q.ads_offset[b], na = q.ads_offset[b + 1] - a0;
    const long long o0 = q.out_row[p];
    if (s0 < 0 || s1 > q.N || s1 < s0 || na <= 0 || a0 < 0 || o0 < 0 || o0 + na > q.out_rows) {
        if (lane == 0) atomicOr(q.err, PL_ERR_RANGE);
        return;
    }
    pl_frame F;
    pl_load_frame(q.cell + 9 * (size_t)b, F);
    const int32_t* pbc = q.pbc + 3 * (size_t)b;
    const double site[3] = {(double)q.site[3 * (size_t)p], (double)q.site[3 * (size_t)p + 1], (double)q.site[3 * (size_t)p + 2]};

    // centre C of the rotations: every lane computes it alike (a short serial loop in a fixed order)
    double C[3] = {0.0, 0.0, 0.0};
    bool bad = false;
    if (q.mode == 0) {
        double m = 0.0;
        for (int a = 0; a < na; ++a) {
            const int z = q.ads_Z[a0 + a];
            const bool oob = z < 0 || z >= q.num_masses;
            bad = bad || oob;
            const double w = (double)q.masses[oob ? 0 : z];
            for (int k = 0; k < 3; ++k) C[k] += w * (double)q.ads_pos[3 * (size_t)(a0 + a) + k];
            m += w;
        }
        for (int k = 0; k < 3; ++k) C[k] /= m;
    } else {
        int bi = q.binding_idx[p];
        if (bi < 0 || bi >= na) { if (lane == 0) atomicOr(q.err, PL_ERR_BINDING); bi = 0; }
        for (int k = 0; k < 3; ++k) C[k] = (double)q.ads_pos[3 * (size_t)(a0 + bi) + k];
    }

    // R = Rodrigues(+z -> rotvec) . Rz(zrot); the identity for a one-atom adsorbate
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double meta[4] = {0.0, 0.0, 0.0, 0.0};
    if (na > 1) {
        const double* row = q.draws + 8 * (size_t)p;
        const double u0 = row[3], u1 = row[4], u2 = row[5];
        const double zrot = 360.0 * u0, phi = 2.0 * 3.141592653589793 * u2;
        const double cmin = 0.93969262078590838;   // cos(pi / 9)
        const double z = q.mode == 0 ? -1.0 + 2.0 * u1 : cmin + (1.0 - cmin) * u1;
        const double sxy = sqrt(fmax(0.0, 1.0 - z * z));
        const double rv[3] = {sxy * cos(phi), sxy * sin(phi), z};
        meta[0] = zrot; meta[1] = rv[0]; meta[2] = rv[1]; meta[3] = rv[2];
        const double ang = zrot * (3.141592653589793 / 180.0);
        const double cz = cos(ang), sz = sin(ang);
        // axis z_hat x rotvec = (-ry, rx, 0), of length s; below 1e-7: x_hat x rotvec = (0, -rz, ry), normalised
        double v[3] = {-rv[1], rv[0], 0.0};
        const double s = sqrt(v[0] * v[0] + v[1] * v[1]);
        if (s < 1e-7) {
            v[0] = 0.0; v[1] = -rv[2]; v[2] = rv[1];
            const double l = sqrt(v[1] * v[1] + v[2] * v[2]);
            v[1] /= l; v[2] /= l;
        } else {
            v[0] /= s; v[1] /= s;
        }
        const double c = z, t = 1.0 - c;
        // Rodrigues: c I + s [v]x + (1 - c) v v^T
        const double Q[9] = {c + t * v[0] * v[0],        t * v[0] * v[1] - s * v[2], t * v[0] * v[2] + s * v[1],
                             t * v[1] * v[0] + s * v[2], c + t * v[1] * v[1],        t * v[1] * v[2] - s * v[0],
                             t * v[2] * v[0] - s * v[1], t * v[2] * v[1] + s * v[0], c + t * v[2] * v[2]};
        const double Z[9] = {cz, -sz, 0.0, sz, cz, 0.0, 0.0, 0.0, 1.0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[3 * i + j] = Q[3 * i] * Z[j] + Q[3 * i + 1] * Z[3 + j] + Q[3 * i + 2] * Z[6 + j];
    }
    auto rotated = [&](int a, double* r) {   // R (p_a - C): the adsorbate atom relative to the site
        const float* pa = q.ads_pos + 3 * (size_t)(a0 + a);
        const double d[3] = {(double)pa[0] - C[0], (double)pa[1] - C[1], (double)pa[2] - C[2]};
        for (int i = 0; i < 3; ++i) r[i] = R[3 * i] * d[0] + R[3 * i + 1] * d[1] + R[3 * i + 2] * d[2];
    };

    // height: the wrapped image of every slab atom in the frame that puts the site on the cell centre
    double best = -DBL_MAX;
    int cnt = 0;
    for (int s = s0 + lane; s < s1; s += 64) {
        const int zs = q.slab_Z[s];
        const bool oob = zs < 0 || zs >= q.num_radii;
        bad = bad || oob;
        const double Rs = (double)q.radii[oob ? 0 : zs];
        double ps[3];
        for (int k = 0; k < 3; ++k) ps[k] = (double)q.slab_pos[3 * (size_t)s + k] + (F.cc[k] - site[k]);
        pl_wrap(F, pbc, ps);
        for (int a = 0; a < na; ++a) {
            const int za = q.ads_Z[a0 + a];
            const bool oa = za < 0 || za >= q.num_radii;
            bad = bad || oa;
            const double D = (double)q.radii[oa ? 0 : za] + Rs + q.gap;
            double r[3];
            rotated(a, r);
            const double w[3] = {ps[0] - (r[0] + F.cc[0]), ps[1] - (r[1] + F.cc[1]), ps[2] - (r[2] + F.cc[2])};
            const double h = w[0] * F.n[0] + w[1] * F.n[1] + w[2] * F.n[2];
            const double t[3] = {w[0] - h * F.n[0], w[1] - h * F.n[1], w[2] - h * F.n[2]};
            const double qd = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
            if (qd <= D) {
                ++cnt;
                best = fmax(best, h + sqrt(D * D - qd * qd));
            }
        }
    }
    if (s1 == s0)   // no slab atom: the adsorbate's radii are still checked
        for (int a = 0; a < na; ++a) { const int za = q.ads_Z[a0 + a]; bad = bad || za < 0 || za >= q.num_radii; }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(q.err, PL_ERR_Z);
    cnt = adf_wave_sum(cnt);
    best = adf_wave_max(best);
    const double sn = cnt > 0 ? best : 0.0;
    if (lane == 0) {
        q.scaled_normal[p] = sn;
        q.n_combos[p] = cnt;
        for (int k = 0; k < 4; ++k) q.rot_meta[4 * (size_t)p + k] = meta[k];
    }
    for (int a = lane; a < na; a += 64) {
        double r[3];
        rotated(a, r);
        for (int k = 0; k < 3; ++k) q.out_pos[3 * (size_t)(o0 + a) + k] = (float)(r[k] + site[k] + sn * F.n[k]);
    }
}

static int32_t pl_finish(adf_errword& err, hipStream_t s, const char* who, int32_t num_radii, int32_t num_masses) {
    const adf_errrow rows[] = {
        {PL_ERR_RANGE, ADF_EINVAL, "%s: an offset, slab index or output row out of range"},
        {PL_ERR_BINDING, ADF_EINVAL, "%s: binding_idx outside the adsorbate"},
        {PL_ERR_Z, ADF_EINVAL, "%s: atomic number outside [0, %d) (rows of the radius table) or [0, %d) (mass table)", num_radii,
         num_masses}};
    return err.finish(s, who, rows);
}

extern "C" int32_t adf_place_adsorbates(const adf_batch* slabs, const int32_t* slab_of, const float* site, const double* draws,
                                        const int32_t* ads_offset, const float* ads_pos, const int32_t* ads_Z,
                                        const float* radii, int32_t num_radii, const float* masses, int32_t num_masses,
                                        float interstitial_gap, int32_t mode, const int32_t* binding_idx, const int32_t* pbc,
                                        int32_t P, const int32_t* out_row, int64_t out_rows, float* out_pos,
                                        double* scaled_normal, int32_t* n_combos, double* rot_meta, void* stream) {
    if (!slabs || !slab_of || !site || !draws || !ads_offset || !ads_pos || !ads_Z || !radii || !masses || !pbc || !out_row ||
        !out_pos || !scaled_normal || !n_combos || !rot_meta) { adf_set_error("place_adsorbates: null argument"); return ADF_EINVAL; }
    if (!slabs->pos || !slabs->cell || !slabs->atomic_numbers || !slabs->atom_offset) { adf_set_error("place_adsorbates: null batch array"); return ADF_EINVAL; }
    if (slabs->num_systems <= 0 || slabs->num_atoms < 0 || P <= 0 || out_rows <= 0) { adf_set_error("place_adsorbates: empty input"); return ADF_EINVAL; }
    if (num_radii <= 0 || num_masses <= 0) { adf_set_error("place_adsorbates: empty radius or mass table"); return ADF_EINVAL; }
    if (mode != 0 && mode != 1) { adf_set_error("place_adsorbates: mode %d (0 random, 1 heuristic placement)", mode); return ADF_EINVAL; }
    if (mode == 1 && !binding_idx) { adf_set_error("place_adsorbates: heuristic placement needs binding_idx"); return ADF_EINVAL; }
    if (!(interstitial_gap >= 0.f && interstitial_gap < 5.f)) { adf_set_error("place_adsorbates: interstitial_gap %g outside [0, 5)", (double)interstitial_gap); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    adf_errword err;   // freed on every return (after the synchronisation in finish)
    ADF_TRY(err.create(s));
    pl_place_params q = {};
    q.slab_pos = slabs->pos; q.cell = slabs->cell; q.slab_Z = slabs->atomic_numbers; q.slab_offset = slabs->atom_offset;
    q.B = slabs->num_systems; q.N = slabs->num_atoms;
    q.slab_of = slab_of; q.site = site; q.draws = draws;
    q.ads_offset = ads_offset; q.ads_pos = ads_pos; q.ads_Z = ads_Z;
    q.radii = radii; q.num_radii = num_radii; q.masses = masses; q.num_masses = num_masses;
    q.gap = (double)interstitial_gap; q.mode = mode; q.binding_idx = binding_idx; q.pbc = pbc;
    q.P = P; q.out_row = out_row; q.out_rows = out_rows;
    q.out_pos = out_pos; q.scaled_normal = scaled_normal; q.n_combos = n_combos; q.rot_meta = rot_meta; q.err = err.dev;
    hipLaunchKernelGGL(pl_place_kernel, dim3(P), dim3(64), 0, s, q);
    ADF_HIP_CHECK(hipGetLastError());
    return pl_finish(err, s, "place_adsorbates", num_radii, num_masses);
}

// ------------------------------------------------------------------------------------------------ candidate sites
__global__ void pl_candidates_kernel(const float* __restrict__ tri, const int32_t* __restrict__ tri_offset,
                                     const int32_t* __restrict__ per_tri, const int32_t* __restrict__ cand_offset,
                                     const int32_t* __restrict__ cand_slab, const float* __restrict__ cell,
                                     const double* __restrict__ draws, int B, int n_cand, float* __restrict__ cand,
                                     int32_t* __restrict__ keep, int32_t* err) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cand) return;
    const int b = cand_slab[c];
    bool ok = b >= 0 && b < B;
    int t = 0;
    if (ok) {
        const int j = c - cand_offset[b], per = per_tri[b];
        ok = j >= 0 && per > 0;
        if (ok) {
            t = tri_offset[b] + j / per;
            ok = t >= tri_offset[b] && t < tri_offset[b + 1];
        }
    }
    if (!ok) {
        atomicOr(err, PL_ERR_RANGE);
        for (int k = 0; k < 3; ++k) cand[3 * (size_t)c + k] = 0.f;
        keep[c] = 0;
        return;
    }
    const double r1 = sqrt(draws[8 * (size_t)c]), r2 = draws[8 * (size_t)c + 1];
    const double w0 = 1.0 - r1, w1 = r1 * (1.0 - r2), w2 = r1 * r2;
    const float* v = tri + 9 * (size_t)t;
    double x[3];
    for (int k = 0; k < 3; ++k) x[k] = w0 * (double)v[k] + w1 * (double)v[3 + k] + w2 * (double)v[6 + k];
    pl_frame F;
    pl_load_frame(cell + 9 * (size_t)b, F);
    bool in = true;
    for (int k = 0; k < 2; ++k) {   // along a and b; c is not periodic for a site
        const double f = x[0] * F.inv[k] + x[1] * F.inv[3 + k] + x[2] * F.inv[6 + k];
        in = in && f >= -ADF_WRAP_EPS && f < 1.0 - ADF_WRAP_EPS;
    }
    for (int k = 0; k < 3; ++k) cand[3 * (size_t)c + k] = (float)x[k];
    keep[c] = in ? 1 : 0;
}

extern "C" int32_t adf_place_site_candidates(const float* tri, const int32_t* tri_offset, const int32_t* per_tri,
                                             const int32_t* cand_offset, const int32_t* cand_slab, const float* cell,
                                             const double* draws, int32_t B, int32_t num_candidates, float* cand,
                                             int32_t* keep, void* stream) {
    if (!tri || !tri_offset || !per_tri || !cand_offset || !cand_slab || !cell || !draws || !cand || !keep || B <= 0 ||
        num_candidates <= 0) { adf_set_error("place_site_candidates: bad argument"); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    adf_errword err;   // freed on every return (after the synchronisation in finish)
    ADF_TRY(err.create(s));
    hipLaunchKernelGGL(pl_candidates_kernel, dim3((num_candidates + 255) / 256), dim3(256), 0, s, tri, tri_offset, per_tri,
                       cand_offset, cand_slab, cell, draws, B, num_candidates, cand, keep, err.dev);
    ADF_HIP_CHECK(hipGetLastError());
    return pl_finish(err, s, "place_site_candidates", 0, 0);
}

// ------------------------------------------------------------------------------------------------ interstitial distances
__global__ __launch_bounds__(64) void pl_gap_kernel(const float* __restrict__ pos, const float* __restrict__ cell,
                                                    const int32_t* __restrict__ Z, const int32_t* __restrict__ tags,
                                                    const int32_t* __restrict__ atom_offset, int B, int N,
                                                    const float* __restrict__ radii, int num_radii,
                                                    const float* __restrict__ masses, int num_masses,
                                                    const int32_t* __restrict__ pbc_all, float* __restrict__ out, int32_t* err) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    int a0 = atom_offset[b], a1 = atom_offset[b + 1];
    if (a0 < 0 || a1 > N || a1 < a0) { if (lane == 0) { atomicOr(err, PL_ERR_RANGE); out[b] = INFINITY; } return; }
    pl_frame F;
    pl_load_frame(cell + 9 * (size_t)b, F);
    const int32_t* pbc = pbc_all + 3 * (size_t)b;
    // mass centre of the adsorbate: a serial loop in atom order, alike in every lane
    double com[3] = {0.0, 0.0, 0.0}, m = 0.0;
    bool bad = false;
    int n_ads = 0;
    for (int a = a0; a < a1; ++a)
        if (tags[a] == 2) {
            const int z = Z[a];
            const bool oob = z < 0 || z >= num_masses;
            bad = bad || oob;
            const double w = (double)masses[oob ? 0 : z];
            for (int k = 0; k < 3; ++k) com[k] += w * (double)pos[3 * (size_t)a + k];
            m += w;
            ++n_ads;
        }
    double best = INFINITY;
    if (n_ads > 0) {
        double sh[3];
        for (int k = 0; k < 3; ++k) sh[k] = F.cc[k] - com[k] / m;
        for (int s = a0 + lane; s < a1; s += 64) {
            if (tags[s] != 1) continue;
            const int zs = Z[s];
            const bool os = zs < 0 || zs >= num_radii;
            bad = bad || os;
            const double Rs = (double)radii[os ? 0 : zs];
            double ps[3];
            for (int k = 0; k < 3; ++k) ps[k] = (double)pos[3 * (size_t)s + k] + sh[k];
            pl_wrap(F, pbc, ps);
            for (int a = a0; a < a1; ++a) {
                if (tags[a] != 2) continue;
                const int za = Z[a];
                const bool oa = za < 0 || za >= num_radii;
                bad = bad || oa;
                double pa[3];
                for (int k = 0; k < 3; ++k) pa[k] = (double)pos[3 * (size_t)a + k] + sh[k];
                pl_wrap(F, pbc, pa);
                const double d[3] = {pa[0] - ps[0], pa[1] - ps[1], pa[2] - ps[2]};
                best = fmin(best, sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) - (double)radii[oa ? 0 : za] - Rs);
            }
        }
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(err, PL_ERR_Z);
    best = adf_wave_min(best);
    if (lane == 0) out[b] = (float)best;
}

extern "C" int32_t adf_interstitial_distances(const adf_batch* b, const int32_t* tags, const float* radii, int32_t num_radii,
                                              const float* masses, int32_t num_masses, const int32_t* pbc, float* out,
                                              void* stream) {
    if (!b || !tags || !radii || !masses || !pbc || !out) { adf_set_error("interstitial_distances: null argument"); return ADF_EINVAL; }
    if (b->num_atoms <= 0 || b->num_systems <= 0) { adf_set_error("interstitial_distances: empty batch"); return ADF_EINVAL; }
    if (!b->pos || !b->cell || !b->atomic_numbers || !b->atom_offset) { adf_set_error("interstitial_distances: null batch array"); return ADF_EINVAL; }
    if (num_radii <= 0 || num_masses <= 0) { adf_set_error("interstitial_distances: empty radius or mass table"); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    adf_errword err;   // freed on every return (after the synchronisation in finish)
    ADF_TRY(err.create(s));
    hipLaunchKernelGGL(pl_gap_kernel, dim3(b->num_systems), dim3(64), 0, s, b->pos, b->cell, b->atomic_numbers, tags,
                       b->atom_offset, b->num_systems, b->num_atoms, radii, num_radii, masses, num_masses, pbc, out, err.dev);
    ADF_HIP_CHECK(hipGetLastError());
    return pl_finish(err, s, "interstitial_distances", num_radii, num_masses);
}
