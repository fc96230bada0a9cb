// Relaxation anomaly flags and site ranking: the four first-frame / last-frame tests of the reference's
// DetectTrajAnomaly (adsorbdiff/placement/flag_anomaly.py:6-154) on a whole batch, and the per-system minimum of the
// relaxed energy over the sites that pass (scripts/eval.py:566-579).  The contract is in include/adsorbdiff_hip.h.
//
// Every test is an OR over atom pairs of one system, so the kernel evaluates each unordered pair (i <= j, the diagonal
// included: an atom can bind its own image) once, in two position sets:
//   F  the final positions, and
//   O  "the other frame" of the atom's own class: the initial position of an adsorbate atom (tag 2), the slab
//      reference position of a slab atom.
// A pair of two adsorbate atoms compares conn_1 in O and F (dissociation), a pair of two slab atoms compares the
// bonded / cushioned connectivities of O and F (surface change), a mixed pair looks at F alone (bonded within the
// desorption cutoff; bonded to a frozen atom).  dmin is the minimum over lattice images of the displacement.
//
// Image bound.  The displacement is first reduced to fractional coordinates in [-1/2, 1/2] along every periodic
// direction (reps[k] > 0); the images n_k in [-reps[k], reps[k]] are then tried.  With h_k the spacing of the lattice
// planes of direction k, an image has length >= (|n_k| - 1/2) h_k, so images within a threshold t have
// |n_k| < t / h_k + 1/2, that is |n_k| <= ceil(t / h_k): what engine.cell_repeats returns for radius t.  The caller
// sizes reps for the largest threshold of the batch (plus a margin for float32 rounding of the reduction).  More images
// than needed never change a minimum.
//
// Mapping.  One workgroup of 256 threads per (system, row tile); blockIdx.y strides over the row tiles so that no
// system size is capped and the host needs no per-system count.  The i side (a row) lives in registers, the j side is
// staged through LDS in tiles of 256 atoms (position, radius, tag of both position sets: 8 KiB).  The height of a row
// tile adapts to the system: 2^LR rows with 2^LR >= min(n, 64), and the 256 threads form 2^LR rows x 256 / 2^LR column
// phases, so a 10-atom system occupies 16 x 16 threads with pairs instead of 10 of 64 rows.  Lanes of one column phase
// read the same LDS address (broadcast).  Evidence bits are OR-ed per wave (ballot) and leave with integer atomicOr on the
// zeroed output words; OR is order-independent, so the flags are bit-reproducible.  A last kernel turns "bonded" into
// "desorbed".  No float atomics, no scratch but one error word.
#include <float.h>
#include <limits.h>

#include "host_util.h"
#include "cell3.h"
#include "lanes.h"

#define AN_THREADS 256
#define AN_TJ 256   // atoms per staged j tile

enum { AN_ERR_Z = 1 };   // the one bit of the error word

struct an_params {
    const float* pos_init;
    const float* pos_final;
    const float* pos_ref;      // slab reference, aligned with the batch (the initial positions when none is given)
    const float* cell;
    const int32_t* Z;
    const int32_t* tags;
    const int32_t* atom_offset;
    const float* radii;
    int32_t num_radii;
    int32_t reps[3];
    float skin2, surface_mult, desorption_mult;
    int32_t* flags;            // [B,4], zeroed; word 1 collects "bonded" until an_finish_kernel
    int32_t* err;              // device word: an atomic number outside the table
};

// min over the lattice images of |d + T|^2 for the reduced displacement d; the zero image is left out for i == j
__device__ __forceinline__ float an_min_image(float dx, float dy, float dz, const float (&c)[9], int r0, int r1, int r2,
                                              bool self) {
    float best = FLT_MAX;
    for (int n0 = -r0; n0 <= r0; ++n0) {
        const float ax = fmaf((float)n0, c[0], dx), ay = fmaf((float)n0, c[1], dy), az = fmaf((float)n0, c[2], dz);
        for (int n1 = -r1; n1 <= r1; ++n1) {
            const float bx = fmaf((float)n1, c[3], ax), by = fmaf((float)n1, c[4], ay), bz = fmaf((float)n1, c[5], az);
            for (int n2 = -r2; n2 <= r2; ++n2) {
                const float x = fmaf((float)n2, c[6], bx), y = fmaf((float)n2, c[7], by), z = fmaf((float)n2, c[8], bz);
                float d2 = fmaf(x, x, fmaf(y, y, z * z));
                if ((n0 | n1 | n2) == 0) d2 = self ? FLT_MAX : d2;   // uniform condition, per-lane select
                best = fminf(best, d2);
            }
        }
    }
    return best;
}

__global__ __launch_bounds__(AN_THREADS) void an_pairs_kernel(an_params p) {
    __shared__ float4 sF[AN_TJ];   // final x, y, z, radius
    __shared__ float4 sO[AN_TJ];   // other-frame x, y, z, tag (integer bits)
    const int b = blockIdx.x, tid = threadIdx.x;
    const int a0 = p.atom_offset[b];
    const int n = p.atom_offset[b + 1] - a0;
    if (n <= 0) return;
    int LR = 2;
    while (LR < 6 && (1 << LR) < n) ++LR;
    const int rows = 1 << LR, phases = AN_THREADS >> LR;
    const int ntiles = (n + rows - 1) >> LR;
    if ((int)blockIdx.y >= ntiles) return;

    // lattice (rows = vectors), its inverse for the fractional reduction; a direction with reps 0 is not periodic
    float c[9], inv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) c[k] = p.cell[9 * (size_t)b + k];
    adf_inv3(c, inv);
    const int r0 = p.reps[0], r1 = p.reps[1], r2 = p.reps[2];
    const float w0 = r0 > 0 ? 1.f : 0.f, w1 = r1 > 0 ? 1.f : 0.f, w2 = r2 > 0 ? 1.f : 0.f;

    auto load_atom = [&](int local, float4& f, float4& o) {
        const int a = a0 + min(local, n - 1);            // clamped: no branch around the loads
        const int tag = p.tags[a];
        const int z = p.Z[a];
        const bool bad = z < 0 || z >= p.num_radii;
        if (bad && local < n) atomicOr(p.err, AN_ERR_Z);
        const float rad = p.radii[bad ? 0 : z];
        const float* src = tag == 2 ? p.pos_init : p.pos_ref;
        f = make_float4(p.pos_final[3 * (size_t)a], p.pos_final[3 * (size_t)a + 1], p.pos_final[3 * (size_t)a + 2], rad);
        o = make_float4(src[3 * (size_t)a], src[3 * (size_t)a + 1], src[3 * (size_t)a + 2], __int_as_float(tag));
    };
    auto reduced = [&](float& dx, float& dy, float& dz) {
        const float f0 = rintf(dx * inv[0] + dy * inv[3] + dz * inv[6]) * w0;
        const float f1 = rintf(dx * inv[1] + dy * inv[4] + dz * inv[7]) * w1;
        const float f2 = rintf(dx * inv[2] + dy * inv[5] + dz * inv[8]) * w2;
        dx -= f0 * c[0] + f1 * c[3] + f2 * c[6];
        dy -= f0 * c[1] + f1 * c[4] + f2 * c[7];
        dz -= f0 * c[2] + f1 * c[5] + f2 * c[8];
    };

    const int row = tid & (rows - 1), phase = tid >> LR;
    for (int tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
        const int i0 = tile << LR, i = i0 + row;
        const bool row_ok = i < n;
        float4 iF, iO;
        load_atom(i, iF, iO);
        const int ti = __float_as_int(iO.w);
        int ev = 0;
        for (int j0 = i0; j0 < n; j0 += AN_TJ) {          // pairs i <= j only: tiles before the row tile are skipped
            __syncthreads();
            load_atom(j0 + tid, sF[tid], sO[tid]);
            __syncthreads();
            const int jn = min(AN_TJ, n - j0);
            for (int jj = phase; jj < jn; jj += phases) {
                const int j = j0 + jj;
                const float4 jF = sF[jj], jO = sO[jj];
                const int tj = __float_as_int(jO.w);
                if (!row_ok || j < i) continue;
                float fx = jF.x - iF.x, fy = jF.y - iF.y, fz = jF.z - iF.z;
                float ox = jO.x - iO.x, oy = jO.y - iO.y, oz = jO.z - iO.z;
                reduced(fx, fy, fz);
                reduced(ox, oy, oz);
                const bool self = i == j;
                const float dF = sqrtf(an_min_image(fx, fy, fz, c, r0, r1, r2, self));
                const float dO = sqrtf(an_min_image(ox, oy, oz, c, r0, r1, r2, self));
                const float sumR = iF.w + jF.w;
                const float t1 = sumR + p.skin2;
                const float ts = p.surface_mult * sumR + p.skin2;
                const float td = p.desorption_mult * sumR + p.skin2;
                const bool ai = ti == 2, aj = tj == 2;
                if (ai && aj) {
                    if ((dF < t1) != (dO < t1)) ev |= 1;
                } else if (ai != aj) {
                    if (dF < td) ev |= 2;
                    if ((ai ? tj : ti) == 0 && dF < t1) ev |= 8;
                } else {
                    if (((dF < t1) && !(dO < ts)) || ((dO < t1) && !(dF < ts))) ev |= 4;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned long long any = __ballot((ev >> k) & 1);
            if (any != 0ull && (tid & 63) == 0) atomicOr(&p.flags[4 * (size_t)b + k], 1);
        }
    }
}

__global__ void an_finish_kernel(int32_t* flags, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) flags[4 * (size_t)b + 1] = flags[4 * (size_t)b + 1] ? 0 : 1;   // desorbed = no bonded (adsorbate, slab) pair
}

extern "C" int32_t adf_flag_anomalies(const adf_batch* b, const float* pos_final, const float* pos_slab_ref,
                                      const int32_t* tags, const float* radii, int32_t num_radii, float skin,
                                      float surface_mult, float desorption_mult, int32_t* flags, void* stream) {
    if (!b || !pos_final || !tags || !radii || !flags) { adf_set_error("flag_anomalies: null argument"); return ADF_EINVAL; }
    if (b->num_atoms <= 0 || b->num_systems <= 0) { adf_set_error("flag_anomalies: empty batch"); return ADF_EINVAL; }
    if (!b->pos || !b->cell || !b->atomic_numbers || !b->atom_offset) { adf_set_error("flag_anomalies: null batch array"); return ADF_EINVAL; }
    if (num_radii <= 0) { adf_set_error("flag_anomalies: empty radius table"); return ADF_EINVAL; }
    for (int k = 0; k < 3; ++k)
        if (b->reps[k] < 0 || b->reps[k] > 16) { adf_set_error("flag_anomalies: reps[%d]=%d out of range", k, b->reps[k]); return ADF_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    adf_errword err;   // freed on every return (after the synchronisation in finish)
    ADF_TRY(err.create(s));
    const int B = b->num_systems;
    ADF_HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(int32_t) * 4 * (size_t)B, s));
    an_params p = {};
    p.pos_init = b->pos; p.pos_final = pos_final; p.pos_ref = pos_slab_ref ? pos_slab_ref : b->pos;
    p.cell = b->cell; p.Z = b->atomic_numbers; p.tags = tags; p.atom_offset = b->atom_offset;
    p.radii = radii; p.num_radii = num_radii;
    for (int k = 0; k < 3; ++k) p.reps[k] = b->reps[k];
    p.skin2 = 2.0f * skin; p.surface_mult = surface_mult; p.desorption_mult = desorption_mult;
    p.flags = flags; p.err = err.dev;
    // row-tile slots per system: twice the average system's 64-row tiles, so that the common system has a workgroup
    // per tile; a system with more tiles strides over them, one with fewer leaves its spare workgroups at once
    const long long avg_tiles = ((long long)b->num_atoms / B + 63) / 64;
    // (at least one: a batch with empty systems can average below one atom)
    const int slots = (int)(avg_tiles * 2 > 64 ? 64 : avg_tiles * 2 < 1 ? 1 : avg_tiles * 2);
    hipLaunchKernelGGL(an_pairs_kernel, dim3(B, slots), dim3(AN_THREADS), 0, s, p);
    ADF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(an_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, s, flags, B);
    ADF_HIP_CHECK(hipGetLastError());
    // this message has never named its entry: `who` is empty, and the format's leading %s prints nothing
    const adf_errrow rows[] = {{AN_ERR_Z, ADF_EINVAL, "%satomic number outside [0, %d) (rows of the radius table)", num_radii}};
    return err.finish(s, "", rows);
}

// ---- site ranking: one wave per group, lanes stride over the group's sites in index order, then a butterfly whose
// comparison (energy, then index) is a total order: the result does not depend on the reduction's shape.
__global__ __launch_bounds__(256) void an_best_sites_kernel(const float* energy, const int32_t* flags,
                                                             const int32_t* group_offset, int num_groups, int32_t* best,
                                                             float* best_energy, int32_t* n_valid) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= num_groups) return;
    const int s0 = group_offset[g], s1 = group_offset[g + 1];
    float be = INFINITY;
    int bi = INT_MAX, cnt = 0;
    for (int i = s0 + lane; i < s1; i += 64) {
        const float e = energy[i];
        bool ok = !(e != e);
        if (flags) ok = ok && (flags[4 * (size_t)i] | flags[4 * (size_t)i + 1] | flags[4 * (size_t)i + 2] | flags[4 * (size_t)i + 3]) == 0;
        if (ok) {
            ++cnt;
            if (e < be || (e == be && i < bi)) { be = e; bi = i; }
        }
    }
    // kept inline: as a call to lanes.h this butterfly reorders the kernel's instructions (tools/device_asm_diff.py)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float oe = __shfl_xor(be, o);
        const int oi = __shfl_xor(bi, o);
        cnt += __shfl_xor(cnt, o);
        if (oe < be || (oe == be && oi < bi)) { be = oe; bi = oi; }
    }
    if (lane == 0) {
        best[g] = bi == INT_MAX ? -1 : bi;
        if (best_energy) best_energy[g] = bi == INT_MAX ? INFINITY : be;
        if (n_valid) n_valid[g] = cnt;
    }
}

extern "C" int32_t adf_select_best_sites(const float* energy, const int32_t* flags, const int32_t* group_offset,
                                         int32_t num_groups, int32_t* best, float* best_energy, int32_t* n_valid,
                                         void* stream) {
    if (!energy || !group_offset || !best || num_groups <= 0) { adf_set_error("select_best_sites: bad argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(an_best_sites_kernel, dim3((num_groups + 3) / 4), dim3(256), 0, (hipStream_t)stream, energy, flags,
                       group_offset, num_groups, best, best_energy, n_valid);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}
