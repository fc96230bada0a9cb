// Gather and scatter over the active set of a relaxation (the list adf_lbfgs_active_build writes, csrc/lbfgs.hip): the
// systems whose update mask is set are copied into compact arrays for the model forward, and the compact forces and
// energies go back to the rows of those systems in the full arrays.
//
// A system's rows are contiguous in the full and in the compact array, so every copy is a contiguous range of dwords that
// the threads of a workgroup walk with stride 1 (coalesced).  Workgroup (k, y): the k-th active system, part y of
// gridDim.y of its rows.  The number of active systems is read from info[0] on the device; the grid is sized by the
// capacity (the system count of the full batch) and the workgroups past it exit.  No handle, no atomics, no host read.
#include "common.h"

#define ACT_THREADS 256
#define ACT_MAX_Y 64

struct act_table {
    adf_active_field f[ADF_ACTIVE_MAX_FIELDS];
    int n;
};

// The k-th active system, or false when this workgroup has nothing to do.
__device__ __forceinline__ bool act_system(const int32_t* __restrict__ atom_offset, const int32_t* __restrict__ act_sys,
                                           const int32_t* __restrict__ act_offset, const int32_t* __restrict__ info, int B,
                                           int& s, int64_t& a0, int64_t& c0, int64_t& n) {
    const int k = blockIdx.x;
    if (k >= info[0]) return false;
    s = act_sys[k];
    if (s < 0 || s >= B) return false;
    a0 = atom_offset[s];
    n = (int64_t)atom_offset[s + 1] - a0;
    c0 = act_offset[k];
    return true;
}

__global__ __launch_bounds__(ACT_THREADS) void act_gather_kernel(const int32_t* __restrict__ atom_offset,
                                                                 const int32_t* __restrict__ act_sys,
                                                                 const int32_t* __restrict__ act_offset,
                                                                 const int32_t* __restrict__ info, int B, act_table tab,
                                                                 int64_t* __restrict__ batch_out,
                                                                 int64_t* __restrict__ natoms_out) {
    int s;
    int64_t a0, c0, n;
    if (!act_system(atom_offset, act_sys, act_offset, info, B, s, a0, c0, n)) return;
    const int k = blockIdx.x;
    const int64_t first = (int64_t)blockIdx.y * ACT_THREADS + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.y * ACT_THREADS;
    for (int j = 0; j < tab.n; ++j) {
        const int64_t w = tab.f[j].row_bytes >> 2;   // dwords per row
        const uint32_t* __restrict__ src = (const uint32_t*)tab.f[j].src;
        uint32_t* __restrict__ dst = (uint32_t*)tab.f[j].dst;
        if (tab.f[j].per_system) {
            if (blockIdx.y == 0)
                for (int64_t i = threadIdx.x; i < w; i += ACT_THREADS) dst[(int64_t)k * w + i] = src[(int64_t)s * w + i];
        } else {
            src += a0 * w;
            dst += c0 * w;
            for (int64_t i = first; i < n * w; i += stride) dst[i] = src[i];
        }
    }
    if (batch_out)
        for (int64_t i = first; i < n; i += stride) batch_out[c0 + i] = k;
    if (natoms_out && blockIdx.y == 0 && threadIdx.x == 0) natoms_out[k] = n;
}

__global__ __launch_bounds__(ACT_THREADS) void act_scatter_kernel(const int32_t* __restrict__ atom_offset,
                                                                  const int32_t* __restrict__ act_sys,
                                                                  const int32_t* __restrict__ act_offset,
                                                                  const int32_t* __restrict__ info, int B,
                                                                  const float* __restrict__ forces_c,
                                                                  const uint32_t* __restrict__ energy_c, int energy_w,
                                                                  const int32_t* __restrict__ fixed,
                                                                  float* __restrict__ forces_raw,
                                                                  float* __restrict__ forces_con,
                                                                  uint32_t* __restrict__ energy) {
    int s;
    int64_t a0, c0, n;
    if (!act_system(atom_offset, act_sys, act_offset, info, B, s, a0, c0, n)) return;
    const int k = blockIdx.x;
    const int64_t first = (int64_t)blockIdx.y * ACT_THREADS + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.y * ACT_THREADS;
    for (int64_t i = first; i < 3 * n; i += stride) {
        const float v = forces_c[3 * c0 + i];
        forces_raw[3 * a0 + i] = v;
        forces_con[3 * a0 + i] = fixed[a0 + i / 3] != 0 ? 0.0f : v;
    }
    if (energy && blockIdx.y == 0)
        for (int i = threadIdx.x; i < energy_w; i += ACT_THREADS)
            energy[(int64_t)s * energy_w + i] = energy_c[(int64_t)k * energy_w + i];
}

// parts of a system's rows per workgroup row: about 1024 atoms each at the mean system size (known on the host: the
// capacities), so one large system does not leave its copy to a single workgroup
static int act_grid_y(int32_t num_systems, int64_t num_atoms) {
    const int64_t mean = num_atoms / num_systems;
    const int64_t y = (mean + 1023) / 1024;
    return (int)(y < 1 ? 1 : (y > ACT_MAX_Y ? ACT_MAX_Y : y));
}

static bool act_aligned(const void* p) { return ((uintptr_t)p & 3u) == 0; }

extern "C" int32_t adf_active_gather(const int32_t* atom_offset, const int32_t* act_sys, const int32_t* act_offset,
                                     const int32_t* info, int32_t num_systems, int64_t num_atoms,
                                     const adf_active_field* fields, int32_t num_fields, int64_t* batch_out,
                                     int64_t* natoms_out, void* stream) {
    if (!atom_offset || !act_sys || !act_offset || !info || (num_fields > 0 && !fields)) {
        adf_set_error("active_gather: null argument");
        return ADF_EINVAL;
    }
    if (num_systems <= 0 || num_atoms <= 0 || num_fields < 0 || num_fields > ADF_ACTIVE_MAX_FIELDS) {
        adf_set_error("active_gather: %d systems, %lld atoms, %d fields (at most %d fields, counts positive)", num_systems,
                      (long long)num_atoms, num_fields, ADF_ACTIVE_MAX_FIELDS);
        return ADF_EINVAL;
    }
    if (num_fields == 0 && !batch_out && !natoms_out) {
        adf_set_error("active_gather: nothing to write (no field, no batch, no natoms)");
        return ADF_EINVAL;
    }
    act_table tab;
    tab.n = num_fields;
    for (int j = 0; j < num_fields; ++j) {
        const adf_active_field& f = fields[j];
        if (!f.src || !f.dst) { adf_set_error("active_gather: field %d has a null pointer", j); return ADF_EINVAL; }
        if (f.row_bytes <= 0 || f.row_bytes % 4 != 0) {
            adf_set_error("active_gather: field %d has rows of %d bytes (a positive multiple of 4 is needed)", j, f.row_bytes);
            return ADF_EINVAL;
        }
        if (!act_aligned(f.src) || !act_aligned(f.dst)) {
            adf_set_error("active_gather: field %d is not 4-byte aligned", j);
            return ADF_EINVAL;
        }
        tab.f[j] = f;
    }
    hipLaunchKernelGGL(act_gather_kernel, dim3(num_systems, act_grid_y(num_systems, num_atoms)), dim3(ACT_THREADS), 0,
                       (hipStream_t)stream, atom_offset, act_sys, act_offset, info, num_systems, tab, batch_out, natoms_out);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}

extern "C" int32_t adf_active_scatter(const int32_t* atom_offset, const int32_t* act_sys, const int32_t* act_offset,
                                      const int32_t* info, int32_t num_systems, int64_t num_atoms, const float* forces_c,
                                      const void* energy_c, int32_t energy_row_bytes, const int32_t* fixed,
                                      float* forces_raw, float* forces_con, void* energy, void* stream) {
    if (!atom_offset || !act_sys || !act_offset || !info || !forces_c || !fixed || !forces_raw || !forces_con) {
        adf_set_error("active_scatter: null argument");
        return ADF_EINVAL;
    }
    if ((energy_c == nullptr) != (energy == nullptr)) {
        adf_set_error("active_scatter: energy_c and energy go together (both or neither)");
        return ADF_EINVAL;
    }
    if (num_systems <= 0 || num_atoms <= 0) {
        adf_set_error("active_scatter: %d systems, %lld atoms", num_systems, (long long)num_atoms);
        return ADF_EINVAL;
    }
    if (energy && (energy_row_bytes <= 0 || energy_row_bytes % 4 != 0 || !act_aligned(energy) || !act_aligned(energy_c))) {
        adf_set_error("active_scatter: energy rows of %d bytes (a positive multiple of 4, 4-byte aligned, is needed)",
                      energy_row_bytes);
        return ADF_EINVAL;
    }
    hipLaunchKernelGGL(act_scatter_kernel, dim3(num_systems, act_grid_y(num_systems, num_atoms)), dim3(ACT_THREADS), 0,
                       (hipStream_t)stream, atom_offset, act_sys, act_offset, info, num_systems, forces_c,
                       (const uint32_t*)energy_c, energy_row_bytes / 4, fixed, forces_raw, forces_con, (uint32_t*)energy);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}
