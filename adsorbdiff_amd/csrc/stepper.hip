// Reverse-SDE/ODE stepper of the adsorbate placement, device resident.
//
// Reference: adsorbdiff/relaxation/diffusers/denoising_torch.py
//   :215-232  initial placement   com_xy <- cell . noise, z kept, rigid translation
//   :263-310  per step: per-system mean of the two heads over tag==2 atoms (f2 zeroed on fixed
//             atoms first, :498), ODE/SDE increment, z of the translation zeroed, wrap of the
//             COM into the cell via solve / mod / cell.f   (COLUMNS of `cell` act as lattice
//             vectors here, unlike the graph code — kept as is)
//   :312-320  cumulative early stop over *all* systems (allclose(dcom, 0, 1e-3, 1e-3))
//   :322-353  rigid rotation about the COM (axis-angle -> quaternion -> matrix,
//             utils/rot_utils.py:18-98) + translation of each adsorbate
// The reference does this with a Python loop over systems and a device->host sync per step; here
// it is two tiny kernels (one wave per system) and no host round trip.
#include <stdlib.h>

#include "common.h"

struct StepParams {
    const float* cell;
    const int32_t* atom_offset;
    const int32_t* tags;
    const int32_t* fixed;
    float* pos;
    const float* f1;
    const float* f2;
    const float* z_tr;
    const float* z_rot;
    float* sys;  // [B][16]: com(3) dcom(3) drot(3) cnt conv
    int32_t* state;
    float* dcom_out;
    float* drot_out;
    int B;
    adf_step_coef c;
    const adf_step_coef* coefs_dev;  // optional schedule table on the device, indexed by state[4]
    int num_steps;
    int early_stop_count;
};

__device__ __forceinline__ float pymod1(float x) {
    // torch.remainder(x, 1): result has the sign of the divisor
    float r = fmodf(x, 1.0f);
    if (r < 0.f) r += 1.0f;
    return r;
}

// Solve A f = v, 3x3, partial pivoting (what LAPACK sgesv / torch.linalg.solve does).
__device__ void solve3(const float* A, const float* v, float* f) {
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

__global__ __launch_bounds__(64) void adf_init_placement_kernel(const float* cell, const int32_t* atom_offset,
                                                                 const int32_t* tags, float* pos, const float* noise,
                                                                 int B) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int a0 = atom_offset[b], a1 = atom_offset[b + 1];
    float sx = 0.f, sy = 0.f, sz = 0.f, cnt = 0.f;
    for (int a = a0 + lane; a < a1; a += 64)
        if (tags[a] == 2) { sx += pos[3 * a]; sy += pos[3 * a + 1]; sz += pos[3 * a + 2]; cnt += 1.f; }
    sx = adf_wave_sum(sx); sy = adf_wave_sum(sy); sz = adf_wave_sum(sz); cnt = adf_wave_sum(cnt);
    const float inv = 1.0f / fmaxf(cnt, 1.0f);
    const float cx = sx * inv, cy = sy * inv, cz = sz * inv;
    const float* cl = cell + 9 * b;
    const float* nz = noise + 3 * b;
    // einsum("bi,bij->bj", noise, cell^T): out_j = sum_i noise_i * cell[j][i]
    const float nx = cl[0] * nz[0] + cl[1] * nz[1] + cl[2] * nz[2];
    const float ny = cl[3] * nz[0] + cl[4] * nz[1] + cl[5] * nz[2];
    (void)cz;
    for (int a = a0 + lane; a < a1; a += 64)
        if (tags[a] == 2) {
            pos[3 * a] = (pos[3 * a] - cx) + nx;
            pos[3 * a + 1] = (pos[3 * a + 1] - cy) + ny;
            // z: (z - com_z) + com_z, as the reference evaluates it
            pos[3 * a + 2] = (pos[3 * a + 2] - cz) + cz;
        }
}

// ---- the per-system arithmetic of one step, shared by the coupled kernels (reduce / apply) and the per-system kernel:
// the two paths must give the same bits, so there is one text of it.
// sums over the tag-2 atoms of [a0, a1): pos(3) f1(3) f2*keep(3) count; every lane returns the same totals
__device__ __forceinline__ void step_sums(const StepParams& p, int a0, int a1, int lane, float* s) {
#pragma unroll
    for (int i = 0; i < 10; ++i) s[i] = 0.f;
    for (int a = a0 + lane; a < a1; a += 64)
        if (p.tags[a] == 2) {
            const float keep = (p.fixed && p.fixed[a] == 1) ? 0.f : 1.f;
            s[0] += p.pos[3 * a]; s[1] += p.pos[3 * a + 1]; s[2] += p.pos[3 * a + 2];
            s[3] += p.f1[3 * a]; s[4] += p.f1[3 * a + 1]; s[5] += p.f1[3 * a + 2];
            s[6] += p.f2[3 * a] * keep; s[7] += p.f2[3 * a + 1] * keep; s[8] += p.f2[3 * a + 2] * keep;
            s[9] += 1.f;
        }
#pragma unroll
    for (int i = 0; i < 10; ++i) s[i] = adf_wave_sum(s[i]);
}

// the wrap of the COM into the cell: com + dcom -> solve / mod / cell.f; dcom becomes the wrapped increment.
// Returns the convergence predicate allclose(dcom, 0, 1e-3, 1e-3) of this system.
__device__ __forceinline__ bool step_wrap(const float* cl, const float* tgt, const float* com, float* dcom) {
    float fr[3];
    solve3(cl, tgt, fr);
    for (int k = 0; k < 3; ++k) fr[k] = pymod1(pymod1(fr[k]));
    bool conv = true;
    for (int j = 0; j < 3; ++j) {
        const float w = cl[3 * j] * fr[0] + cl[3 * j + 1] * fr[1] + cl[3 * j + 2] * fr[2];
        dcom[j] = w - com[j];
        conv = conv && (fabsf(dcom[j]) <= 1.0e-3f);
    }
    return conv;
}

// sums -> com, wrapped dcom, drot of system b; returns its convergence predicate
__device__ __forceinline__ bool step_increment(const StepParams& p, int b, const float* s, float* com, float* dcom,
                                               float* drot) {
    const float cnt = fmaxf(s[9], 1.0f);
    // schedule scalars: by value, or (graph replay: identical launch every step) from the device table
    adf_step_coef c = p.c;
    if (p.coefs_dev) c = p.coefs_dev[min(p.state[4], p.num_steps - 1)];
    for (int k = 0; k < 3; ++k) {
        com[k] = s[k] / cnt;
        const float str = s[3 + k] / cnt;
        const float srot = s[6 + k] / cnt;
        float d = __fmul_rn(c.coef_tr, str);
        float r = __fmul_rn(__fmul_rn(__fmul_rn(c.rot_pre, srot), c.rot_dt), c.rot_g2);
        if (p.z_tr) d = __fadd_rn(d, __fmul_rn(c.noise_tr, p.z_tr[3 * b + k]));
        if (p.z_rot) r = __fadd_rn(r, __fmul_rn(c.noise_rot, p.z_rot[3 * b + k]));
        dcom[k] = d;
        drot[k] = r;
    }
    dcom[2] = 0.f;
    const float tgt[3] = {com[0] + dcom[0], com[1] + dcom[1], com[2] + dcom[2]};
    return step_wrap(p.cell + 9 * b, tgt, com, dcom);
}

// rigid update of the adsorbate of [a0, a1): rotation by the axis-angle (ax, ay, az) about (cx, cy, cz), then translation
__device__ __forceinline__ void step_rigid_update(float* pos, const int32_t* tags, int a0, int a1, int lane, float cx,
                                                  float cy, float cz, float tx, float ty, float tz, float ax, float ay,
                                                  float az) {
    // axis-angle -> quaternion (rot_utils.py:50-81)
    const float ang = sqrtf(ax * ax + ay * ay + az * az);
    const float half = 0.5f * ang;
    float k;
    if (fabsf(ang) < 1e-6f) k = 0.5f - (ang * ang) / 48.0f;
    else k = sinf(half) / ang;
    const float qr = cosf(half), qi = ax * k, qj = ay * k, qk = az * k;
    // quaternion -> matrix (rot_utils.py:18-47)
    const float two_s = 2.0f / (qr * qr + qi * qi + qj * qj + qk * qk);
    const float R00 = 1 - two_s * (qj * qj + qk * qk), R01 = two_s * (qi * qj - qk * qr), R02 = two_s * (qi * qk + qj * qr);
    const float R10 = two_s * (qi * qj + qk * qr), R11 = 1 - two_s * (qi * qi + qk * qk), R12 = two_s * (qj * qk - qi * qr);
    const float R20 = two_s * (qi * qk - qj * qr), R21 = two_s * (qj * qk + qi * qr), R22 = 1 - two_s * (qi * qi + qj * qj);
    for (int a = a0 + lane; a < a1; a += 64)
        if (tags[a] == 2) {
            const float rx = pos[3 * a] - cx, ry = pos[3 * a + 1] - cy, rz = pos[3 * a + 2] - cz;
            // (rel @ R^T) + dcom + com   (denoising_torch.py:331-336)
            pos[3 * a] = ((rx * R00 + ry * R01 + rz * R02) + tx) + cx;
            pos[3 * a + 1] = ((rx * R10 + ry * R11 + rz * R12) + ty) + cy;
            pos[3 * a + 2] = ((rx * R20 + ry * R21 + rz * R22) + tz) + cz;
        }
}

// phase 1: per-system scores -> (dcom, drot), wrapped; per-system convergence AND-ed into state[2]
__global__ __launch_bounds__(64) void adf_step_reduce_kernel(StepParams p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int a0 = p.atom_offset[b], a1 = p.atom_offset[b + 1];
    float s[10];
    step_sums(p, a0, a1, lane, s);
    if (lane != 0) return;
    float com[3], dcom[3], drot[3];
    const bool conv = step_increment(p, b, s, com, dcom, drot);
    float* o = p.sys + 16 * b;
    for (int k = 0; k < 3; ++k) { o[k] = com[k]; o[3 + k] = dcom[k]; o[6 + k] = drot[k]; }
    if (!conv) atomicAnd(&p.state[2], 0);
    if (p.dcom_out) for (int k = 0; k < 3; ++k) p.dcom_out[3 * b + k] = dcom[k];
    if (p.drot_out) for (int k = 0; k < 3; ++k) p.drot_out[3 * b + k] = drot[k];
}

// phase 2: early-stop bookkeeping (block 0 decides, every block re-derives the same decision from
// state[] written by the *previous* launch's decision kernel) + rigid update of each adsorbate
__global__ void adf_step_decide_kernel(int32_t* state, int early_stop_count) {
    // state: [0]=cumulative converged count, [1]=frozen, [2]=all-converged flag of this step, [3]=steps applied,
    //        [4]=steps issued (index into the device schedule table)
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (!state[1]) {
            if (state[2]) {
                state[0] += 1;
                if (early_stop_count > 0 && state[0] == early_stop_count) state[1] = 1;
            }
            if (!state[1]) state[3] += 1;
        }
        state[2] = 1;  // re-arm for the next step
        state[4] += 1;
    }
}

// a split run (sample_loop_split) keeps every step's all-converged flag of each view: the whole batch's count of converged
// steps is formed from the two histories at the join.  Runs between the reduce and the decide launch of its step.
__global__ void adf_step_keep_flag_kernel(const int32_t* state, int32_t* hist_t) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *hist_t = state[2];
}

__global__ __launch_bounds__(64) void adf_step_apply_kernel(StepParams p) {
    if (p.state[1]) return;  // the reference's `break`: this and all later steps leave pos untouched
    const int b = blockIdx.x, lane = threadIdx.x;
    const int a0 = p.atom_offset[b], a1 = p.atom_offset[b + 1];
    const float* o = p.sys + 16 * b;
    step_rigid_update(p.pos, p.tags, a0, a1, lane, o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8]);
}

// ---- per-system early stop (adf_*_set_per_system_stop): the decision is local to a system, so scores, wrap, decision and
// the rigid update are ONE kernel, one wave per system.  sys_state[b] = {cvg_count, frozen, steps_applied, stop_step}.
// The rule is the reference's loop (:312-320) for that system alone: a frozen system is not read and not written; a system
// whose cumulative count reaches early_stop_count at step t freezes BEFORE this step's update (the `break`).
// Global state: [0] frozen systems (atomicAdd), [3] max steps applied (atomicMax), [4] steps issued - read here by every
// workgroup as the schedule index and as t, so it is the finish kernel after this one that bumps it and sets [1].
// Returns true when this step's update is to be applied; lane 0 has then done all of the system's bookkeeping.
__device__ __forceinline__ bool system_decide(int32_t* st, int32_t* state, int cvg, bool conv, int early_stop_count,
                                              int lane) {
    bool freeze = false;
    if (conv) {
        cvg += 1;
        freeze = early_stop_count > 0 && cvg == early_stop_count;
    }
    if (lane == 0) {
        st[0] = cvg;
        if (freeze) {
            st[1] = 1;
            st[3] = state[4];
            atomicAdd(&state[0], 1);
        } else {
            const int applied = st[2] + 1;
            st[2] = applied;
            atomicMax(&state[3], applied);
        }
    }
    return !freeze;
}

__global__ __launch_bounds__(64) void adf_step_system_kernel(StepParams p, int32_t* sys_state) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int32_t* st = sys_state + 4 * b;
    const int cvg = st[0], frozen = st[1];
    if (frozen) {
        if (lane < 3) {
            if (p.dcom_out) p.dcom_out[3 * b + lane] = 0.f;
            if (p.drot_out) p.drot_out[3 * b + lane] = 0.f;
        }
        return;
    }
    const int a0 = p.atom_offset[b], a1 = p.atom_offset[b + 1];
    float s[10];
    step_sums(p, a0, a1, lane, s);
    float com[3], dcom[3], drot[3];   // every lane alike: the totals are in all of them
    const bool conv = step_increment(p, b, s, com, dcom, drot);
    if (lane < 3) {
        if (p.dcom_out) p.dcom_out[3 * b + lane] = dcom[lane];
        if (p.drot_out) p.drot_out[3 * b + lane] = drot[lane];
    }
    if (system_decide(st, p.state, cvg, conv, p.early_stop_count, lane))
        step_rigid_update(p.pos, p.tags, a0, a1, lane, com[0], com[1], com[2], dcom[0], dcom[1], dcom[2], drot[0], drot[1],
                          drot[2]);
}

__global__ void adf_step_system_finish_kernel(int32_t* state, int B) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        state[1] = state[0] >= B ? 1 : 0;
        state[4] += 1;
    }
}

int32_t adf_stepper_init(const adf_batch* b, float* pos, const int32_t* tags, const float* noise,
                         hipStream_t s) {
    hipLaunchKernelGGL(adf_init_placement_kernel, dim3(b->num_systems), dim3(64), 0, s, b->cell, b->atom_offset, tags,
                       pos, noise, b->num_systems);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}

int32_t adf_stepper_step(float* sys, const adf_batch* b, float* pos, const int32_t* tags, const int32_t* fixed,
                         const float* f1, const float* f2, const adf_step_coef* coef, const adf_step_coef* coefs_dev,
                         int num_steps, const float* z_tr, const float* z_rot, int32_t early_stop_count,
                         int32_t* state, float* dcom, float* drot, hipStream_t s, int32_t* sys_state, int32_t* hist_t) {
    StepParams p;
    p.cell = b->cell; p.atom_offset = b->atom_offset; p.tags = tags; p.fixed = fixed; p.pos = pos;
    p.f1 = f1; p.f2 = f2; p.z_tr = z_tr; p.z_rot = z_rot; p.sys = sys; p.state = state;
    p.dcom_out = dcom; p.drot_out = drot; p.B = b->num_systems; p.early_stop_count = early_stop_count;
    if (coef) p.c = *coef; else p.c = adf_step_coef{};
    p.coefs_dev = coefs_dev; p.num_steps = num_steps;
    if (sys_state) {   // two launches where the coupled rule needs three
        hipLaunchKernelGGL(adf_step_system_kernel, dim3(p.B), dim3(64), 0, s, p, sys_state);
        hipLaunchKernelGGL(adf_step_system_finish_kernel, dim3(1), dim3(64), 0, s, state, p.B);
        ADF_HIP_CHECK(hipGetLastError());
        return ADF_OK;
    }
    hipLaunchKernelGGL(adf_step_reduce_kernel, dim3(p.B), dim3(64), 0, s, p);
    if (hist_t) hipLaunchKernelGGL(adf_step_keep_flag_kernel, dim3(1), dim3(64), 0, s, state, hist_t);
    hipLaunchKernelGGL(adf_step_decide_kernel, dim3(1), dim3(64), 0, s, state, early_stop_count);
    hipLaunchKernelGGL(adf_step_apply_kernel, dim3(p.B), dim3(64), 0, s, p);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}

// ------------------------------------------------------------------------------------------ translation-only samplers
// Reference: denoising_torch.py
//   :96-196   reverse_sde_sampling  (probability-flow ODE: dcom = 0.5 g^2 dt * score)
//   :369-458  langevin_dynamics     (dcom = step_size * score + sqrt(2 step_size) * z, per noise level x inner step)
// Both take the per-system mean of head 1 over the tag-2 atoms (:460-467; no fixed-atom zeroing, that is head 2's),
// zero the z of the increment, wrap the COM exactly as adf_step_reduce_kernel does, and then add dcom to the adsorbate
// positions (set_positions, :52-56: `pos += update.float()`), not the rot sampler's ((pos - c) R^T + t) + c.
struct TrParams {
    const float* cell;
    const int32_t* atom_offset;
    const int32_t* tags;
    float* pos;
    const float* f1;
    const float* z;      // [B][3] standard normals (Langevin) or NULL (ODE)
    float* sys;          // [B][16]: com(3) dcom(3)
    int32_t* state;
    float* dcom_out;
    adf_tr_coef c;
    const adf_tr_coef* coefs_dev;  // optional schedule table on the device, indexed by state[4]
    int num_steps;
};

// sums over the tag-2 atoms of [a0, a1): pos(3) f1(3) count; every lane returns the same totals
__device__ __forceinline__ void tr_sums(const TrParams& p, int a0, int a1, int lane, float* s) {
#pragma unroll
    for (int i = 0; i < 7; ++i) s[i] = 0.f;
    for (int a = a0 + lane; a < a1; a += 64)
        if (p.tags[a] == 2) {
            s[0] += p.pos[3 * a]; s[1] += p.pos[3 * a + 1]; s[2] += p.pos[3 * a + 2];
            s[3] += p.f1[3 * a]; s[4] += p.f1[3 * a + 1]; s[5] += p.f1[3 * a + 2];
            s[6] += 1.f;
        }
#pragma unroll
    for (int i = 0; i < 7; ++i) s[i] = adf_wave_sum(s[i]);
}

// sums -> com and the wrapped dcom of system b; returns its convergence predicate
__device__ __forceinline__ bool tr_increment(const TrParams& p, int b, const float* s, float* com, float* dcom) {
    const float cnt = fmaxf(s[6], 1.0f);
    adf_tr_coef c = p.c;
    if (p.coefs_dev) c = p.coefs_dev[min(p.state[4], p.num_steps - 1)];
    for (int k = 0; k < 3; ++k) {
        com[k] = s[k] / cnt;
        float d = __fmul_rn(c.coef, s[3 + k] / cnt);
        // Langevin: noise = randn * sqrt(2 step_size) is its own f32 tensor, then added (:417-421)
        if (p.z) d = __fadd_rn(d, __fmul_rn(c.noise, p.z[3 * b + k]));
        dcom[k] = d;
    }
    dcom[2] = 0.f;
    const float tgt[3] = {__fadd_rn(com[0], dcom[0]), __fadd_rn(com[1], dcom[1]), __fadd_rn(com[2], dcom[2])};
    return step_wrap(p.cell + 9 * b, tgt, com, dcom);
}

// pos += dcom on the adsorbate of [a0, a1)
__device__ __forceinline__ void tr_update(float* pos, const int32_t* tags, int a0, int a1, int lane, float tx, float ty,
                                          float tz) {
    for (int a = a0 + lane; a < a1; a += 64)
        if (tags[a] == 2) {
            pos[3 * a] = __fadd_rn(pos[3 * a], tx);
            pos[3 * a + 1] = __fadd_rn(pos[3 * a + 1], ty);
            pos[3 * a + 2] = __fadd_rn(pos[3 * a + 2], tz);
        }
}

__global__ __launch_bounds__(64) void adf_tr_reduce_kernel(TrParams p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int a0 = p.atom_offset[b], a1 = p.atom_offset[b + 1];
    float s[7];
    tr_sums(p, a0, a1, lane, s);
    if (lane != 0) return;
    float com[3], dcom[3];
    const bool conv = tr_increment(p, b, s, com, dcom);
    float* o = p.sys + 16 * b;
    for (int k = 0; k < 3; ++k) { o[k] = com[k]; o[3 + k] = dcom[k]; }
    if (!conv) atomicAnd(&p.state[2], 0);
    if (p.dcom_out) for (int k = 0; k < 3; ++k) p.dcom_out[3 * b + k] = dcom[k];
}

__global__ __launch_bounds__(64) void adf_tr_apply_kernel(TrParams p) {
    if (p.state[1]) return;  // the reference's `break`
    const int b = blockIdx.x, lane = threadIdx.x;
    const int a0 = p.atom_offset[b], a1 = p.atom_offset[b + 1];
    const float* o = p.sys + 16 * b;
    tr_update(p.pos, p.tags, a0, a1, lane, o[3], o[4], o[5]);
}

// the per-system rule (adf_step_system_kernel) for the translation-only samplers
__global__ __launch_bounds__(64) void adf_tr_system_kernel(TrParams p, int32_t* sys_state, int early_stop_count) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int32_t* st = sys_state + 4 * b;
    const int cvg = st[0], frozen = st[1];
    if (frozen) {
        if (lane < 3 && p.dcom_out) p.dcom_out[3 * b + lane] = 0.f;
        return;
    }
    const int a0 = p.atom_offset[b], a1 = p.atom_offset[b + 1];
    float s[7];
    tr_sums(p, a0, a1, lane, s);
    float com[3], dcom[3];
    const bool conv = tr_increment(p, b, s, com, dcom);
    if (lane < 3 && p.dcom_out) p.dcom_out[3 * b + lane] = dcom[lane];
    if (system_decide(st, p.state, cvg, conv, early_stop_count, lane))
        tr_update(p.pos, p.tags, a0, a1, lane, dcom[0], dcom[1], dcom[2]);
}

int32_t adf_stepper_tr_step(float* sys, const adf_batch* b, float* pos, const int32_t* tags, const float* f1,
                            const adf_tr_coef* coef, const adf_tr_coef* coefs_dev, int num_steps, const float* z,
                            int32_t early_stop_count, int32_t* state, float* dcom, hipStream_t s, int32_t* sys_state) {
    TrParams p;
    p.cell = b->cell; p.atom_offset = b->atom_offset; p.tags = tags; p.pos = pos; p.f1 = f1; p.z = z; p.sys = sys;
    p.state = state; p.dcom_out = dcom;
    if (coef) p.c = *coef; else p.c = adf_tr_coef{};
    p.coefs_dev = coef ? nullptr : coefs_dev; p.num_steps = num_steps;
    const int B = b->num_systems;
    if (sys_state) {
        hipLaunchKernelGGL(adf_tr_system_kernel, dim3(B), dim3(64), 0, s, p, sys_state, early_stop_count);
        hipLaunchKernelGGL(adf_step_system_finish_kernel, dim3(1), dim3(64), 0, s, state, B);
        ADF_HIP_CHECK(hipGetLastError());
        return ADF_OK;
    }
    hipLaunchKernelGGL(adf_tr_reduce_kernel, dim3(B), dim3(64), 0, s, p);
    hipLaunchKernelGGL(adf_step_decide_kernel, dim3(1), dim3(64), 0, s, state, early_stop_count);
    hipLaunchKernelGGL(adf_tr_apply_kernel, dim3(B), dim3(64), 0, s, p);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}

// ------------------------------------------------------------------------------- the entries on a model's handle
int32_t adf_model_set_per_system_stop(int32_t** slot, int32_t* slot_B, int32_t* sys_state, int32_t B) {
    if (sys_state && B <= 0) { adf_set_error("set_per_system_stop: B must be positive"); return ADF_EINVAL; }
    *slot = sys_state;
    *slot_B = sys_state ? B : 0;
    return ADF_OK;
}
static int32_t check_per_system(const adf_model& m, const adf_batch* b) {
    if (m.sys_state && m.sys_B != b->num_systems) {
        adf_set_error("per-system stop is set for %d systems, the batch has %d", (int)m.sys_B, (int)b->num_systems);
        return ADF_EINVAL;
    }
    return ADF_OK;
}

int32_t adf_model_init_placement(const adf_model& m, const adf_batch* b, float* pos, const int32_t* tags,
                                 const float* noise, hipStream_t s) {
    ADF_TRY(m.check(m.h, b));
    if (!pos || !tags || !noise) { adf_set_error("null argument"); return ADF_EINVAL; }
    return adf_stepper_init(b, pos, tags, noise, s);
}

int32_t adf_model_sde_step(const adf_model& m, const adf_batch* b, float* pos, const int32_t* tags, const int32_t* fixed,
                           const float* f1, const float* f2, const adf_step_coef* coef, const adf_step_coef* coefs_dev,
                           int32_t num_steps, const float* z_tr, const float* z_rot, int32_t early_stop_count,
                           int32_t* state, float* dcom, float* drot, hipStream_t s, int32_t* hist_t) {
    ADF_TRY(m.check(m.h, b));
    if (!pos || !tags || !f1 || !f2 || (!coef && !coefs_dev) || !state) { adf_set_error("null argument"); return ADF_EINVAL; }
    if (!coef && num_steps <= 0) { adf_set_error("num_steps must be positive"); return ADF_EINVAL; }
    ADF_TRY(check_per_system(m, b));
    float* sys = nullptr;
    ADF_TRY(m.grow(m.h, b, &sys));
    m.prof(m.h, true, s);
    const int32_t st = adf_stepper_step(sys, b, pos, tags, fixed, f1, f2, coef, coef ? nullptr : coefs_dev, num_steps, z_tr,
                                        z_rot, early_stop_count, state, dcom, drot, s, m.sys_state, hist_t);
    m.prof(m.h, false, s);
    return st;
}

int32_t adf_model_tr_step(const adf_model& m, const adf_batch* b, float* pos, const int32_t* tags, const float* f1,
                          const adf_tr_coef* coef, const adf_tr_coef* coefs_dev, int32_t num_steps, const float* z,
                          int32_t early_stop_count, int32_t* state, float* dcom, hipStream_t s) {
    ADF_TRY(m.check(m.h, b));
    if (!pos || !tags || !f1 || (!coef && !coefs_dev) || !state) { adf_set_error("tr_step: null argument"); return ADF_EINVAL; }
    if (!coef && num_steps <= 0) { adf_set_error("tr_step: num_steps must be positive"); return ADF_EINVAL; }
    ADF_TRY(check_per_system(m, b));
    float* sys = nullptr;
    ADF_TRY(m.grow(m.h, b, &sys));
    m.prof(m.h, true, s);
    const int32_t st = adf_stepper_tr_step(sys, b, pos, tags, f1, coef, coefs_dev, num_steps, z, early_stop_count, state,
                                           dcom, s, m.sys_state);
    m.prof(m.h, false, s);
    return st;
}

// The whole reverse loop of every sampler on either model (denoising_torch.py:235-356, :96-196, :369-458) in one call:
// num_steps x (forward + step), all on `s`.  `step(z)` is the sampler's step on its noise tables' slices at offset z.
// Host round trips: with poll_every > 0 the frozen flag is read back every poll_every steps and the loop ends early,
// exactly like the reference's `break`.
template <class Step>
static int32_t sample_loop(const adf_model& m, const adf_batch* b, float* pos, const int32_t* tags, const void* coefs_dev,
                           int32_t num_steps, int32_t early_stop_count, int32_t poll_every, int32_t* state,
                           const int32_t* out_idx, int32_t n_out, float* f1, float* f2, adf_frames* sink,
                           int32_t frame_every, hipStream_t s, Step step) {
    ADF_TRY(m.check(m.h, b));
    if (num_steps <= 0 || !f1 || !state || !coefs_dev || !pos || !tags || (out_idx && n_out < 0)) {
        adf_set_error("sample: bad argument");
        return ADF_EINVAL;
    }
    if (sink && frame_every <= 0) { adf_set_error("sample: frame_every must be positive"); return ADF_EINVAL; }
    ADF_TRY(check_per_system(m, b));
    for (int t = 0; t < num_steps; ++t) {
        ADF_TRY(m.forward(m.h, b, out_idx, n_out, f1, f2, s));
        ADF_TRY(step((size_t)t * b->num_systems * 3));
        // trajectory frame of this step: snapshot on this stream, copy-out on the sink's stream (frames.hip)
        if (sink && ((t + 1) % frame_every == 0 || t + 1 == num_steps)) ADF_TRY(adf_frames_push_impl(sink, pos, s));
        if (early_stop_count > 0 && poll_every > 0 && (t % poll_every) == poll_every - 1 && t + 1 < num_steps) {
            int32_t frozen = 0;
            ADF_HIP_CHECK(hipMemcpyAsync(&frozen, state + 1, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            ADF_HIP_CHECK(hipStreamSynchronize(s));
            if (frozen) break;
        }
    }
    return ADF_OK;
}

int32_t adf_model_sample(const adf_model& m, const adf_batch* b, float* pos, const int32_t* tags, const int32_t* fixed,
                         const adf_step_coef* coefs_dev, int32_t num_steps, const float* z_tr_all, const float* z_rot_all,
                         int32_t early_stop_count, int32_t poll_every, int32_t* state, const int32_t* out_idx,
                         int32_t n_out, float* f1, float* f2, adf_frames* sink, int32_t frame_every, hipStream_t s) {
    if (!f2) { adf_set_error("sample: f2 is null"); return ADF_EINVAL; }
    if ((z_tr_all == nullptr) != (z_rot_all == nullptr)) { adf_set_error("sample: need both noise tables or none"); return ADF_EINVAL; }
    return sample_loop(m, b, pos, tags, coefs_dev, num_steps, early_stop_count, poll_every, state, out_idx, n_out, f1, f2,
                       sink, frame_every, s, [&](size_t z) {
                           return adf_model_sde_step(m, b, pos, tags, fixed, f1, f2, nullptr, coefs_dev, num_steps,
                                                     z_tr_all ? z_tr_all + z : nullptr, z_rot_all ? z_rot_all + z : nullptr,
                                                     early_stop_count, state, nullptr, nullptr, s);
                       });
}

int32_t adf_model_tr_sample(const adf_model& m, const adf_batch* b, float* pos, const int32_t* tags,
                            const adf_tr_coef* coefs_dev, int32_t num_steps, const float* z_all, int32_t early_stop_count,
                            int32_t poll_every, int32_t* state, const int32_t* out_idx, int32_t n_out, float* f1,
                            adf_frames* sink, int32_t frame_every, hipStream_t s) {
    return sample_loop(m, b, pos, tags, coefs_dev, num_steps, early_stop_count, poll_every, state, out_idx, n_out, f1,
                       nullptr, sink, frame_every, s, [&](size_t z) {
                           return adf_model_tr_step(m, b, pos, tags, f1, nullptr, coefs_dev, num_steps,
                                                    z_all ? z_all + z : nullptr, early_stop_count, state, nullptr, s);
                       });
}

// ---------------------------------------------------------------------------- two half-batches, two streams
// The join of a split run, one thread: the caller's state[] as the one-stream loop on the whole batch leaves it.
// st: view A's state (the caller's array), sb: view B's, init: the caller's state at the fork.
//   per-system rule: [0] frozen systems and [3] max steps applied are a sum / a maximum over the views, [1] all B frozen.
//   coupled rule (no early stop, nothing freezes): [0] counts the steps at which EVERY system had converged = the steps at
//   which both views' flags were set; [3] steps applied and [4] steps issued are the same on both views.
__global__ void adf_split_combine_kernel(int32_t* st, const int32_t* sb, const int32_t* init, const int32_t* hist_a,
                                         const int32_t* hist_b, int steps, int B, int per_system) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (per_system) {
        st[0] = st[0] + sb[0] - init[0];
        st[1] = st[0] >= B ? 1 : 0;
        st[3] = max(st[3], sb[3]);
        return;
    }
    int both = 0;
    for (int t = 0; t < steps; ++t) both += (hist_a[t] != 0 && hist_b[t] != 0) ? 1 : 0;
    st[0] = init[0] + both;
}

// sample_loop for two views of one batch cut at a system boundary: view A on its own (the caller's) stream with the model,
// view B on the pair's second stream with the twin.  One event forks B off A's stream at entry, one joins it before the
// return; in between the two chains share nothing: each has its handle, its state[] and its rows of every array.  The
// host enqueues step t of A, then step t of B, so both queues stay fed; it synchronises only where sample_loop does
// (the poll of the per-system early stop).  The noise tables are [step][system][3] over the WHOLE batch: a view reads
// its systems' rows of step t at t * total_systems * 3 + sys0 * 3.
int32_t adf_model_sample_split(const adf_model& mA, const adf_model& mB, adf_split_side A, adf_split_side B,
                               const adf_step_coef* coefs_dev, int32_t num_steps, const float* z_tr_all,
                               const float* z_rot_all, int32_t total_systems, int32_t early_stop_count, int32_t poll_every,
                               int32_t* state_init, hipEvent_t fork, hipEvent_t join) {
    ADF_TRY(mA.check(mA.h, A.b));
    ADF_TRY(mB.check(mB.h, B.b));
    if (num_steps <= 0 || !coefs_dev || !A.state || !B.state || !state_init || !A.f1 || !A.f2 || !A.pos || !A.tags) {
        adf_set_error("sample_split: bad argument");
        return ADF_EINVAL;
    }
    if ((z_tr_all == nullptr) != (z_rot_all == nullptr)) { adf_set_error("sample_split: need both noise tables or none"); return ADF_EINVAL; }
    ADF_TRY(check_per_system(mA, A.b));
    ADF_TRY(check_per_system(mB, B.b));
    const bool per_system = mA.sys_state != nullptr;
    if (!per_system && (!A.hist || !B.hist)) { adf_set_error("sample_split: no step history"); return ADF_EINVAL; }
    // fork: B's stream takes over from everything enqueued on A's so far; both views start from the caller's state
    ADF_HIP_CHECK(hipMemcpyAsync(state_init, A.state, 8 * sizeof(int32_t), hipMemcpyDeviceToDevice, A.s));
    ADF_HIP_CHECK(hipEventRecord(fork, A.s));
    ADF_HIP_CHECK(hipStreamWaitEvent(B.s, fork, 0));
    ADF_HIP_CHECK(hipMemcpyAsync(B.state, state_init, 8 * sizeof(int32_t), hipMemcpyDeviceToDevice, B.s));
    const size_t z_stride = (size_t)total_systems * 3;
    auto one = [&](const adf_model& m, const adf_split_side& v, int t) -> int32_t {
        ADF_TRY(m.forward(m.h, v.b, v.out_idx, v.out_idx ? v.n_out : 0, v.f1, v.f2, v.s));
        const size_t z = (size_t)t * z_stride + (size_t)v.sys0 * 3;
        return adf_model_sde_step(m, v.b, v.pos, v.tags, v.fixed, v.f1, v.f2, nullptr, coefs_dev, num_steps,
                                  z_tr_all ? z_tr_all + z : nullptr, z_rot_all ? z_rot_all + z : nullptr, early_stop_count,
                                  v.state, nullptr, nullptr, v.s, per_system ? nullptr : v.hist + t);
    };
    int32_t st = ADF_OK;
    int steps = 0;
    for (int t = 0; t < num_steps && st == ADF_OK; ++t) {
        st = one(mA, A, t);
        if (st == ADF_OK) st = one(mB, B, t);
        if (st != ADF_OK) break;
        steps = t + 1;
        if (early_stop_count > 0 && poll_every > 0 && (t % poll_every) == poll_every - 1 && t + 1 < num_steps) {
            int32_t fa = 0, fb = 0;   // all systems frozen = both views all frozen
            if (hipMemcpyAsync(&fa, A.state + 1, sizeof(int32_t), hipMemcpyDeviceToHost, A.s) != hipSuccess ||
                hipMemcpyAsync(&fb, B.state + 1, sizeof(int32_t), hipMemcpyDeviceToHost, B.s) != hipSuccess ||
                hipStreamSynchronize(A.s) != hipSuccess || hipStreamSynchronize(B.s) != hipSuccess) {
                adf_set_error("sample_split: reading the frozen flags failed: %s", hipGetErrorString(hipGetLastError()));
                st = ADF_EHIP;
                break;
            }
            if (fa && fb) break;
        }
    }
    // join - on an error too: the caller's stream must not run ahead of what B's stream still holds
    if (hipEventRecord(join, B.s) != hipSuccess || hipStreamWaitEvent(A.s, join, 0) != hipSuccess) {
        if (st == ADF_OK) { adf_set_error("sample_split: join failed: %s", hipGetErrorString(hipGetLastError())); st = ADF_EHIP; }
        return st;
    }
    if (st != ADF_OK) return st;
    hipLaunchKernelGGL(adf_split_combine_kernel, dim3(1), dim3(64), 0, A.s, A.state, B.state, state_init, A.hist, B.hist,
                       steps, total_systems, per_system ? 1 : 0);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}

// The cut of a split run (adsorbdiff_hip.h, "Two half-batches, two streams"): host arithmetic only.
extern "C" int32_t adf_split_choose_cut(const int32_t* natoms, const int64_t* edges, int32_t num_systems, int32_t* cut) {
    if (!natoms || !cut || num_systems < 0) { adf_set_error("split_choose_cut: bad argument"); return ADF_EINVAL; }
    *cut = 0;
    if (num_systems < 2) return ADF_OK;
    long long total = 0, etotal = 0;
    for (int b = 0; b < num_systems; ++b) {
        if (natoms[b] < 0 || (edges && edges[b] < 0)) { adf_set_error("split_choose_cut: negative count at system %d", b); return ADF_EINVAL; }
        total += natoms[b];
        if (edges) etotal += edges[b];
    }
    long long best = -1, best_e = -1, a = 0, e = 0;
    for (int c = 1; c < num_systems; ++c) {
        a += natoms[c - 1];
        if (edges) e += edges[c - 1];
        const long long d = llabs(2 * a - total), de = edges ? llabs(2 * e - etotal) : 0;
        if (best < 0 || d < best || (d == best && de < best_e)) { best = d; best_e = de; *cut = c; }
    }
    return ADF_OK;
}

// Hand-off rule of the reference's final-frame -> LMDB converter (scripts/create_lmdbs/pred_traj_to_lmdb.py:81-90): if the
// lowest adsorbate atom (tag 2) is less than `min_gap` above the highest surface atom (tag 1), the whole adsorbate is
// lifted by |diff| + min_gap.  One wave per system, in place; lifted[b] (optional) = applied shift.
__global__ __launch_bounds__(64) void adf_lift_kernel(float* pos, const int32_t* tags, const int32_t* atom_offset,
                                                       float min_gap, float* lifted) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int a0 = atom_offset[b], a1 = atom_offset[b + 1];
    float zs = -3.0e38f, za = 3.0e38f;
    for (int a = a0 + lane; a < a1; a += 64) {
        const float z = pos[3 * a + 2];
        if (tags[a] == 1) zs = fmaxf(zs, z);
        if (tags[a] == 2) za = fminf(za, z);
    }
    // kept inline: as a call to lanes.h this butterfly reorders the kernel's instructions (tools/device_asm_diff.py)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { zs = fmaxf(zs, __shfl_xor(zs, o)); za = fminf(za, __shfl_xor(za, o)); }
    float shift = 0.f;
    if (zs > -1.0e38f && za < 1.0e38f) {
        const float diff = za - zs;
        if (diff < min_gap) shift = fabsf(diff) + min_gap;
    }
    if (shift != 0.f)
        for (int a = a0 + lane; a < a1; a += 64)
            if (tags[a] == 2) pos[3 * a + 2] = pos[3 * a + 2] + shift;
    if (lifted && lane == 0) lifted[b] = shift;
}

extern "C" int32_t adf_lift_adsorbates(float* pos, const int32_t* tags, const int32_t* atom_offset, int32_t B, float min_gap,
                                       float* lifted, void* stream) {
    if (!pos || !tags || !atom_offset || B <= 0) { adf_set_error("lift_adsorbates: bad argument"); return ADF_EINVAL; }
    hipLaunchKernelGGL(adf_lift_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, pos, tags, atom_offset, min_gap, lifted);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}
