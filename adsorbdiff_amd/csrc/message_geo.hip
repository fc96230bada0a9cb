// Gradient of the energy with respect to the EDGE GEOMETRY of a PaiNN message block, for forces as the gradient of the
// energy (energy_grad.hip; the one piece the training step's backward never needed).
//
// Reference: torch.autograd.grad(energy.sum(), pos) through adsorbdiff/models/painn/painn.py:318-340 (distances and unit
// vectors from pos) and PaiNNMessage.forward / .message: the edge j -> i enters through rbfh = rbf_proj(rbf(d)) (distance)
// and through the c (x) r_hat term (unit vector).  Same point of view as message_bwd.hip: one wave walks the CSR segment of
// atom j in 32-row blocks and sees the REVERSE edge of every row (stored unit vector u, the message j -> i uses -u); with
// gx, g the packed gradient records of the neighbour i, (xa, xb, xc) = xh[j], w = vec[j] / sqrt3, S = g . w, T = -(g . u):
//   alpha_e = dE/dd   = sum_c [gx xa ra' + S xb rb' + T xc rc']     rbfh' = rbf_proj.weight . d(rbf)/dd  (no bias term)
//   b_e     = dE/d(-u) = sum_c g_c xc_c rc_c                          (a 3-vector)
// d(rbf_k)/dd = [env'(s) + env(s) 2 coeff (s - mu_k)] exp(coeff (s - mu_k)^2) / cutoff, s = d / cutoff.
// The kernel regenerates rbfh' on the matrix cores exactly as message_bwd.hip regenerates rbfh (same staged image of
// rbf_proj, same f16x3 split, same Gaussian recurrence with the derivative's factor applied per element, the bias column
// left out), then the c part of rbfh itself for b_e: 8 accumulator blocks per 32-row block, 6 + 2 in two sweeps, so that
// no more than 96 accumulators are live.  Sizing against the alternative (contract d(rbfh) with rbf_proj.weight on the
// matrix cores, then a banded dot with d(rbf)/dd): profiles/NOTES.md, "gradient forces".
//
// The four values of an edge row are sums over the channels: the 32 channel lanes of a half-wave hold 16 rows x 4 values
// each and reduce them with a transposing butterfly (5 steps, 32 + 16 + 8 + 4 + 2 exchanges instead of 64 x 5), after
// which lane q holds two finished values of row q / 2.  They are stored (first layer of an evaluation) or added (later
// layers: every (slice, row) is owned by exactly one wave of a launch and launches are stream-ordered) into
// part[slice][row] = (alpha, bx, by, bz): plain vector stores, fixed summation order, bit-reproducible.  The slices are
// summed in slice order by the position kernel (energy_grad.hip).
#include <stdlib.h>
#include <string.h>

#include "message.h"

struct MsgGeoParams {
    MsgParams m;          // rec = gradient records (adf_pack_grad_records)
    const float* xh;      // [N, 3H]
    const float* vec;     // [N, 3, H] or null (first layer: vec == 0)
    float4* part;         // [nslices][ecap] (alpha, bx, by, bz)
    long long ecap;
    int accumulate;
    float dcoef;          // 2 ln2 sarg: d/ds of exp2(-(sarg (s - mu))^2) = -dcoef t exp2(-t^2), t = sarg (s - mu)
};

#define GEO_BFLY(NV, MASK)                                             \
    {                                                                  \
        const bool up = (q & MASK) != 0;                               \
        _Pragma("unroll") for (int i = 0; i < NV / 2; ++i) {           \
            const float keep = up ? v[i + NV / 2] : v[i];              \
            const float send = up ? v[i] : v[i + NV / 2];              \
            v[i] = keep + __shfl_xor(send, MASK);                      \
        }                                                              \
    }

template <bool VZ>
__global__ __launch_bounds__(MSG_THREADS, 2) void adf_message_geo_kernel(MsgGeoParams pg) {
    const MsgParams& p = pg.m;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wfloats = (2 * MSG_COLS * MSG_LDK) / 2;
    _Float16* Wh = reinterpret_cast<_Float16*>(lds);       // [192][MSG_LDK] hi
    _Float16* Wlo = Wh + MSG_COLS * MSG_LDK;               // [192][MSG_LDK] lo
    float* Bl = lds + wfloats;
    float* Mu = Bl + MSG_COLS;
    float* Meta = Mu + 128;
    int* Ctr = reinterpret_cast<int*>(Meta + MSG_WAVES * 32 * 8);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int q = lane & 31;
    const int hi = lane >> 5;
    const int slice = blockIdx.x % p.nslices;
    const int worker = blockIdx.x / p.nslices;
    const int nworkers = gridDim.x / p.nslices;
    const int items = p.items;
    const int ngroups = (items + ADF_GROUP_NODES - 1) / ADF_GROUP_NODES;
    if (worker >= ngroups) return;
    const int H = p.H;
    const int c0 = slice * ADF_SLICE_CH;

    {   // stage this slice's rbf_proj image once (same image as the forward and backward kernels)
        const int R8 = p.R / 8;
        const half8* src = reinterpret_cast<const half8*>(p.wpack16 + (size_t)slice * 2 * MSG_COLS * p.R);
        const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        const _Float16* b16 = reinterpret_cast<const _Float16*>(p.bpack) + (size_t)slice * MSG_COLS * 2;
        for (int i = tid; i < 2 * MSG_COLS * 17; i += MSG_THREADS) {
            const int row = i / 17, piece = i - row * 17;
            half8 v = piece < R8 ? src[row * R8 + piece] : zero8;
            if (piece == 16 && row < MSG_COLS) { v[0] = b16[2 * row]; v[1] = b16[2 * row + 1]; }
            *reinterpret_cast<half8*>(Wh + (size_t)row * MSG_LDK + piece * 8) = v;
        }
        if (tid < 128) Mu[tid] = (tid < p.R ? p.mu[tid] : 2.0f) * p.sarg;
        if (tid == 0) *Ctr = 0;
    }
    __syncthreads();
    float* meta_w = Meta + wave * 32 * 8;
    const float inv_sqrt3 = 0.57735026918962576f;
    const float out_scale = *p.inv_scale * (1.0f / 256.0f);  // accumulators hold 256*scale*rbfh
    const float umax_scale = (float)(p.R - 1);
    const float dmu = 0.5f * p.dmu2;
    const unsigned int row_bytes = (unsigned int)p.nslices * 1280u;
    const char* recS = reinterpret_cast<const char*>(p.rec) + (size_t)slice * 1280;
    const unsigned int qA = (unsigned int)q * 16u;
    float4* part_s = pg.part + (size_t)slice * pg.ecap;

    auto fetch_target = [&](int& n_out) -> bool {
        while (true) {
            int t = 0;
            if (lane == 0) t = atomicAdd(Ctr, 1);
            t = __builtin_amdgcn_readfirstlane(t);
            const int g = worker + (t >> 5) * nworkers;
            if (g >= ngroups) return false;
            const int e = g * ADF_GROUP_NODES + (t & 31);
            if (e < items) { n_out = e; return true; }
        }
    };

    unsigned long long ksteps = 0;   // one add per wave at the end: an add per block on one address slows the kernel down
    int n = 0;
    while (fetch_target(n)) {
        const int e0 = p.nptr[n], e1 = p.nptr[n + 1];
        // per-atom constants of this lane's two channels (c0 + q, c0 + 32 + q)
        const float* xr = pg.xh + (size_t)n * 3 * H + c0 + q;
        const float xa0 = xr[0], xa1 = xr[32], xb0 = xr[H], xb1 = xr[H + 32], xc0 = xr[2 * H], xc1 = xr[2 * H + 32];
        float wx0 = 0.f, wy0 = 0.f, wz0 = 0.f, wx1 = 0.f, wy1 = 0.f, wz1 = 0.f;
        if (!VZ) {
            const float* vr = pg.vec + (size_t)n * 3 * H + c0 + q;
            wx0 = vr[0] * inv_sqrt3; wx1 = vr[32] * inv_sqrt3; wy0 = vr[H] * inv_sqrt3; wy1 = vr[H + 32] * inv_sqrt3;
            wz0 = vr[2 * H] * inv_sqrt3; wz1 = vr[2 * H + 32] * inv_sqrt3;
        }
        for (int eb = e0; eb < e1; eb += 32) {
            const int e = eb + q;
            const bool valid = e < e1;
            float4 geo = make_float4(0.f, 0.f, 0.f, 0.f);
            int src = 0;
            if (valid) { geo = p.e_geom[e]; src = p.e_src[e]; }
            const float xs = geo.w * p.inv_cutoff;
            // envelope and its derivative: env = 1 + a s^p + b s^(p+1) + c s^(p+2)
            float xq = 1.0f;   // s^(p-1)
            for (int i = 1; i < p.env_pi; ++i) xq *= xs;
            const float xp = xq * xs;
            const float pe = (float)p.env_pi;
            float env = 1.0f + p.env_a * xp + p.env_b * (xp * xs) + p.env_c * (xp * xs * xs);
            float envd = p.env_a * pe * xq + p.env_b * (pe + 1.0f) * xp + p.env_c * (pe + 2.0f) * (xp * xs);
            const bool in = xs < 1.0f && valid;
            env = in ? env : 0.0f;
            envd = in ? envd : 0.0f;
            __builtin_amdgcn_wave_barrier();
            if (hi == 0) {
                float* m = meta_w + q * 8;
                m[0] = __uint_as_float((unsigned int)(valid ? src : p.N) * row_bytes);
                m[1] = geo.x; m[2] = geo.y; m[3] = geo.z;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const float u = xs * umax_scale;
            const int nvalid = __builtin_amdgcn_readfirstlane(min(32, e1 - eb));
            const float umin = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u), 0));
            const float umax = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u), nvalid - 1));
            // band of the basis the block's rows reach (rows are sorted by distance); two centres wider on each side than the
            // forward's: the derivative's factor grows with the distance from the centre
            int klo = max(0, (int)floorf(umin) - 7) & ~7;
            int khi = min(p.R, (int)ceilf(umax) + 8);
            khi = klo + ((khi - klo + 15) & ~15);
            if (khi > 128) { klo -= khi - 128; khi = 128; }
            klo = __builtin_amdgcn_readfirstlane(klo);
            khi = __builtin_amdgcn_readfirstlane(khi);
            // profiling: contracted k length x 32-column blocks run (6 or 4 for rbfh', 2 for the c part), as message.hip counts
            ksteps += (unsigned long long)((khi - klo) * ((VZ ? 4 : 6) + 2));

#define ROW_OF(r) ((r & 3) + 8 * (r >> 2) + 4 * hi)
            float v[64];
            const float xsq = xs * p.sarg;
            const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            {   // ---- sweep 1: rbfh' (all parts) -> alpha
                f32x16 acc[6];
#pragma unroll
                for (int b = 0; b < 6; ++b) acc[b] = zero16;
                // the operand is 256 d(rbf)/ds; the 1 / cutoff of d/dd multiplies the finished sum (alpha_scale), so the fp16
                // operand does not depend on the cutoff: |256 env 2 ln2 sarg t exp2(-t^2)| <= 256 x 1.386 x 0.849 (R - 1) x
                // 0.515 = 2.0e4 at R = 128 (the handle's largest basis), |256 env'| <= 256 x 2.2: inside the fp16 range
                const float dp = 256.0f * envd;           // 256 env'(s)
                const float dc = 256.0f * env * pg.dcoef; // 256 env(s) 2 ln2 sarg
                int k0 = klo;
                do {
                    half8 ah, al;
                    const float t0 = xsq - Mu[k0 + 8 * hi];
                    float a = __builtin_amdgcn_exp2f(-(t0 * t0));
                    float r = __builtin_amdgcn_exp2f(fminf(p.dmu2 * t0 - p.dmusq, 64.0f));
                    float av[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        av[j] = a * (dp - dc * (t0 - (float)j * dmu));
                        a *= r;
                        r *= p.cstep;
                    }
#pragma unroll
                    for (int j = 0; j < 8; j += 2) {
                        typedef __fp16 h2_t __attribute__((ext_vector_type(2)));
                        const h2_t hh = __builtin_amdgcn_cvt_pkrtz(av[j], av[j + 1]);
                        const h2_t ll = __builtin_amdgcn_cvt_pkrtz(av[j] - (float)hh[0], av[j + 1] - (float)hh[1]);
                        ah[j] = (_Float16)hh[0]; ah[j + 1] = (_Float16)hh[1];
                        al[j] = (_Float16)ll[0]; al[j + 1] = (_Float16)ll[1];
                    }
                    const _Float16* wh = Wh + (size_t)q * MSG_LDK + k0 + 8 * hi;
                    const _Float16* wl = Wlo + (size_t)q * MSG_LDK + k0 + 8 * hi;
#pragma unroll
                    for (int b = 0; b < 6; ++b) {
                        if (VZ && (b == 2 || b == 3)) continue;   // vec == 0: S = 0
                        const half8 bh = *reinterpret_cast<const half8*>(wh + b * 32 * MSG_LDK);
                        const half8 bl = *reinterpret_cast<const half8*>(wl + b * 32 * MSG_LDK);
                        acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[b], 0, 0, 0);
                        acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[b], 0, 0, 0);
                        acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[b], 0, 0, 0);
                    }
                    k0 += 16;
                } while (k0 < khi);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float* m = meta_w + ROW_OF(r) * 8;
                    unsigned int o = __float_as_uint(m[0]);
                    // two rows' gathers in flight, not sixteen (which would not fit beside the 96 accumulators): the address
                    // of row r waits for the result of row r - 2
                    if (r >= 2) asm volatile("" : "+v"(o) : "v"(v[4 * (r - 2)]));
                    const float4 g0 = *reinterpret_cast<const float4*>(recS + (size_t)(o + qA));
                    const float4 g1 = *reinterpret_cast<const float4*>(recS + (size_t)(o + qA) + 640);
                    const float ux = m[1], uy = m[2], uz = m[3];
                    const float T0 = -(g0.x * ux + g0.y * uy + g0.z * uz);
                    const float T1 = -(g1.x * ux + g1.y * uy + g1.z * uz);
                    float al0 = g0.w * xa0 * acc[0][r] + T0 * xc0 * acc[4][r];
                    float al1 = g1.w * xa1 * acc[1][r] + T1 * xc1 * acc[5][r];
                    if (!VZ) {
                        const float S0 = g0.x * wx0 + g0.y * wy0 + g0.z * wz0;
                        const float S1 = g1.x * wx1 + g1.y * wy1 + g1.z * wz1;
                        al0 += S0 * xb0 * acc[2][r];
                        al1 += S1 * xb1 * acc[3][r];
                    }
                    v[4 * r] = al0 + al1;
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // keep the two sweeps apart: together they would not fit the registers
            {   // ---- sweep 2: the c part of rbfh itself (bias included) -> b
                f32x16 acc4, acc5;
                {
                    half8 aone = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (hi == 0) { aone[0] = (_Float16)256.0f; aone[1] = (_Float16)256.0f; }
                    const half8 b4 = *reinterpret_cast<const half8*>(Wh + (size_t)(4 * 32 + q) * MSG_LDK + 128);
                    const half8 b5 = *reinterpret_cast<const half8*>(Wh + (size_t)(5 * 32 + q) * MSG_LDK + 128);
                    acc4 = __builtin_amdgcn_mfma_f32_32x32x16_f16(aone, b4, zero16, 0, 0, 0);
                    acc5 = __builtin_amdgcn_mfma_f32_32x32x16_f16(aone, b5, zero16, 0, 0, 0);
                }
                const float env256 = env * 256.0f;
                int k0 = klo;
                do {
                    half8 ah, al;
                    const float t0 = xsq - Mu[k0 + 8 * hi];
                    float a = env256 * __builtin_amdgcn_exp2f(-(t0 * t0));
                    float r = __builtin_amdgcn_exp2f(fminf(p.dmu2 * t0 - p.dmusq, 64.0f));
                    float av[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        av[j] = a;
                        a *= r;
                        r *= p.cstep;
                    }
#pragma unroll
                    for (int j = 0; j < 8; j += 2) {
                        typedef __fp16 h2_t __attribute__((ext_vector_type(2)));
                        const h2_t hh = __builtin_amdgcn_cvt_pkrtz(av[j], av[j + 1]);
                        const h2_t ll = __builtin_amdgcn_cvt_pkrtz(av[j] - (float)hh[0], av[j + 1] - (float)hh[1]);
                        ah[j] = (_Float16)hh[0]; ah[j + 1] = (_Float16)hh[1];
                        al[j] = (_Float16)ll[0]; al[j + 1] = (_Float16)ll[1];
                    }
                    const _Float16* wh = Wh + (size_t)q * MSG_LDK + k0 + 8 * hi;
                    const _Float16* wl = Wlo + (size_t)q * MSG_LDK + k0 + 8 * hi;
                    {
                        const half8 bh = *reinterpret_cast<const half8*>(wh + 4 * 32 * MSG_LDK);
                        const half8 bl = *reinterpret_cast<const half8*>(wl + 4 * 32 * MSG_LDK);
                        acc4 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc4, 0, 0, 0);
                        acc4 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc4, 0, 0, 0);
                        acc4 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc4, 0, 0, 0);
                    }
                    {
                        const half8 bh = *reinterpret_cast<const half8*>(wh + 5 * 32 * MSG_LDK);
                        const half8 bl = *reinterpret_cast<const half8*>(wl + 5 * 32 * MSG_LDK);
                        acc5 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc5, 0, 0, 0);
                        acc5 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc5, 0, 0, 0);
                        acc5 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc5, 0, 0, 0);
                    }
                    k0 += 16;
                } while (k0 < khi);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float* m = meta_w + ROW_OF(r) * 8;
                    unsigned int o = __float_as_uint(m[0]);
                    // gathered again, not kept from sweep 1 (32 records would not fit the registers); two rows in flight
                    if (r >= 2) asm volatile("" : "+v"(o) : "v"(v[4 * (r - 2) + 1]));
                    else asm volatile("" : "+v"(o));
                    const float4 g0 = *reinterpret_cast<const float4*>(recS + (size_t)(o + qA));
                    const float4 g1 = *reinterpret_cast<const float4*>(recS + (size_t)(o + qA) + 640);
                    const float f0 = xc0 * acc4[r], f1 = xc1 * acc5[r];
                    v[4 * r + 1] = g0.x * f0 + g1.x * f1;
                    v[4 * r + 2] = g0.y * f0 + g1.y * f1;
                    v[4 * r + 3] = g0.z * f0 + g1.z * f1;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            // ---- channel sums: transposing butterfly over the 32 lanes of this half-wave; value index 4 r + c ends on lane
            // (4 r + c) / 2, so lane q holds (alpha, bx) (q even) or (by, bz) (q odd) of its row slot q / 2
            GEO_BFLY(64, 16) GEO_BFLY(32, 8) GEO_BFLY(16, 4) GEO_BFLY(8, 2) GEO_BFLY(4, 1)
            {
                const int r = q >> 1;
                const int row = ROW_OF(r);
                if (row < nvalid) {
                    float2* dst = reinterpret_cast<float2*>(part_s + (size_t)(eb + row)) + (q & 1);
                    // lane q even: (alpha, bx), odd: (by, bz); alpha carries the 1 / cutoff of d/dd
                    float2 o = make_float2(v[0] * ((q & 1) ? out_scale : out_scale * p.inv_cutoff), v[1] * out_scale);
                    if (pg.accumulate) { const float2 old = *dst; o.x += old.x; o.y += old.y; }
                    *dst = o;
                }
            }
#undef ROW_OF
            __builtin_amdgcn_wave_barrier();   // the next block rewrites this wave's meta rows
        }
    }
    if (p.kcount && lane == 0 && ksteps) atomicAdd(p.kcount, ksteps);
}

static size_t msgg_lds_bytes() {
    return (size_t)2 * MSG_COLS * MSG_LDK * 2 + sizeof(float) * (MSG_COLS + 128 + MSG_WAVES * 32 * 8) + 16;
}

bool adf_message_geo_supported(const adf_painn* h) {
    return h && h->weights_set && !h->msg_f32 && h->rbf_uniform && h->hp.num_rbf <= 128 && (h->hp.num_rbf % 8) == 0;
}

// part[nslices][ecap] (+)= the layer's per-edge-row (alpha, b); h->rec must hold the gradient records of this layer
// (adf_pack_grad_records, or a preceding adf_op_message_bwd_fused of the same gradients).
int32_t adf_message_geo(adf_painn* h, int layer, const float* xh, const float* vec, bool vec_is_zero, float4* part,
                        long long ecap, bool accumulate, hipStream_t s) {
    if (!h || h->lastN <= 0 || layer < 0 || layer >= h->hp.num_layers || !xh || !part || (!vec_is_zero && !vec)) {
        adf_set_error("message_geo: bad argument or no graph");
        return ADF_EINVAL;
    }
    if (!adf_message_geo_supported(h)) {
        adf_set_error("message_geo: needs the f16x3 arithmetic and equally spaced Gaussian centres");
        return ADF_EINVAL;
    }
    const int N = (int)h->lastN, H = h->hp.hidden_channels, R = h->hp.num_rbf;
    if ((unsigned long long)(N + 1) * 5ull * H * sizeof(float) >= (1ull << 32)) {
        adf_set_error("message kernel uses 32-bit byte offsets into the node tables: N=%d is too large, split the batch", N);
        return ADF_EOOM;
    }
    static bool attr_set = false;  // per process and device, as in message_bwd.hip
    if (!attr_set) {
        ADF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(adf_message_geo_kernel<false>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)msgg_lds_bytes()));
        ADF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(adf_message_geo_kernel<true>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)msgg_lds_bytes()));
        attr_set = true;
    }
    MsgGeoParams pg;
    memset(&pg, 0, sizeof(pg));
    MsgParams& p = pg.m;
    p.rec = h->rec; p.nptr = h->nptr; p.e_src = h->e_src; p.e_geom = h->e_geom;
    p.nslices = H / ADF_SLICE_CH;
    p.wpack16 = reinterpret_cast<const _Float16*>(h->rbf_pack16) + (size_t)layer * 2 * p.nslices * R * MSG_COLS;
    p.bpack = h->rbf_bias_pack16 + (size_t)layer * p.nslices * MSG_COLS;
    p.inv_scale = h->rbf_scales + layer;
    p.mu = h->rbf_offset;
    p.N = N; p.H = H; p.R = R; p.items = N;
    p.G = (N + ADF_GROUP_NODES - 1) / ADF_GROUP_NODES;
    p.inv_cutoff = 1.0f / h->hp.cutoff;
    const double step = 1.0 / (R - 1);
    const double sarg = sqrt(0.5 / (step * step) * 1.4426950408889634);
    p.sarg = (float)sarg;
    const double pe = (double)h->hp.envelope_exponent;
    p.env_pi = h->hp.envelope_exponent;
    p.env_a = (float)(-(pe + 1) * (pe + 2) / 2);
    p.env_b = (float)(pe * (pe + 2));
    p.env_c = (float)(-pe * (pe + 1) / 2);
    {
        const double d = sarg * step;
        p.dmu2 = (float)(2.0 * d); p.dmusq = (float)(d * d); p.cstep = (float)exp2(-2.0 * d * d);
    }
    pg.dcoef = (float)(2.0 * 0.69314718055994531 * sarg);
    p.kcount = h->prof.on ? h->kcount : nullptr;
    pg.xh = xh; pg.vec = vec; pg.part = part; pg.ecap = ecap; pg.accumulate = accumulate ? 1 : 0;
    int workers = h->num_cus / p.nslices;
    if (workers < 1) workers = 1;
    if (workers > p.G) workers = p.G;
    dim3 grid((unsigned)(workers * p.nslices));
    // the only launches of a gradient evaluation timed under this category, and the only ones that count k-steps
    // (energy_grad.hip switches the counter off around its forward message kernel)
    adf_prof_begin(h, ADF_PROF_MESSAGE, s);
    if (vec_is_zero) hipLaunchKernelGGL((adf_message_geo_kernel<true>), grid, dim3(MSG_THREADS), msgg_lds_bytes(), s, pg);
    else hipLaunchKernelGGL((adf_message_geo_kernel<false>), grid, dim3(MSG_THREADS), msgg_lds_bytes(), s, pg);
    adf_prof_end(h, s);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}
