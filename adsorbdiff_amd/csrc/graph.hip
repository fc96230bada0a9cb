// Periodic radius graph + strict top-K + symmetrisation, built on the device every forward.
//
// Reference semantics (all in adsorbdiff/):
//   utils/utils.py:556-730   radius_graph_pbc      candidates (centre i, neighbour j, lattice shift)
//                                                   with 1e-4 < d^2 <= rc^2, ordered by (i, j, shift)
//   utils/utils.py:733-853   get_max_neighbors_mask keep the K nearest per centre (strict)
//   utils/utils.py:513-553   get_pbc_distances      v = pos[j]-pos[i] + shift.cell, d = |v|
//   models/painn/painn_denoising.py:262-327         keep j<i (or same atom & lexicographically
//                                                   negative shift), append reversed copies
//
// MI355X design: the graph is integer/HBM-latency work, not GEMM work.
//   1. adf_topk_kernel: one wave per centre atom.  All n x n_shift candidates
//      of the centre's own system are evaluated from L2-resident positions; in-cutoff ones are
//      compacted into LDS (ballot + prefix popcount), then the K smallest are selected by rank counting on the key
//      (d^2, candidate index) — i.e. a *stable* sort order.  (The reference's torch.sort is not
//      stable, so for exact d^2 ties at the K-th place its pick is arbitrary; ours is the
//      lowest candidate index.  Everything else is bit-identical: d^2 is evaluated with the
//      reference's fp32 operation order, no FMA contraction.)  Survivors are written in
//      candidate order, which is the reference's edge order before symmetrisation.
//   2. count / scan / fill / sort: the symmetrised edge list is produced directly in the layout the
//      message kernel consumes — a CSR over *target* atoms (nptr[N+1]), each record = source index
//      + (unit vector target->source, d), every target's edges ordered by distance.
#include <hipcub/hipcub.hpp>

#include "common.h"
#include "graph.h"

// One wave per centre atom, 4 centres per workgroup.  Lane = neighbour atom j (64 per pass), inner
// loop over the lattice shifts; in-cutoff candidates are compacted into the wave's LDS list with
// ballot + prefix popcount (no atomics).  Selection of the K smallest keys (d^2, candidate index):
// every lane keeps its candidates in registers and counts, for each of them, how many list entries
// are smaller (entries are broadcast from LDS).  Survivors are emitted in candidate order.
//
// Static-atom cache (sampling: only adsorbate atoms move between reverse steps).  MODE 1 additionally
// stores, for every static centre, its K nearest *static* candidates; MODE 2 then rebuilds a static
// centre's list from that cache plus the candidates of the system's few moving atoms — any static
// candidate among the K nearest overall is among the K nearest static ones, so the result is
// identical to the full evaluation (same d^2 arithmetic, same keys) at ~1/50 of the work.  Moving
// centres are always evaluated in full.
#define TOPK_CAP 1024  // in-cutoff candidates per centre (a 12 A sphere in a dense bulk holds ~630)
#define MOVBIT 0x40000000

struct TopkLds {
    float d2[4][TOPK_CAP];
    int32_t id[4][TOPK_CAP];     // candidate index j*C + c, | MOVBIT when atom j moves
    float off[4][3 * 128];       // Cartesian offsets of the shift table (<= 125 shifts cached)
    int32_t kept[4][ADF_MAX_K];
};

// rank selection among entries with (id & skip_mask) == 0; returns per-lane keep bits for e = lane + 64 t.
// Order: (d^2, candidate index).  d^2 > 1e-4 > 0, so its bit pattern orders like the float and the pair packs into one
// 64-bit key: one compare per pair instead of three (round 6; the graph build of a reverse step spent 0.85 ms here).
// Lists of at most 64 entries (the static-atom path: K cached + the moving atoms' candidates) take the one-entry-per-lane
// form; longer ones keep four entries per lane.
__device__ __forceinline__ unsigned int topk_select(const TopkLds& L, int w, int lane, int M, int K, int skip_mask) {
    const int T = (M + 63) >> 6;  // <= 16
    unsigned int keepbits = 0;
    auto key_of = [&](int e) -> unsigned long long {
        return ((unsigned long long)__float_as_uint(L.d2[w][e]) << 32) | (unsigned int)(L.id[w][e] & ~MOVBIT);
    };
    if (T == 1) {
        const int raw = lane < M ? L.id[w][lane] : 0;
        const bool use = lane < M && (raw & skip_mask) == 0;
        const unsigned long long kq = use ? key_of(lane) : ~0ull;
        int rank = 0;
        for (int f = 0; f < M; ++f) {
            if (L.id[w][f] & skip_mask) continue;  // wave-uniform
            rank += key_of(f) < kq ? 1 : 0;
        }
        return (use && rank < K) ? 1u : 0u;
    }
    for (int t0 = 0; t0 < T; t0 += 4) {  // 4 entries of this lane at a time
        unsigned long long kq[4]; int rank[4]; bool use[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = lane + 64 * (t0 + u);
            const int raw = e < M ? L.id[w][e] : 0;
            use[u] = e < M && (raw & skip_mask) == 0;
            kq[u] = use[u] ? key_of(e) : ~0ull;
            rank[u] = 0;
        }
        for (int f = 0; f < M; ++f) {
            if (L.id[w][f] & skip_mask) continue;  // wave-uniform
            const unsigned long long kf = key_of(f);
#pragma unroll
            for (int u = 0; u < 4; ++u) rank[u] += kf < kq[u] ? 1 : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (use[u] && rank[u] < K) keepbits |= 1u << (t0 + u);
    }
    return keepbits;
}

template <int MODE>
__global__ __launch_bounds__(256) void adf_topk_kernel(GraphParams p) {
    __shared__ TopkLds L;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + w;
    if (i >= p.N) return;
    const int b = p.batch[i];
    const int a0 = p.atom_offset[b];
    const int n = p.atom_offset[b + 1] - a0;
    const int C = (2 * p.r0 + 1) * (2 * p.r1 + 1) * (2 * p.r2 + 1);
    const int K = p.K;
    const float* cl = p.cell + 9 * b;
    const float c00 = cl[0], c01 = cl[1], c02 = cl[2];
    const float c10 = cl[3], c11 = cl[4], c12 = cl[5];
    const float c20 = cl[6], c21 = cl[7], c22 = cl[8];
    const bool cached = C <= 128;
    if (cached) {
        for (int c = lane; c < C; c += 64) {
            float sa, sb, sc;
            decode_shift(c, p.r0, p.r1, p.r2, sa, sb, sc);
            // offset = cell^T . shift, summed in k order without FMA (utils.py:680-681)
            L.off[w][3 * c] = __fadd_rn(__fadd_rn(__fmul_rn(c00, sa), __fmul_rn(c10, sb)), __fmul_rn(c20, sc));
            L.off[w][3 * c + 1] = __fadd_rn(__fadd_rn(__fmul_rn(c01, sa), __fmul_rn(c11, sb)), __fmul_rn(c21, sc));
            L.off[w][3 * c + 2] = __fadd_rn(__fadd_rn(__fmul_rn(c02, sa), __fmul_rn(c12, sb)), __fmul_rn(c22, sc));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    const float pix = p.pos[3 * i], piy = p.pos[3 * i + 1], piz = p.pos[3 * i + 2];
    int M = 0;  // wave-uniform count of in-cutoff candidates

    // candidate (atom j of this system, shift c): evaluate with the reference's op order and append
    auto consider = [&](bool active, int j, int c, int movbit) {
        float ox, oy, oz;
        if (cached) {
            ox = L.off[w][3 * c]; oy = L.off[w][3 * c + 1]; oz = L.off[w][3 * c + 2];
        } else {
            float sa, sb, sc;
            decode_shift(c, p.r0, p.r1, p.r2, sa, sb, sc);
            ox = __fadd_rn(__fadd_rn(__fmul_rn(c00, sa), __fmul_rn(c10, sb)), __fmul_rn(c20, sc));
            oy = __fadd_rn(__fadd_rn(__fmul_rn(c01, sa), __fmul_rn(c11, sb)), __fmul_rn(c21, sc));
            oz = __fadd_rn(__fadd_rn(__fmul_rn(c02, sa), __fmul_rn(c12, sb)), __fmul_rn(c22, sc));
        }
        const float* pj = p.pos + 3 * (size_t)(a0 + (active ? j : 0));
        const float dx = __fsub_rn(pix, __fadd_rn(pj[0], ox));
        const float dy = __fsub_rn(piy, __fadd_rn(pj[1], oy));
        const float dz = __fsub_rn(piz, __fadd_rn(pj[2], oz));
        const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
        const bool in = active && d2 <= p.rc2 && d2 > 0.0001f;
        const unsigned long long mask = __ballot(in);
        if (in) {
            const int slot = M + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot < TOPK_CAP) { L.d2[w][slot] = d2; L.id[w][slot] = (j * C + c) | movbit; }
        }
        M += __popcll(mask);
    };

    const bool centre_moves = MODE == 0 ? true : (p.moving[i] != 0);
    if (MODE == 2 && !centre_moves) {
        // cached K nearest static candidates + every candidate of the system's moving atoms
        const int cnt = p.cache_cnt[i];
        for (int t = lane; t < cnt; t += 64) {
            L.d2[w][t] = p.cache_d2[(size_t)i * K + t];
            L.id[w][t] = p.cache_cid[(size_t)i * K + t];
        }
        M = cnt;
        const int m0 = p.mov_off[b], nm = p.mov_off[b + 1] - m0;
        const int npairs = nm * C;
        for (int q0 = 0; q0 < npairs; q0 += 64) {
            const int q = q0 + lane;
            const bool act = q < npairs;
            const int m = act ? q / C : 0;
            const int c = act ? q - m * C : 0;
            const int j = p.mov_idx[m0 + m] - a0;
            consider(act, j, c, MOVBIT);
        }
    } else {
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            const bool jv = j < n;
            const int movbit = (MODE == 1 && jv && p.moving[a0 + j]) ? MOVBIT : 0;
            for (int c = 0; c < C; ++c) consider(jv, j, c, movbit);
        }
    }
    if (M > TOPK_CAP) {
        if (lane == 0) atomicExch(&p.flags[0], 1);
        M = TOPK_CAP;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int T = (M + 63) >> 6;

    if (MODE == 1 && !centre_moves) {  // cache: the K nearest among static candidates
        const unsigned int kb = topk_select(L, w, lane, M, K, MOVBIT);
        int nc = 0;
        for (int t = 0; t < T; ++t) {
            const int e = lane + 64 * t;
            const bool kp = e < M && ((kb >> t) & 1u);
            const unsigned long long mask = __ballot(kp);
            if (kp) {
                const int slot = nc + __popcll(mask & ((1ull << lane) - 1ull));
                p.cache_d2[(size_t)i * K + slot] = L.d2[w][e];
                p.cache_cid[(size_t)i * K + slot] = L.id[w][e];
            }
            nc += __popcll(mask);
        }
        if (lane == 0) p.cache_cnt[i] = nc;
    }

    const unsigned int keepbits = M <= K ? 0xFFFFu : topk_select(L, w, lane, M, K, 0);
    // survivors in candidate order: position = number of survivors with a smaller candidate index
    int nk = 0;
    for (int t = 0; t < T; ++t) {
        const int e = lane + 64 * t;
        const bool kp = e < M && ((keepbits >> t) & 1u);
        const unsigned long long mask = __ballot(kp);
        if (kp) L.kept[w][nk + __popcll(mask & ((1ull << lane) - 1ull))] = L.id[w][e] & ~MOVBIT;
        nk += __popcll(mask);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int t = lane; t < nk; t += 64) {
        const int id = L.kept[w][t];
        int posn = 0;
        for (int f = 0; f < nk; ++f) posn += L.kept[w][f] < id;
        const int j = id / C;
        p.nbr_src[(size_t)i * K + posn] = a0 + j;
        p.nbr_shift[(size_t)i * K + posn] = id - j * C;
    }
    if (lane == 0) {
        p.nbr_cnt[i] = nk;
        if (nk) atomicAdd(&p.img_cnt[b], nk);
    }
}

__device__ __forceinline__ bool edge_kept(int j, int i, int c, int r0, int r1, int r2) {
    if (j < i) return true;
    if (j != i) return false;
    float sa, sb, sc;
    decode_shift(c, r0, r1, r2, sa, sb, sc);
    return (sa < 0.f) || (sa == 0.f && sb < 0.f) || (sa == 0.f && sb == 0.f && sc < 0.f);
}

// only: null = every system; else the systems flagged in it (the ones the per-system LDS kernels below passed on)
__global__ void adf_count_kernel(GraphParams p, int32_t* deg, const int32_t* __restrict__ only) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(t / p.K);
    const int k = (int)(t - (long long)i * p.K);
    if (i >= p.N || k >= p.nbr_cnt[i]) return;
    if (only && !only[p.batch[i]]) return;
    const int j = p.nbr_src[(size_t)i * p.K + k];
    const int c = p.nbr_shift[(size_t)i * p.K + k];
    if (!edge_kept(j, i, c, p.r0, p.r1, p.r2)) return;
    atomicAdd(&deg[i], 1);
    atomicAdd(&deg[j], 1);
}

// validates capacities / empty images after the scan
__global__ void adf_validate_kernel(const int32_t* nptr, int N, long long capE, const int32_t* img_cnt, int B,
                                    int32_t* flags) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0 && (long long)nptr[N] > capE) atomicExch(&flags[2], 1);
    if (t < B && img_cnt[t] == 0) atomicExch(&flags[1], 1);
}

__global__ void adf_fill_kernel(GraphParams p, const int32_t* nptr, int32_t* cursor, int32_t* e_src, float4* e_geom,
                                long long capE, const int32_t* __restrict__ only) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(t / p.K);
    const int k = (int)(t - (long long)i * p.K);
    if (i >= p.N || k >= p.nbr_cnt[i]) return;
    if (only && !only[p.batch[i]]) return;
    const int j = p.nbr_src[(size_t)i * p.K + k];
    const int c = p.nbr_shift[(size_t)i * p.K + k];
    if (!edge_kept(j, i, c, p.r0, p.r1, p.r2)) return;
    float sa, sb, sc;
    decode_shift(c, p.r0, p.r1, p.r2, sa, sb, sc);
    const float* cl = p.cell + 9 * p.batch[i];
    // shift (row vector) . cell   (utils.py:529)
    const float ox = __fadd_rn(__fadd_rn(__fmul_rn(sa, cl[0]), __fmul_rn(sb, cl[3])), __fmul_rn(sc, cl[6]));
    const float oy = __fadd_rn(__fadd_rn(__fmul_rn(sa, cl[1]), __fmul_rn(sb, cl[4])), __fmul_rn(sc, cl[7]));
    const float oz = __fadd_rn(__fadd_rn(__fmul_rn(sa, cl[2]), __fmul_rn(sb, cl[5])), __fmul_rn(sc, cl[8]));
    const float vx = __fadd_rn(__fsub_rn(p.pos[3 * j], p.pos[3 * i]), ox);
    const float vy = __fadd_rn(__fsub_rn(p.pos[3 * j + 1], p.pos[3 * i + 1]), oy);
    const float vz = __fadd_rn(__fsub_rn(p.pos[3 * j + 2], p.pos[3 * i + 2]), oz);
    float d = sqrtf(fmaf(vz, vz, fmaf(vy, vy, vx * vx)));
    // utils.py:536-540 drops d == 0 edges: unreachable after the d^2 > 1e-4 filter, so not handled
    if (fabsf(d) <= p.dist_floor) d = p.dist_floor;  // painn_denoising.py:366-367 / painn.py:334-335
    const float ux = vx / d, uy = vy / d, uz = vz / d;
    // edge j -> i, stored in the segment of its target i
    long long slot = (long long)nptr[i] + atomicAdd(&cursor[i], 1);
    if (slot < capE) { e_src[slot] = j; e_geom[slot] = make_float4(ux, uy, uz, d); }
    // reversed copy i -> j, same distance, negated unit vector (painn_denoising.py:171-181,322-327)
    slot = (long long)nptr[j] + atomicAdd(&cursor[j], 1);
    if (slot < capE) { e_src[slot] = i; e_geom[slot] = make_float4(-ux, -uy, -uz, d); }
}

// Order every target's incoming edges by distance (ties: source index, then unit vector), one wave
// per target.  Two reasons: (1) a 32-edge row block of the message kernel then spans a narrow band of
// the Gaussian basis, which shrinks the k-window it has to contract over; (2) the order no longer
// depends on the atomic cursor above, so the segmented sums are run-to-run reproducible.
#define SORT_MAX 256
__device__ __forceinline__ bool edge_before(const float4& h, int sf, const float4& g, int sj) {
    if (h.w != g.w) return h.w < g.w;
    if (sf != sj) return sf < sj;
    if (h.x != g.x) return h.x < g.x;
    if (h.y != g.y) return h.y < g.y;
    return h.z < g.z;
}

__global__ __launch_bounds__(256) void adf_sort_edges_kernel(const int32_t* nptr, int32_t* e_src, float4* e_geom,
                                                              int N, int32_t* flags, const int32_t* __restrict__ only,
                                                              const int32_t* __restrict__ batch) {
    __shared__ float4 s_geo[4][SORT_MAX];
    __shared__ int32_t s_src[4][SORT_MAX];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + w;
    if (n >= N) return;
    if (only && !only[batch[n]]) return;
    const int e0 = nptr[n];
    int deg = nptr[n + 1] - e0;
    // In-degree = own kept entries (<= K) + every centre that lists this atom, so only sum(deg) <= 2NK is bounded:
    // a hub atom can exceed 2K.  Up to SORT_MAX the segment is ranked out of LDS; up to ADF_MAX_INDEG each lane keeps
    // its <= 16 records in registers and ranks them against the (still unmodified) global segment, then all lanes
    // write; beyond that the message kernel's distance-ordered k-window would be wrong: flagged (ADF_EOVERFLOW).
    if (deg > SORT_MAX) {
        if (deg > ADF_MAX_INDEG) {
            if (lane == 0) atomicExch(&flags[3], 1);
            deg = ADF_MAX_INDEG;
        }
        float4 g[ADF_MAX_INDEG / 64]; int sj[ADF_MAX_INDEG / 64]; int rk[ADF_MAX_INDEG / 64];
#pragma unroll
        for (int u = 0; u < ADF_MAX_INDEG / 64; ++u) {
            const int t = lane + 64 * u;
            g[u] = t < deg ? e_geom[e0 + t] : make_float4(0.f, 0.f, 0.f, 0.f);
            sj[u] = t < deg ? e_src[e0 + t] : 0;
            rk[u] = 0;
        }
        for (int f = 0; f < deg; ++f) {
            const float4 hh = e_geom[e0 + f];
            const int sf = e_src[e0 + f];
#pragma unroll
            for (int u = 0; u < ADF_MAX_INDEG / 64; ++u) rk[u] += edge_before(hh, sf, g[u], sj[u]) ? 1 : 0;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int u = 0; u < ADF_MAX_INDEG / 64; ++u)
            if (lane + 64 * u < deg) { e_geom[e0 + rk[u]] = g[u]; e_src[e0 + rk[u]] = sj[u]; }
        return;
    }
    for (int t = lane; t < deg; t += 64) { s_geo[w][t] = e_geom[e0 + t]; s_src[w][t] = e_src[e0 + t]; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int t = lane; t < deg; t += 64) {
        const float4 g = s_geo[w][t];
        const int sj = s_src[w][t];
        int rank = 0;
        for (int f = 0; f < deg; ++f) {
            const float4 h = s_geo[w][f];
            const int sf = s_src[w][f];
            rank += edge_before(h, sf, g, sj) ? 1 : 0;
        }
        e_geom[e0 + rank] = g;
        e_src[e0 + rank] = sj;
    }
}

// ---- Round 6: count / fill / sort of a whole system out of LDS (one workgroup per system).
// The global-memory pipeline above spends its time on atomics and scattered 20-byte stores (count 0.33 + fill 0.80 + sort
// 0.39 ms per build of 1000 x 200 atoms).  A system of <= CSR_SYS_MAX atoms fits a workgroup: its kept directed entries
// are dealt to their SOURCE atom's bucket in LDS (16-bit references: owner of the list, slot), and one wave per target then
// forms the target's records - its own kept entries plus the reversed copies of the bucket's - with the fill kernel's
// arithmetic, ranks them with the sort kernel's order and writes the segment once, coalesced.  Same nptr / e_src / e_geom,
// bit for bit (tests/test_gpu_parity.py graph fixtures, test_system_csr_kernels_equal_the_global_pipeline).  A system
// that does not fit (more atoms, longer lists or more lattice shifts than the 16-bit references hold, a bucket beyond
// CSR_REF_CAP, a target beyond CSR_SEG_MAX records) is flagged and goes through the global-memory kernels, which skip
// every other system.  The second kernel also keeps the system's directed lists and positions in LDS, so a target's
// records are formed without a global load (first version, lists and positions from L2: 1.14 ms per build, no gain).
#define CSR_SYS_MAX 256    // atoms per system
#define CSR_K_MAX 64       // directed list length (max_neighbors)
#define CSR_C_MAX 256      // lattice shifts (a reference is 8 bits of atom + 8 bits of shift)
#define CSR_REF_CAP 96     // kept entries of OTHER atoms' lists naming one atom as their source
#define CSR_SEG_MAX 128    // records of one target the per-wave sorter holds

__device__ __forceinline__ bool csr_fits(const GraphParams& p, int n) {
    return n <= CSR_SYS_MAX && p.K <= CSR_K_MAX && (2 * p.r0 + 1) * (2 * p.r1 + 1) * (2 * p.r2 + 1) <= CSR_C_MAX;
}

__global__ __launch_bounds__(256) void adf_count_sys_kernel(GraphParams p, int32_t* __restrict__ deg, int32_t* __restrict__ slow) {
    __shared__ int32_t cnt[CSR_SYS_MAX];
    const int b = blockIdx.x;
    const int a0 = p.atom_offset[b], n = p.atom_offset[b + 1] - a0;
    if (!csr_fits(p, n)) {
        if (threadIdx.x == 0) slow[b] = 1;   // adf_count_kernel takes this system
        return;
    }
    if (threadIdx.x == 0) slow[b] = 0;
    for (int t = threadIdx.x; t < n; t += 256) cnt[t] = 0;
    __syncthreads();
    const int K = p.K;
    for (int sl = threadIdx.x; sl < n * K; sl += 256) {
        const int il = sl / K, k = sl - il * K, i = a0 + il;
        if (k >= p.nbr_cnt[i]) continue;
        const int j = p.nbr_src[(size_t)i * K + k];
        const int c = p.nbr_shift[(size_t)i * K + k];
        if (!edge_kept(j, i, c, p.r0, p.r1, p.r2)) continue;
        atomicAdd(&cnt[il], 1);
        atomicAdd(&cnt[j - a0], 1);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < n; t += 256) deg[a0 + t] = cnt[t];
}

struct CsrLds {
    unsigned short ent[CSR_SYS_MAX][CSR_K_MAX];     // directed lists of the system: (local source << 8) | shift
    unsigned short refs[CSR_SYS_MAX][CSR_REF_CAP];  // per source atom: (local owner of the list << 8) | shift, kept entries only
    int32_t rcnt[CSR_SYS_MAX];
    unsigned char ncnt[CSR_SYS_MAX];
    float pos[CSR_SYS_MAX * 3];
    float4 s_geo[16][CSR_SEG_MAX];
    int32_t s_src[16][CSR_SEG_MAX];
    unsigned long long s_key[16][CSR_SEG_MAX];      // (distance bits << 32) | source: the leading two fields of the sort order
    int32_t bad;
};

// the record of directed entry (centre i, source j, shift c) as adf_fill_kernel forms it: (unit vector i -> j, distance);
// il, jl: local indices into the LDS copy of the system's positions (the same floats)
__device__ __forceinline__ float4 csr_edge_geom(const GraphParams& p, const float* __restrict__ cl, const float* spos, int il,
                                                int jl, int c) {
    float sa, sb, sc;
    decode_shift(c, p.r0, p.r1, p.r2, sa, sb, sc);
    const float ox = __fadd_rn(__fadd_rn(__fmul_rn(sa, cl[0]), __fmul_rn(sb, cl[3])), __fmul_rn(sc, cl[6]));
    const float oy = __fadd_rn(__fadd_rn(__fmul_rn(sa, cl[1]), __fmul_rn(sb, cl[4])), __fmul_rn(sc, cl[7]));
    const float oz = __fadd_rn(__fadd_rn(__fmul_rn(sa, cl[2]), __fmul_rn(sb, cl[5])), __fmul_rn(sc, cl[8]));
    const float vx = __fadd_rn(__fsub_rn(spos[3 * jl], spos[3 * il]), ox);
    const float vy = __fadd_rn(__fsub_rn(spos[3 * jl + 1], spos[3 * il + 1]), oy);
    const float vz = __fadd_rn(__fsub_rn(spos[3 * jl + 2], spos[3 * il + 2]), oz);
    float d = sqrtf(fmaf(vz, vz, fmaf(vy, vy, vx * vx)));
    if (fabsf(d) <= p.dist_floor) d = p.dist_floor;
    return make_float4(vx / d, vy / d, vz / d, d);
}

__global__ __launch_bounds__(1024) void adf_fill_sort_sys_kernel(GraphParams p, const int32_t* __restrict__ nptr,
                                                                  int32_t* __restrict__ e_src, float4* __restrict__ e_geom,
                                                                  long long capE, int32_t* __restrict__ slow) {
    __shared__ CsrLds L;
    const int b = blockIdx.x;
    if (slow[b]) return;   // does not fit: the global-memory kernels build this system
    const int a0 = p.atom_offset[b], n = p.atom_offset[b + 1] - a0;
    const int K = p.K, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const float* cl = p.cell + 9 * b;
    for (int t = tid; t < n; t += 1024) { L.rcnt[t] = 0; L.ncnt[t] = (unsigned char)p.nbr_cnt[a0 + t]; }
    for (int t = tid; t < 3 * n; t += 1024) L.pos[t] = p.pos[3 * (size_t)a0 + t];
    if (tid == 0) L.bad = 0;
    __syncthreads();
    // 1. the system's directed lists -> LDS; every kept entry (i, k) also -> the bucket of its source j
    for (int sl = tid; sl < n * K; sl += 1024) {
        const int il = sl / K, k = sl - il * K, i = a0 + il;
        if (k >= (int)L.ncnt[il]) continue;
        const int j = p.nbr_src[(size_t)i * K + k];
        const int c = p.nbr_shift[(size_t)i * K + k];
        L.ent[il][k] = (unsigned short)(((j - a0) << 8) | c);
        if (!edge_kept(j, i, c, p.r0, p.r1, p.r2)) continue;
        const int r = atomicAdd(&L.rcnt[j - a0], 1);
        if (r < CSR_REF_CAP) L.refs[j - a0][r] = (unsigned short)((il << 8) | c);
        else L.bad = 1;
    }
    // a segment beyond the per-wave sorter, or beyond the edge capacity (flag 2 is raised by adf_validate_kernel)
    for (int t = tid; t < n; t += 1024) {
        const int dg = nptr[a0 + t + 1] - nptr[a0 + t];
        if (dg > CSR_SEG_MAX || (long long)nptr[a0 + t + 1] > capE) L.bad = 1;
    }
    __syncthreads();
    if (L.bad) {
        if (tid == 0) slow[b] = 1;   // adf_fill_kernel + adf_sort_edges_kernel take this system
        return;
    }
    // 2. one wave per target: gather, rank, write
    for (int tl = w; tl < n; tl += 16) {
        const int t = a0 + tl;
        const int e0 = nptr[t], dg = nptr[t + 1] - e0;
        // own kept entries: edge j -> t, compacted by ballot (the order inside a segment is settled by the ranks)
        int m = 0;
        const int own = (int)L.ncnt[tl];
        for (int k0 = 0; k0 < own; k0 += 64) {
            const int k = k0 + lane;
            bool keep = false;
            int jl = 0, c = 0;
            if (k < own) {
                const int e = L.ent[tl][k];
                jl = e >> 8; c = e & 255;
                keep = edge_kept(a0 + jl, t, c, p.r0, p.r1, p.r2);
            }
            const unsigned long long bal = __ballot(keep);
            if (keep) {
                const int at = m + __popcll(bal & ((1ull << lane) - 1ull));
                const float4 g = csr_edge_geom(p, cl, L.pos, tl, jl, c);
                L.s_geo[w][at] = g;
                L.s_src[w][at] = a0 + jl;
                L.s_key[w][at] = ((unsigned long long)__float_as_uint(g.w) << 32) | (unsigned int)(a0 + jl);
            }
            m += __popcll(bal);
        }
        // reversed copies of the entries that name t as their source: src = the list's owner, negated unit vector
        const int nr = L.rcnt[tl];
        for (int r = lane; r < nr; r += 64) {
            const int ref = L.refs[tl][r];
            const int il = ref >> 8, c = ref & 255;
            const float4 g = csr_edge_geom(p, cl, L.pos, il, tl, c);
            L.s_geo[w][m + r] = make_float4(-g.x, -g.y, -g.z, g.w);
            L.s_src[w][m + r] = a0 + il;
            L.s_key[w][m + r] = ((unsigned long long)__float_as_uint(g.w) << 32) | (unsigned int)(a0 + il);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int q = lane; q < dg; q += 64) {
            const float4 g = L.s_geo[w][q];
            const int sj = L.s_src[w][q];
            // rank on the 64-bit (distance, source) key (distances are positive: their bit patterns order like the floats);
            // only records that share both - lattice images of one atom at one distance - need the full comparison
            const unsigned long long kq = L.s_key[w][q];
            int rank = 0, eq = 0;
            for (int f = 0; f < dg; ++f) {
                const unsigned long long kf = L.s_key[w][f];
                rank += kf < kq ? 1 : 0;
                eq += kf == kq ? 1 : 0;
            }
            if (eq > 1) {
                rank = 0;
                for (int f = 0; f < dg; ++f) rank += edge_before(L.s_geo[w][f], L.s_src[w][f], g, sj) ? 1 : 0;
            }
            e_geom[e0 + rank] = g;
            e_src[e0 + rank] = sj;
        }
        __builtin_amdgcn_wave_barrier();   // the wave's scratch is refilled by its next target
    }
}

// The directed strict top-K stage alone (the EquiformerV2 path uses it without the symmetrisation): mode 0 full
// evaluation, 1 full + fill the static-atom cache, 2 rebuild static centres from the cache.
int32_t adf_topk_launch(const GraphParams& p, int mode, hipStream_t s) {
    const dim3 tg((p.N + 3) / 4);
    if (mode == 0) hipLaunchKernelGGL(adf_topk_kernel<0>, tg, dim3(256), 0, s, p);
    else if (mode == 1) hipLaunchKernelGGL(adf_topk_kernel<1>, tg, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(adf_topk_kernel<2>, tg, dim3(256), 0, s, p);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}

int32_t adf_graph_build_impl(adf_painn* h, const adf_batch* b, hipStream_t s) {
    ++h->build_serial;
    const int N = b->num_atoms, B = b->num_systems, K = h->hp.max_neighbors;
    GraphParams p;
    p.pos = b->pos; p.cell = b->cell; p.batch = b->batch; p.atom_offset = b->atom_offset;
    p.r0 = b->reps[0]; p.r1 = b->reps[1]; p.r2 = b->reps[2];
    p.rc2 = h->hp.cutoff * h->hp.cutoff;
    p.dist_floor = h->dist_floor;
    p.K = K; p.N = N;
    p.nbr_cnt = h->nbr_cnt; p.nbr_src = h->nbr_src; p.nbr_shift = h->nbr_shift;
    p.img_cnt = h->img_cnt;
    p.flags = h->flags;
    ADF_HIP_CHECK(hipMemsetAsync(h->deg, 0, sizeof(int32_t) * (N + 1), s));
    ADF_HIP_CHECK(hipMemsetAsync(h->cursor, 0, sizeof(int32_t) * N, s));
    ADF_HIP_CHECK(hipMemsetAsync(h->img_cnt, 0, sizeof(int32_t) * B, s));
    // static-atom cache: valid for the same batch as long as only atoms flagged `moving` moved
    p.moving = h->moving; p.mov_idx = h->mov_idx; p.mov_off = h->mov_off;
    p.cache_d2 = h->cache_d2; p.cache_cid = h->cache_cid; p.cache_cnt = h->cache_cnt;
    const dim3 tg((N + 3) / 4);
    if (!h->moving) {
        hipLaunchKernelGGL(adf_topk_kernel<0>, tg, dim3(256), 0, s, p);
    } else if (!h->cache_valid) {
        hipLaunchKernelGGL(adf_topk_kernel<1>, tg, dim3(256), 0, s, p);
        h->cache_valid = true;
    } else {
        hipLaunchKernelGGL(adf_topk_kernel<2>, tg, dim3(256), 0, s, p);
    }
    const long long slots = (long long)N * K;
    const unsigned nb = (unsigned)((slots + 255) / 256);
    // count / fill / sort: per system out of LDS (above); systems that do not fit go through the global-memory kernels
    const int32_t* only = nullptr;
    if (h->sw.tune.graph_sys_csr) {
        hipLaunchKernelGGL(adf_count_sys_kernel, dim3(B), dim3(256), 0, s, p, h->deg, h->sys_slow);
        only = h->sys_slow;
    }
    hipLaunchKernelGGL(adf_count_kernel, dim3(nb), dim3(256), 0, s, p, h->deg, only);
    size_t tmp = h->scan_tmp_bytes;
    ADF_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(h->scan_tmp, tmp, h->deg, h->nptr, N + 1, s));
    const int vb = (max(B, 1) + 255) / 256;
    hipLaunchKernelGGL(adf_validate_kernel, dim3(vb), dim3(256), 0, s, h->nptr, N, (long long)h->capE, h->img_cnt, B,
                       h->flags);
    if (only)
        hipLaunchKernelGGL(adf_fill_sort_sys_kernel, dim3(B), dim3(1024), 0, s, p, h->nptr, h->e_src, h->e_geom,
                           (long long)h->capE, h->sys_slow);
    hipLaunchKernelGGL(adf_fill_kernel, dim3(nb), dim3(256), 0, s, p, h->nptr, h->cursor, h->e_src, h->e_geom,
                       (long long)h->capE, only);
    hipLaunchKernelGGL(adf_sort_edges_kernel, dim3((N + 3) / 4), dim3(256), 0, s, h->nptr, h->e_src, h->e_geom, N,
                       h->flags, only, p.batch);
    ADF_HIP_CHECK(hipGetLastError());
    h->lastN = N; h->lastB = B;
    h->last_reps[0] = p.r0; h->last_reps[1] = p.r1; h->last_reps[2] = p.r2;
    return ADF_OK;
}

size_t adf_scan_temp_bytes(int64_t n) {
    size_t bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (int32_t*)nullptr, (int32_t*)nullptr, (int)n);
    return bytes;
}
