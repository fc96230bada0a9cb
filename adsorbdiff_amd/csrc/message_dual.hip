// Dual (primal, tangent) message block of the PaiNN training step, with the structure of tr_msg_fwd_kernel /
// tr_msg_bwd_kernel (train.hip): the plain path - rbfh and its gradient materialised [E, 3H], exact f32, fixed summation
// order, no atomics.  The message is trilinear in (xh[src] * rbfh, vec[src], u):
//     dx[i,c]     = sum_e xa ra
//     dvec[i,k,c] = sum_e (vec[j,k] xb rb / sqrt3 + xc rc u_k) / sqrtH;     x1 = (x + dx) / sqrt2,  vec1 = vec + dvec
// so its tangent is the sum of the one-factor-replaced terms, formed in the same pass over the segment.  Dual operands hold
// the primal block followed by the tangent block; e_tan[e] = (u_dot, d_dot) (adf_op_edge_tangent, dual_ops.hip).
#include "common.h"
#include "dual_ops.h"

// forward: one workgroup per target atom i over its CSR segment, channels strided over the threads
__global__ __launch_bounds__(256) void md_msg_fwd_kernel(const int32_t* __restrict__ nptr, const int32_t* __restrict__ e_src,
                                                          const float4* __restrict__ e_geom, const float4* __restrict__ e_tan,
                                                          const float* __restrict__ xh2, const float* __restrict__ vec2,
                                                          const float* __restrict__ rbfh2, const float* __restrict__ x2,
                                                          float* __restrict__ x1_2, float* __restrict__ vec1_2, int N,
                                                          long long E, int H, int vec_is_zero) {
    const int i = blockIdx.x;
    const int e0 = nptr[i], e1 = (int)min((long long)nptr[i + 1], E);
    const float is3 = 0.57735026918962576f, ish = 1.0f / sqrtf((float)H), is2 = 0.70710678118654752f;
    const size_t H3 = 3 * (size_t)H, tn = (size_t)N * H3, te = (size_t)E * H3, tx = (size_t)N * H;
    for (int c = threadIdx.x; c < H; c += 256) {
        float sx = 0.f, v0 = 0.f, v1 = 0.f, v2 = 0.f, sxd = 0.f, d0 = 0.f, d1 = 0.f, d2 = 0.f;
        for (int e = e0; e < e1; ++e) {
            const int j = e_src[e];
            const float4 g = e_geom[e], t = e_tan[e];
            const float* xr = xh2 + (size_t)j * H3;
            const float* rr = rbfh2 + (size_t)e * H3;
            const float xa = xr[c], xb = xr[H + c], xc = xr[2 * H + c];
            const float xad = xr[tn + c], xbd = xr[tn + H + c], xcd = xr[tn + 2 * H + c];
            const float ra = rr[c], rb = rr[H + c], rc = rr[2 * H + c];
            const float rad = rr[te + c], rbd = rr[te + H + c], rcd = rr[te + 2 * H + c];
            sx += xa * ra;
            sxd += xad * ra + xa * rad;
            const float cb = xb * rb * is3, cbd = (xbd * rb + xb * rbd) * is3;
            const float cc = xc * rc, ccd = xcd * rc + xc * rcd;
            if (!vec_is_zero) {
                const float* vr = vec2 + (size_t)j * H3;
                const float w0 = vr[c], w1 = vr[H + c], w2 = vr[2 * H + c];
                v0 += w0 * cb; v1 += w1 * cb; v2 += w2 * cb;
                d0 += vr[tn + c] * cb + w0 * cbd; d1 += vr[tn + H + c] * cb + w1 * cbd; d2 += vr[tn + 2 * H + c] * cb + w2 * cbd;
            }
            v0 += cc * g.x; v1 += cc * g.y; v2 += cc * g.z;
            d0 += ccd * g.x + cc * t.x; d1 += ccd * g.y + cc * t.y; d2 += ccd * g.z + cc * t.z;
        }
        const size_t xo = (size_t)i * H + c, vo = (size_t)i * H3 + c;
        x1_2[xo] = (x2[xo] + sx) * is2;
        x1_2[tx + xo] = (x2[tx + xo] + sxd) * is2;
        float b0 = 0.f, b1 = 0.f, b2 = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
        if (!vec_is_zero) {
            b0 = vec2[vo]; b1 = vec2[vo + H]; b2 = vec2[vo + 2 * H];
            c0 = vec2[tn + vo]; c1 = vec2[tn + vo + H]; c2 = vec2[tn + vo + 2 * H];
        }
        vec1_2[vo] = b0 + v0 * ish; vec1_2[vo + H] = b1 + v1 * ish; vec1_2[vo + 2 * H] = b2 + v2 * ish;
        vec1_2[tn + vo] = c0 + d0 * ish; vec1_2[tn + vo + H] = c1 + d1 * ish; vec1_2[tn + vo + 2 * H] = c2 + d2 * ish;
    }
}

// backward: one workgroup per SOURCE atom j over its own CSR segment.  The graph is symmetric: for each row e' = (i -> j) of
// j's segment the reverse edge (j -> i) carries the same rbfh and rbfh_dot rows (functions of d and d_dot, equal bits on the
// two rows of a pair), the negated unit vector and the negated u_dot.  The gradients of rbfh / rbfh_dot are written at row e'
// instead of the reverse edge's row: the sums over edges that make rbf_proj's weight gradient are invariant under that
// relabelling.  gx1_2, gv1_2: gradients of x1, vec1 (dual).  Writes dxh2[j], drbfh2[e'], dvec2[j] (unless vec == 0) and
// the residual path dx2[j] = gx1_2[j] / sqrt2.
__global__ __launch_bounds__(256) void md_msg_bwd_kernel(const int32_t* __restrict__ nptr, const int32_t* __restrict__ e_src,
                                                          const float4* __restrict__ e_geom, const float4* __restrict__ e_tan,
                                                          const float* __restrict__ xh2, const float* __restrict__ vec2,
                                                          const float* __restrict__ rbfh2, const float* __restrict__ gx1_2,
                                                          const float* __restrict__ gv1_2, float* __restrict__ dxh2,
                                                          float* __restrict__ drbfh2, float* __restrict__ dvec2,
                                                          float* __restrict__ dx2, int N, long long E, int H, int vec_is_zero) {
    const int j = blockIdx.x;
    const int e0 = nptr[j], e1 = (int)min((long long)nptr[j + 1], E);
    const float is3 = 0.57735026918962576f, ish = 1.0f / sqrtf((float)H), is2 = 0.70710678118654752f;
    const size_t H3 = 3 * (size_t)H, tn = (size_t)N * H3, te = (size_t)E * H3, tx = (size_t)N * H;
    for (int c = threadIdx.x; c < H; c += 256) {
        const float* xr = xh2 + (size_t)j * H3;
        const float xa = xr[c], xb = xr[H + c], xc = xr[2 * H + c];
        const float xad = xr[tn + c], xbd = xr[tn + H + c], xcd = xr[tn + 2 * H + c];
        float w0 = 0.f, w1 = 0.f, w2 = 0.f, y0 = 0.f, y1 = 0.f, y2 = 0.f;   // vec[j] and its tangent
        if (!vec_is_zero) {
            const float* vr = vec2 + (size_t)j * H3;
            w0 = vr[c]; w1 = vr[H + c]; w2 = vr[2 * H + c];
            y0 = vr[tn + c]; y1 = vr[tn + H + c]; y2 = vr[tn + 2 * H + c];
        }
        float dxa = 0.f, dxb = 0.f, dxc = 0.f, dxad = 0.f, dxbd = 0.f, dxcd = 0.f;
        float dv0 = 0.f, dv1 = 0.f, dv2 = 0.f, dy0 = 0.f, dy1 = 0.f, dy2 = 0.f;
        for (int e = e0; e < e1; ++e) {
            const int i = e_src[e];            // the neighbour: target of the reverse edge (j -> i)
            const float4 g = e_geom[e];        // unit vector j -> i; the reverse edge's is its negative
            const float4 t = e_tan[e];         // (u_dot, d_dot); the reverse edge's u_dot is its negative
            const float* rr = rbfh2 + (size_t)e * H3;
            const float ra = rr[c], rb = rr[H + c], rc = rr[2 * H + c];
            const float rad = rr[te + c], rbd = rr[te + H + c], rcd = rr[te + 2 * H + c];
            const size_t xo = (size_t)i * H + c, vo = (size_t)i * H3 + c;
            const float gx = gx1_2[xo] * is2, gxd = gx1_2[tx + xo] * is2;
            const float g0 = gv1_2[vo] * ish, g1 = gv1_2[vo + H] * ish, g2 = gv1_2[vo + 2 * H] * ish;
            const float h0 = gv1_2[tn + vo] * ish, h1 = gv1_2[tn + vo + H] * ish, h2 = gv1_2[tn + vo + 2 * H] * ish;
            // scalar path
            dxa += gx * ra + gxd * rad;
            dxad += gxd * ra;
            // vector path through vec[j] xb rb / sqrt3
            const float S = (g0 * w0 + g1 * w1 + g2 * w2) * is3;
            const float Sd1 = (h0 * y0 + h1 * y1 + h2 * y2) * is3;   // tangent outputs against vec_dot
            const float Sd2 = (h0 * w0 + h1 * w1 + h2 * w2) * is3;   // tangent outputs against vec
            dxb += (S + Sd1) * rb + Sd2 * rbd;
            dxbd += Sd2 * rb;
            const float f = xb * rb * is3, fd = (xbd * rb + xb * rbd) * is3;
            dv0 += g0 * f + h0 * fd; dv1 += g1 * f + h1 * fd; dv2 += g2 * f + h2 * fd;
            dy0 += h0 * f; dy1 += h1 * f; dy2 += h2 * f;
            // vector path through xc rc u (reverse edge: -u, -u_dot)
            const float T = -(g0 * g.x + g1 * g.y + g2 * g.z);
            const float Td1 = -(h0 * g.x + h1 * g.y + h2 * g.z);
            const float Td2 = -(h0 * t.x + h1 * t.y + h2 * t.z);
            dxc += (T + Td2) * rc + Td1 * rcd;
            dxcd += Td1 * rc;
            float* dr = drbfh2 + (size_t)e * H3;
            dr[c] = gx * xa + gxd * xad;
            dr[te + c] = gxd * xa;
            dr[H + c] = (S + Sd1) * xb + Sd2 * xbd;
            dr[te + H + c] = Sd2 * xb;
            dr[2 * H + c] = (T + Td2) * xc + Td1 * xcd;
            dr[te + 2 * H + c] = Td1 * xc;
        }
        float* dh = dxh2 + (size_t)j * H3;
        dh[c] = dxa; dh[H + c] = dxb; dh[2 * H + c] = dxc;
        dh[tn + c] = dxad; dh[tn + H + c] = dxbd; dh[tn + 2 * H + c] = dxcd;
        const size_t xo = (size_t)j * H + c;
        dx2[xo] = gx1_2[xo] * is2;
        dx2[tx + xo] = gx1_2[tx + xo] * is2;
        if (!vec_is_zero) {
            const size_t vo = (size_t)j * H3 + c;
            dvec2[vo] = gv1_2[vo] + dv0; dvec2[vo + H] = gv1_2[vo + H] + dv1; dvec2[vo + 2 * H] = gv1_2[vo + 2 * H] + dv2;
            dvec2[tn + vo] = gv1_2[tn + vo] + dy0; dvec2[tn + vo + H] = gv1_2[tn + vo + H] + dy1;
            dvec2[tn + vo + 2 * H] = gv1_2[tn + vo + 2 * H] + dy2;
        }
    }
}

// num_edges: the graph's edge count (adf_graph_build), which is also the row offset of the tangent blocks of rbfh2 / drbfh2
static bool md_graph_ok(adf_painn_t h, int64_t num_edges) {
    return h && h->lastN > 0 && num_edges >= 0 && num_edges <= (int64_t)0x7fffffff;
}
extern "C" int32_t adf_op_message_dual_fwd(adf_painn_t h, const float* e_tan, const float* xh2, const float* vec2,
                                           const float* rbfh2, const float* x2, float* x1_2, float* vec1_2,
                                           int32_t vec_is_zero, int64_t num_edges, void* stream) {
    if (!md_graph_ok(h, num_edges) || !e_tan || !xh2 || !rbfh2 || !x2 || !x1_2 || !vec1_2 || (!vec2 && !vec_is_zero)) {
        adf_set_error("message_dual_fwd: bad argument or no graph");
        return ADF_EINVAL;
    }
    hipLaunchKernelGGL(md_msg_fwd_kernel, dim3((unsigned)h->lastN), dim3(256), 0, (hipStream_t)stream, h->nptr, h->e_src,
                       h->e_geom, reinterpret_cast<const float4*>(e_tan), xh2, vec2, rbfh2, x2, x1_2, vec1_2, (int)h->lastN,
                       (long long)num_edges, h->hp.hidden_channels, vec_is_zero);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}
extern "C" int32_t adf_op_message_dual_bwd(adf_painn_t h, const float* e_tan, const float* xh2, const float* vec2,
                                           const float* rbfh2, const float* gx1_2, const float* gv1_2, float* dxh2,
                                           float* drbfh2, float* dvec2, float* dx2, int32_t vec_is_zero, int64_t num_edges,
                                           void* stream) {
    if (!md_graph_ok(h, num_edges) || !e_tan || !xh2 || !rbfh2 || !gx1_2 || !gv1_2 || !dxh2 || !drbfh2 || !dx2 ||
        ((!vec2 || !dvec2) && !vec_is_zero)) {
        adf_set_error("message_dual_bwd: bad argument or no graph");
        return ADF_EINVAL;
    }
    hipLaunchKernelGGL(md_msg_bwd_kernel, dim3((unsigned)h->lastN), dim3(256), 0, (hipStream_t)stream, h->nptr, h->e_src,
                       h->e_geom, reinterpret_cast<const float4*>(e_tan), xh2, vec2, rbfh2, gx1_2, gv1_2, dxh2, drbfh2, dvec2,
                       dx2, (int)h->lastN, (long long)num_edges, h->hp.hidden_channels, vec_is_zero);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}
