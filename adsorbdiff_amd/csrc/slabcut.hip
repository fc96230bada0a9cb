// Slab cutting: the slabs of a batch of bulk crystals along Miller indices - oriented cell, thickness,
// terminations, primitive in-plane cell, duplicate terminations, top and bottom - and the distinct Miller indices of a bulk
// under its point group.  The contract is in include/adsorbdiff_hip.h, section "Slab cutting".  It is the reference's compute_slabs
// (placement/slab.py:485-552: pymatgen's SlabGenerator, StructureMatcher and SpacegroupAnalyzer per Miller index) as a written
// contract: parity with pymatgen unpinned.
//
// One wave per (bulk, Miller index) pair in the count pass (sc_count_kernel), one wave per emitted slab in the fill pass
// (sc_fill_kernel), one wave per bulk for the point group (sc_group_kernel).  All arithmetic is double.  The lattice steps
// (extended Euclid, Lagrange-Gauss reduction, the 625 integer 2 x 2 matrices) are a few hundred flops that every lane does
// alike; what grows with the structure - the candidate rigid motions of the equivalence tests, the 3^9 integer matrices of
// the point group, the rank sort of a slab's atoms - is spread over the lanes.  A pair's working set (its atoms in the
// oriented frame, the cut planes) lies in a scratch segment that the host sized from the bulk's atom count; a slab's atoms
// are never stored before the fill pass: atom (a, m) of the slab above the plane s is atom a of the oriented cell lifted by
// whole oriented cells, a few flops from the segment.  No float atomics, no dependence on the neighbours in the batch.
//
// The wave-level helpers below have a one-lane host form, so that the whole contract can also be run as plain C++ on the
// host, under the host sanitizers: include this file and call sc_analyze / sc_emit / sc_group, which then run with one lane.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "host_util.h"

#define SC_THREADS 256
#define SC_WAVES (SC_THREADS / 64)
#define SC_MAX_OPS 48            // the largest crystallographic point group
#define SC_MAX_W 12              // a two-dimensional lattice has at most 12 point operations
#define SC_RD 80                 // doubles of a pair's record
#define SC_RI 32                 // ints of a pair's record
#define SC_FTOL 1e-6             // fractional in-plane coordinates closer than this count as equal (wrap and order)
#define SC_TIE 1e-9              // squared lengths closer than this times the cell's longest squared edge tie
#define SC_MAX_SLAB_ATOMS (1 << 20)
#define SC_GROUP_WORDS (SC_MAX_OPS * 9)

// error bits of a pair / a bulk
#define SC_E_ZERO 1              // h = (0,0,0)
#define SC_E_CELL 2              // singular, left-handed or non-finite cell
#define SC_E_EMPTY 4             // a bulk without atoms
#define SC_E_SIZE 8              // the slab would hold more than SC_MAX_SLAB_ATOMS atoms
#define SC_E_TRANS 16            // the in-plane translations found do not form a group at this symprec

#define SC_HD __host__ __device__ inline

#ifdef __HIP_DEVICE_COMPILE__
#define SC_NL 64
#define SC_LANE() ((int)(threadIdx.x & 63))
#define SC_SYNC() __threadfence()
SC_HD bool sc_any(bool x) { return __ballot(x) != 0ull; }
// the slot of a flagged lane among the flagged lanes of this round, counted from base; base moves past the round
SC_HD int sc_slot(bool flag, int& base) {
    const unsigned long long m = __ballot(flag);
    const int at = base + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
    base += __popcll(m);
    return flag ? at : -1;
}
#else
#define SC_NL 1
#define SC_LANE() 0
#define SC_SYNC() ((void)0)
SC_HD bool sc_any(bool x) { return x; }
SC_HD int sc_slot(bool flag, int& base) {
    const int at = base;
    base += flag ? 1 : 0;
    return flag ? at : -1;
}
#endif

// ---- small integer and vector helpers
SC_HD long long sc_abs(long long a) { return a < 0 ? -a : a; }
SC_HD long long sc_gcd(long long a, long long b) {
    a = sc_abs(a); b = sc_abs(b);
    while (b) { const long long t = a % b; a = b; b = t; }
    return a;
}
// g = gcd(a, b) >= 0 and a x + b y = g (x = y = 0 for a = b = 0)
SC_HD long long sc_egcd(long long a, long long b, long long& x, long long& y) {
    long long r0 = sc_abs(a), r1 = sc_abs(b), x0 = 1, x1 = 0, y0 = 0, y1 = 1;
    while (r1) {
        const long long q = r0 / r1;
        long long t = r0 - q * r1; r0 = r1; r1 = t;
        t = x0 - q * x1; x0 = x1; x1 = t;
        t = y0 - q * y1; y0 = y1; y1 = t;
    }
    if (r0 == 0) { x = y = 0; return 0; }
    x = a < 0 ? -x0 : x0;
    y = b < 0 ? -y0 : y0;
    return r0;
}
SC_HD bool sc_lex_greater(const int* a, const int* b) {
    return a[0] != b[0] ? a[0] > b[0] : a[1] != b[1] ? a[1] > b[1] : a[2] > b[2];
}
// the Cartesian vector of integer lattice coordinates v: v . A, rows of A the lattice vectors
SC_HD void sc_cart(const int* v, const double* A, double* c) {
    for (int k = 0; k < 3; ++k) c[k] = (double)v[0] * A[k] + (double)v[1] * A[3 + k] + (double)v[2] * A[6 + k];
}
SC_HD double sc_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
SC_HD void sc_cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// ---- a pair's record.  rd: doubles, ri: ints; the per-atom arrays hold nb entries each.
// rd[0..9): the frame, rows x, y, z (unit vectors in the bulk's Cartesian axes); rd[9]: d; rd[10..12): p1, rd[12..14): p2,
// rd[14..16): the in-plane part of u3, all in the frame; rd[16..16 + 4 nW): the point operations as Cartesian 2 x 2 matrices
#define SC_D 9
#define SC_P1 10
#define SC_P2 12
#define SC_U3 14
#define SC_RW 16
// ri[0]: error bits, [1]: atoms of the primitive oriented cell, [2]: n_slab, [3]: n_vac, [4]: cuts, [5]: kept cuts,
// [6]: slabs emitted, [7]: point operations, [8]: anchor atom, [9..12): the reduced Miller index, [12..21): u1, u2, u3
#define SC_ERR 0
#define SC_NP 1
#define SC_NSLAB 2
#define SC_NVAC 3
#define SC_NCUT 4
#define SC_NKEPT 5
#define SC_NOUT 6
#define SC_NW 7
#define SC_ANCHOR 8
#define SC_H 9
#define SC_U 12

struct sc_seg {
    double *X, *Y, *H, *hs, *cut;   // in-plane coordinates and height in [0, d) of the oriented cell's atoms; sorted heights; cut planes
    int32_t *Z, *flag, *aux;        // species; per cut: bit 0 kept, bit 1 invertible; scratch flags
    double* rd;
    int32_t* ri;
};

struct sc_params {
    double min_slab, min_vac, tol, symprec;
};

// the least (count, Z, index) atom among n: the first atom of the rarest species
SC_HD int sc_anchor(const int32_t* Z, int n) {
    int bc = INT_MAX, bz = INT_MAX, bi = 0;
    for (int i = 0; i < n; ++i) {
        const int zi = Z[i];
        int cnt = 0;
        for (int k = 0; k < n; ++k) cnt += Z[k] == zi ? 1 : 0;
        if (cnt < bc || (cnt == bc && zi < bz)) { bc = cnt; bz = zi; bi = i; }
    }
    return bi;
}

// the geometry of a pair as the matchers and the emitter read it
struct sc_geo {
    double d, p1x, p2x, p2y, u3x, u3y, symprec;
    int np, nslab;
};
SC_HD sc_geo sc_load_geo(const sc_seg& s, double symprec) {
    sc_geo g;
    g.d = s.rd[SC_D]; g.p1x = s.rd[SC_P1]; g.p2x = s.rd[SC_P2]; g.p2y = s.rd[SC_P2 + 1];
    g.u3x = s.rd[SC_U3]; g.u3y = s.rd[SC_U3 + 1]; g.symprec = symprec;
    g.np = s.ri[SC_NP]; g.nslab = s.ri[SC_NSLAB];
    return g;
}
// atom i = (a, m) of the slab above the plane `cut`: in-plane coordinates and height above the plane
SC_HD void sc_slab_atom(const sc_seg& s, const sc_geo& g, double cut, int i, double& x, double& y, double& z, int& Z) {
    const int a = i % g.np, m = i / g.np;
    const double h = s.H[a];
    const int j = m + (h < cut ? 1 : 0);
    x = s.X[a] + (double)j * g.u3x;
    y = s.Y[a] + (double)j * g.u3y;
    z = h + (double)j * g.d - cut;
    Z = s.Z[a];
}
// lowest and highest atom of that slab
SC_HD void sc_slab_range(const sc_seg& s, const sc_geo& g, double cut, double& zmin, double& zmax) {
    zmin = INFINITY; zmax = -INFINITY;
    for (int a = 0; a < g.np; ++a) {
        const double h = s.H[a], z = h + (h < cut ? g.d : 0.0) - cut;
        zmin = fmin(zmin, z);
        zmax = fmax(zmax, z + (double)(g.nslab - 1) * g.d);
    }
}

// Does (x, y, z) -> (R (x, y) + tau, zc2 +- (z - zc1)) take every atom of the slab above cut1 onto an atom of its species of
// the slab above cut2, within symprec, modulo the in-plane lattice (p1, p2)?  One lane, serial.
SC_HD bool sc_match(const sc_seg& s, const sc_geo& g, double cut1, double cut2, double zc1, double zc2, bool mirror,
                    const double* R, double taux, double tauy) {
    const int N = g.np * g.nslab;
    const double s2 = g.symprec * g.symprec, idet = 1.0 / (g.p1x * g.p2y);
    for (int i = 0; i < N; ++i) {
        double x, y, z;
        int Zi;
        sc_slab_atom(s, g, cut1, i, x, y, z, Zi);
        const double tx = R[0] * x + R[1] * y + taux, ty = R[2] * x + R[3] * y + tauy;
        const double tz = mirror ? zc2 - (z - zc1) : zc2 + (z - zc1);
        bool found = false;
        for (int a = 0; a < g.np && !found; ++a) {
            if (s.Z[a] != Zi) continue;
            // the one lift of atom a that can lie at this height
            const double h = s.H[a];
            const double j = rint((tz + cut2 - h) / g.d);
            const double m = j - (h < cut2 ? 1.0 : 0.0);
            if (m < 0.0 || m > (double)(g.nslab - 1)) continue;
            const double dz = tz - (h + j * g.d - cut2);
            if (!(fabs(dz) <= g.symprec)) continue;
            const double dx = tx - (s.X[a] + j * g.u3x), dy = ty - (s.Y[a] + j * g.u3y);
            double f2 = dy * g.p1x * idet, f1 = (dx * g.p2y - dy * g.p2x) * idet;   // (dx, dy) = f1 p1 + f2 p2, p1 = (p1x, 0)
            f1 -= rint(f1);
            f2 -= rint(f2);
            const double ex = f1 * g.p1x + f2 * g.p2x, ey = f2 * g.p2y;
            found = ex * ex + ey * ey + dz * dz <= s2;
        }
        if (!found) return false;
    }
    return true;
}

// Are the slabs above cuts c1 and c2 the same up to an in-plane rigid motion (mirror: after mirroring the first through its
// mid-plane)?  Candidates are (point operation w, atom q of the second slab that the first slab's anchor may land on);
// the lanes share them, and every lane returns the same answer.
SC_HD bool sc_equivalent(const sc_seg& s, const sc_geo& g, int c1, int c2, bool mirror) {
    const int lane = SC_LANE();
    const double cut1 = s.cut[c1], cut2 = s.cut[c2];
    double lo1, hi1, lo2, hi2;
    sc_slab_range(s, g, cut1, lo1, hi1);
    sc_slab_range(s, g, cut2, lo2, hi2);
    if (!(fabs((hi1 - lo1) - (hi2 - lo2)) <= 2.0 * g.symprec)) return false;
    const double zc1 = 0.5 * (lo1 + hi1), zc2 = 0.5 * (lo2 + hi2);
    const int N = g.np * g.nslab, nW = s.ri[SC_NW], anchor = s.ri[SC_ANCHOR];
    double ax, ay, az;
    int aZ;
    sc_slab_atom(s, g, cut1, anchor, ax, ay, az, aZ);                   // (anchor, m = 0)
    const double tz = mirror ? zc2 - (az - zc1) : zc2 + (az - zc1);
    const long long total = (long long)nW * N;
    for (long long c0 = 0; c0 < total; c0 += SC_NL) {
        const long long c = c0 + lane;
        bool ok = c < total;
        if (ok) {
            const int w = (int)(c / N), q = (int)(c % N);
            double x, y, z;
            int Zq;
            sc_slab_atom(s, g, cut2, q, x, y, z, Zq);
            ok = Zq == aZ && fabs(z - tz) <= g.symprec;
            if (ok) {
                const double* R = s.rd + SC_RW + 4 * w;
                ok = sc_match(s, g, cut1, cut2, zc1, zc2, mirror, R, x - (R[0] * ax + R[1] * ay), y - (R[2] * ax + R[3] * ay));
            }
        }
        if (sc_any(ok)) return true;
    }
    return false;
}

// Does the in-plane translation (tx, ty) map the oriented cell's atoms onto themselves, modulo (u1, u2, u3)?  One lane.
SC_HD bool sc_cell_translation(const sc_seg& s, int nb, double d, double u1x, double u2x, double u2y, double u3x, double u3y,
                               double symprec, double tx, double ty) {
    const double s2 = symprec * symprec, idet = 1.0 / (u1x * u2y);
    for (int i = 0; i < nb; ++i) {
        bool found = false;
        for (int k = 0; k < nb && !found; ++k) {
            if (s.Z[k] != s.Z[i]) continue;
            double dz = s.H[i] - s.H[k];
            const double j = rint(dz / d);
            dz -= j * d;
            if (!(fabs(dz) <= symprec)) continue;
            const double dx = s.X[i] + tx - s.X[k] - j * u3x, dy = s.Y[i] + ty - s.Y[k] - j * u3y;
            double f2 = dy * u1x * idet, f1 = (dx * u2y - dy * u2x) * idet;
            f1 -= rint(f1);
            f2 -= rint(f2);
            const double ex = f1 * u1x + f2 * u2x, ey = f2 * u2y;
            found = ex * ex + ey * ey + dz * dz <= s2;
        }
        if (!found) return false;
    }
    return true;
}

// The second basis vector for a given first one p = (px, py) and any v that completes it to a right-handed basis: the member
// of v + k p, k integer, with p . v <= SC_TIE |p|^2 and the largest such k - the shortest obtuse partner.
SC_HD double sc_obtuse_shift(double pp, double pv) { return floor(SC_TIE - pv / pp); }

// ---- the count pass of one pair: steps 1 - 6 of the contract.  Fills the pair's record and scratch segment.
SC_HD void sc_analyze(const double* pos, const double* cell, const int32_t* Zin, int a0, int nb, const int32_t* hkl,
                      const sc_params& P, const sc_seg& s) {
    const int lane = SC_LANE();
    int err = 0;
    long long h[3] = {hkl[0], hkl[1], hkl[2]};
    const long long g = sc_gcd(sc_gcd(h[0], h[1]), h[2]);
    double A[9];
    for (int k = 0; k < 9; ++k) A[k] = cell[k];
    double bc[3];
    sc_cross(A + 3, A + 6, bc);
    const double V = sc_dot(A, bc);
    const double la2 = sc_dot(A, A), lb2 = sc_dot(A + 3, A + 3), lc2 = sc_dot(A + 6, A + 6);
    const double L2 = fmax(la2, fmax(lb2, lc2));
    if (g == 0) err |= SC_E_ZERO;
    if (!(V > 1e-9 * sqrt(la2 * lb2 * lc2)) || !(L2 < 1e30)) err |= SC_E_CELL;
    if (nb <= 0) err |= SC_E_EMPTY;
    if (err) {
        if (lane == 0) {
            for (int k = 0; k < SC_RI; ++k) s.ri[k] = 0;
            s.ri[SC_ERR] = err;
        }
        return;
    }
    for (int k = 0; k < 3; ++k) h[k] /= g;
    const int hi[3] = {(int)h[0], (int)h[1], (int)h[2]};

    // -- step 1: a basis (b1, b2) of {u : h . u = 0} with b1 x b2 = h, and w with h . w = 1, by extended Euclid
    int b1[3], b2[3], w[3];
    {
        long long x, y, p, q;
        const long long g1 = sc_egcd(h[0], h[1], x, y);
        if (g1 == 0) {                                                   // h = (0, 0, +-1)
            b1[0] = 1; b1[1] = 0; b1[2] = 0;
            b2[0] = 0; b2[1] = (int)h[2]; b2[2] = 0;
            w[0] = 0; w[1] = 0; w[2] = (int)h[2];
        } else {
            (void)sc_egcd(g1, h[2], p, q);                               // g1 p + l q = 1
            b1[0] = (int)(h[1] / g1); b1[1] = (int)(-h[0] / g1); b1[2] = 0;
            b2[0] = (int)(x * h[2]); b2[1] = (int)(y * h[2]); b2[2] = (int)(-g1);
            w[0] = (int)(x * p); w[1] = (int)(y * p); w[2] = (int)q;
        }
    }
    // Lagrange-Gauss: (a, b) the two shortest independent vectors of the plane lattice
    int a[3] = {b1[0], b1[1], b1[2]}, b[3] = {b2[0], b2[1], b2[2]};
    double ac[3], bcv[3];
    for (int it = 0; it < 200; ++it) {
        sc_cart(a, A, ac);
        sc_cart(b, A, bcv);
        const double aa = sc_dot(ac, ac), bb = sc_dot(bcv, bcv);
        if (aa > bb) {
            for (int k = 0; k < 3; ++k) { const int t = a[k]; a[k] = b[k]; b[k] = t; }
            continue;
        }
        const double q = rint(sc_dot(ac, bcv) / aa);
        if (q == 0.0 || !(fabs(q) < 1e9)) break;
        for (int k = 0; k < 3; ++k) b[k] -= (int)q * a[k];
    }
    sc_cart(a, A, ac);
    sc_cart(b, A, bcv);
    // u1: the shortest vector; among ties the lexicographically greatest integer triple
    int u1[3] = {0, 0, 0}, al = 0, be = 0;
    {
        const double aa = sc_dot(ac, ac);
        bool have = false;
        for (int code = 0; code < 9; ++code) {
            const int ca = code / 3 - 1, cb = code % 3 - 1;
            if (ca == 0 && cb == 0) continue;
            const int v[3] = {ca * a[0] + cb * b[0], ca * a[1] + cb * b[1], ca * a[2] + cb * b[2]};
            double vc[3];
            sc_cart(v, A, vc);
            if (!(sc_dot(vc, vc) <= aa + SC_TIE * L2)) continue;
            if (!have || sc_lex_greater(v, u1)) { u1[0] = v[0]; u1[1] = v[1]; u1[2] = v[2]; al = ca; be = cb; have = true; }
        }
    }
    // v0 completes u1 to a basis with u1 x v0 = h; u2 = v0 + k u1, the shortest obtuse partner
    int u2[3];
    double u1c[3], u2c[3];
    {
        const int ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const int sg = ab[0] * hi[0] + ab[1] * hi[1] + ab[2] * hi[2] > 0 ? 1 : -1;
        // u1 = al a + be b; v0 = ga a + de b with al de - be ga = sg; when both are non-zero, al != 0 decides
        const int ga = al != 0 ? 0 : -sg * be, de = al != 0 ? sg * al : 0;
        int v0[3];
        for (int k = 0; k < 3; ++k) v0[k] = ga * a[k] + de * b[k];
        double v0c[3];
        sc_cart(u1, A, u1c);
        sc_cart(v0, A, v0c);
        const double kk = sc_obtuse_shift(sc_dot(u1c, u1c), sc_dot(u1c, v0c));
        for (int k = 0; k < 3; ++k) u2[k] = v0[k] + (int)kk * u1[k];
        sc_cart(u2, A, u2c);
    }
    // the frame: x along u1, z along the normal
    double ex[3], ey[3], ez[3];
    sc_cross(u1c, u2c, ez);
    const double area = sqrt(sc_dot(ez, ez)), l1 = sqrt(sc_dot(u1c, u1c));
    for (int k = 0; k < 3; ++k) { ez[k] /= area; ex[k] = u1c[k] / l1; }
    sc_cross(ez, ex, ey);
    const double u1x = l1, u2x = sc_dot(u2c, ex), u2y = sc_dot(u2c, ey);
    // u3 = w - i u1 - j u2 with the shortest in-plane part; ties to the lexicographically greatest triple
    int u3[3] = {0, 0, 0};
    double d, u3x = 0.0, u3y = 0.0;
    {
        double wc[3];
        sc_cart(w, A, wc);
        d = sc_dot(wc, ez);
        const double wx = sc_dot(wc, ex), wy = sc_dot(wc, ey);
        const double f2 = wy / u2y, f1 = (wx - f2 * u2x) / u1x;
        const int i0 = (int)rint(f1), j0 = (int)rint(f2);
        double best = INFINITY;
        for (int di = -2; di <= 2; ++di)
            for (int dj = -2; dj <= 2; ++dj) {
                const int i = i0 + di, j = j0 + dj;
                const int v[3] = {w[0] - i * u1[0] - j * u2[0], w[1] - i * u1[1] - j * u2[1], w[2] - i * u1[2] - j * u2[2]};
                const double vx = wx - i * u1x - j * u2x, vy = wy - j * u2y, len = vx * vx + vy * vy;
                const bool better = len < best - SC_TIE * L2, tie = !better && len <= best + SC_TIE * L2;
                if (better || (tie && sc_lex_greater(v, u3))) {
                    if (better || len < best) best = len;
                    u3[0] = v[0]; u3[1] = v[1]; u3[2] = v[2];
                    u3x = vx; u3y = vy;
                }
            }
    }
    // -- step 2: thickness
    const double ns = ceil(P.min_slab / d), nv = ceil(P.min_vac / d);
    if (!(ns * (double)nb <= (double)SC_MAX_SLAB_ATOMS) || !(nv <= (double)SC_MAX_SLAB_ATOMS) || !(d > 0.0)) {
        if (lane == 0) {
            for (int k = 0; k < SC_RI; ++k) s.ri[k] = 0;
            s.ri[SC_ERR] = SC_E_SIZE;
        }
        return;
    }
    const int nslab = (int)fmax(ns, 1.0), nvac = (int)fmax(nv, 1.0);
    // the atoms in the frame, lifted by whole u3 into heights [0, d)
    for (int i = lane; i < nb; i += SC_NL) {
        const double* r = pos + 3 * (size_t)(a0 + i);
        double x = sc_dot(r, ex), y = sc_dot(r, ey), z = sc_dot(r, ez);
        const double j = floor(z / d);
        x -= j * u3x; y -= j * u3y; z -= j * d;
        if (z >= d) { x -= u3x; y -= u3y; z -= d; }
        if (z < 0.0) z = 0.0;
        s.X[i] = x; s.Y[i] = y; s.H[i] = z; s.Z[i] = Zin[a0 + i];
    }
    SC_SYNC();
    // -- step 3: sorted heights (a rank sort: every lane places its atoms), then the cut planes in ascending shift
    for (int i = lane; i < nb; i += SC_NL) {
        const double z = s.H[i];
        int rank = 0;
        for (int k = 0; k < nb; ++k) rank += (s.H[k] < z || (s.H[k] == z && k < i)) ? 1 : 0;
        s.hs[rank] = z;
    }
    SC_SYNC();
    int ncut = 0;
    {
        const double last_gap = s.hs[0] + d - s.hs[nb - 1], last_mid = s.hs[nb - 1] + 0.5 * last_gap;
        const bool last = last_gap > P.tol;
        const bool around = last_mid >= d - 1e-9;                         // a plane within 1e-9 A of d is the plane at 0
        if (last && around) { if (lane == 0) s.cut[ncut] = fmax(last_mid - d, 0.0); ++ncut; }
        for (int i = 0; i + 1 < nb; ++i) {
            const double gap = s.hs[i + 1] - s.hs[i];
            if (gap > P.tol) { if (lane == 0) s.cut[ncut] = s.hs[i] + 0.5 * gap; ++ncut; }
        }
        if (last && !around) { if (lane == 0) s.cut[ncut] = last_mid; ++ncut; }
        if (ncut == 0) {                                                 // no gap beyond tol: the largest, ties to the lowest height
            double best = -1.0, mid = 0.0;
            for (int i = 0; i < nb; ++i) {
                const double gap = (i + 1 < nb ? s.hs[i + 1] : s.hs[0] + d) - s.hs[i];
                if (gap > best + 1e-9) { best = gap; mid = s.hs[i] + 0.5 * gap; }
            }
            if (mid >= d - 1e-9) mid = fmax(mid - d, 0.0);
            if (lane == 0) s.cut[0] = mid;
            ncut = 1;
        }
    }
    // -- step 4: the in-plane translations of the oriented cell; the lanes share the candidate atoms
    const int anchor0 = sc_anchor(s.Z, nb);
    int ntr = 0;
    for (int j0 = 0; j0 < nb; j0 += SC_NL) {
        const int j = j0 + lane;
        bool ok = j < nb && j != anchor0 && s.Z[j] == s.Z[anchor0];
        if (ok) {
            double dz = s.H[j] - s.H[anchor0];
            const double m = rint(dz / d);
            dz -= m * d;
            ok = fabs(dz) <= P.symprec &&
                 sc_cell_translation(s, nb, d, u1x, u2x, u2y, u3x, u3y, P.symprec, s.X[j] - s.X[anchor0] - m * u3x,
                                     s.Y[j] - s.Y[anchor0] - m * u3y);
        }
        if (j < nb) s.aux[j] = ok ? 1 : 0;
        int base = ntr;
        (void)sc_slot(ok, base);
        ntr = base;
    }
    SC_SYNC();
    double p1x = u1x, p1y = 0.0, p2x = u2x, p2y = u2y;
    if (ntr > 0) {
        // the shortest vector of the finer lattice: ties to the greatest x, then the greatest y, in the frame of u1
        const double tl = SC_TIE * L2, tx = 1e-9 * sqrt(L2), idet = 1.0 / (u1x * u2y);
        double best = INFINITY;
        for (int j = -1; j < nb; ++j) {
            if (j >= 0 && !s.aux[j]) continue;
            double dx = 0.0, dy = 0.0;
            if (j >= 0) {
                const double m = rint((s.H[j] - s.H[anchor0]) / d);
                dx = s.X[j] - s.X[anchor0] - m * u3x;
                dy = s.Y[j] - s.Y[anchor0] - m * u3y;
            }
            double f2 = dy * u1x * idet, f1 = (dx * u2y - dy * u2x) * idet;
            f1 -= rint(f1);
            f2 -= rint(f2);
            for (int di = -2; di <= 2; ++di)
                for (int dj = -2; dj <= 2; ++dj) {
                    if (j < 0 && di == 0 && dj == 0) continue;
                    const double vx = (f1 + di) * u1x + (f2 + dj) * u2x, vy = (f2 + dj) * u2y, len = vx * vx + vy * vy;
                    const bool better = len < best - tl, tie = !better && len <= best + tl;
                    if (better || (tie && (vx > p1x + tx || (fabs(vx - p1x) <= tx && vy > p1y + tx)))) {
                        if (better || len < best) best = len;
                        p1x = vx; p1y = vy;
                    }
                }
        }
        // its partner: any lattice vector at the primitive area to its left, then the shortest obtuse one
        const double want = u1x * u2y / (double)(ntr + 1);
        double bestdev = INFINITY, vx0 = 0.0, vy0 = 0.0;
        for (int j = -1; j < nb; ++j) {
            if (j >= 0 && !s.aux[j]) continue;
            double dx = 0.0, dy = 0.0;
            if (j >= 0) {
                const double m = rint((s.H[j] - s.H[anchor0]) / d);
                dx = s.X[j] - s.X[anchor0] - m * u3x;
                dy = s.Y[j] - s.Y[anchor0] - m * u3y;
            }
            double f2 = dy * u1x * idet, f1 = (dx * u2y - dy * u2x) * idet;
            f1 -= rint(f1);
            f2 -= rint(f2);
            for (int di = -2; di <= 2; ++di)
                for (int dj = -2; dj <= 2; ++dj) {
                    const double vx = (f1 + di) * u1x + (f2 + dj) * u2x, vy = (f2 + dj) * u2y;
                    const double dev = fabs(p1x * vy - p1y * vx - want);
                    if (dev < bestdev - 1e-9 * want) { bestdev = dev; vx0 = vx; vy0 = vy; }
                }
        }
        const double pp = p1x * p1x + p1y * p1y, kk = sc_obtuse_shift(pp, p1x * vx0 + p1y * vy0);
        p2x = vx0 + kk * p1x;
        p2y = vy0 + kk * p1y;
        if (!(bestdev <= 1e-6 * want) || nb % (ntr + 1) != 0) err |= SC_E_TRANS;
    }
    // one atom per translation class: the lowest index
    {
        const double det = p1x * p2y - p1y * p2x, s2 = P.symprec * P.symprec;
        for (int i = lane; i < nb; i += SC_NL) {
            bool keep = true;
            for (int k = 0; k < i && keep && ntr > 0; ++k) {
                if (s.Z[k] != s.Z[i]) continue;
                double dz = s.H[i] - s.H[k];
                const double m = rint(dz / d);
                dz -= m * d;
                if (!(fabs(dz) <= P.symprec)) continue;
                const double dx = s.X[i] - s.X[k] - m * u3x, dy = s.Y[i] - s.Y[k] - m * u3y;
                double f1 = (dx * p2y - dy * p2x) / det, f2 = (p1x * dy - p1y * dx) / det;
                f1 -= rint(f1);
                f2 -= rint(f2);
                const double qx = f1 * p1x + f2 * p2x, qy = f1 * p1y + f2 * p2y;
                keep = !(qx * qx + qy * qy + dz * dz <= s2);
            }
            s.flag[i] = keep ? 1 : 0;                                  // (flag: free until the cuts are judged)
        }
    }
    SC_SYNC();
    // compaction and the turn of the frame onto p1, one lane; every lane counts
    const double pl = sqrt(p1x * p1x + p1y * p1y), co = p1x / pl, si = p1y / pl;
    int np = 0;
    for (int i = 0; i < nb; ++i) np += s.flag[i] ? 1 : 0;
    if (np * (ntr + 1) != nb) err |= SC_E_TRANS;
    SC_SYNC();
    if (lane == 0) {
        int at = 0;
        for (int i = 0; i < nb; ++i) {
            if (!s.flag[i]) continue;
            const double x = s.X[i], y = s.Y[i];
            s.X[at] = co * x + si * y; s.Y[at] = -si * x + co * y; s.H[at] = s.H[i]; s.Z[at] = s.Z[i];
            ++at;
        }
    }
    SC_SYNC();
    const double q2x = co * p2x + si * p2y, q2y = -si * p2x + co * p2y;
    const double v3x = co * u3x + si * u3y, v3y = -si * u3x + co * u3y;
    // the point operations of the lattice (p1, p2): integer W with |entries| <= 2 that keep the three lengths
    int nW = 0;
    {
        const double l0 = pl, l1b = sqrt(q2x * q2x + q2y * q2y), l2 = sqrt((pl + q2x) * (pl + q2x) + q2y * q2y);
        for (int code = 0; code < 625 && nW < SC_MAX_W; ++code) {
            const int w00 = code / 125 - 2, w01 = (code / 25) % 5 - 2, w10 = (code / 5) % 5 - 2, w11 = code % 5 - 2;
            const int det = w00 * w11 - w01 * w10;
            if (det != 1 && det != -1) continue;
            // images of p1 and p2: the columns of [p1 p2] W
            const double c0x = pl * w00 + q2x * w10, c0y = q2y * w10, c1x = pl * w01 + q2x * w11, c1y = q2y * w11;
            const double m0 = sqrt(c0x * c0x + c0y * c0y), m1 = sqrt(c1x * c1x + c1y * c1y);
            const double m2 = sqrt((c0x + c1x) * (c0x + c1x) + (c0y + c1y) * (c0y + c1y));
            if (!(fmax(fmax(fabs(m0 - l0), fabs(m1 - l1b)), fabs(m2 - l2)) <= P.symprec)) continue;
            // R = [c0 c1] [p1 p2]^-1
            if (lane == 0) {
                const double id = 1.0 / (pl * q2y);
                double* R = s.rd + SC_RW + 4 * nW;
                R[0] = c0x * q2y * id; R[1] = (c1x * pl - c0x * q2x) * id;
                R[2] = c0y * q2y * id; R[3] = (c1y * pl - c0y * q2x) * id;
            }
            ++nW;
        }
    }
    if (lane == 0) {
        // the frame's rows, turned
        for (int k = 0; k < 3; ++k) { s.rd[k] = co * ex[k] + si * ey[k]; s.rd[3 + k] = -si * ex[k] + co * ey[k]; s.rd[6 + k] = ez[k]; }
        s.rd[SC_D] = d;
        s.rd[SC_P1] = pl; s.rd[SC_P1 + 1] = 0.0;
        s.rd[SC_P2] = q2x; s.rd[SC_P2 + 1] = q2y;
        s.rd[SC_U3] = v3x; s.rd[SC_U3 + 1] = v3y;
        for (int k = 0; k < SC_RI; ++k) s.ri[k] = 0;
        s.ri[SC_NP] = np; s.ri[SC_NSLAB] = nslab; s.ri[SC_NVAC] = nvac; s.ri[SC_NCUT] = ncut; s.ri[SC_NW] = nW;
        for (int k = 0; k < 3; ++k) { s.ri[SC_H + k] = hi[k]; s.ri[SC_U + k] = u1[k]; s.ri[SC_U + 3 + k] = u2[k]; s.ri[SC_U + 6 + k] = u3[k]; }
    }
    SC_SYNC();
    if (err == 0 && np > 0) {
        if (lane == 0) s.ri[SC_ANCHOR] = sc_anchor(s.Z, np);
        SC_SYNC();
    }
    int nkept = 0, nout = 0;
    if (err == 0) {
        // -- step 5: a cut is dropped when an earlier kept one is the same slab; step 6: is a kept one its own mirror image?
        const sc_geo G = sc_load_geo(s, P.symprec);
        for (int c = 0; c < ncut; ++c) {
            bool kept = true;
            for (int e = 0; e < c && kept; ++e)
                if ((s.flag[e] & 1) && sc_equivalent(s, G, e, c, false)) kept = false;
            int f = 0;
            if (kept) {
                f = 1 | (sc_equivalent(s, G, c, c, true) ? 2 : 0);
                ++nkept;
                nout += (f & 2) ? 1 : 2;
            }
            SC_SYNC();
            if (lane == 0) s.flag[c] = f;
            SC_SYNC();
        }
    }
    if (lane == 0) {
        s.ri[SC_ERR] = err;
        s.ri[SC_NKEPT] = nkept;
        s.ri[SC_NOUT] = nout;
    }
}

// where one emitted slab goes
struct sc_out {
    double* pos64;
    float* pos32;
    int32_t* Z;
    double* cell;        // 9
    int32_t* millers;    // 3
    double* shift;
    int32_t *top, *bulk_index, *natoms;
};

// ---- the fill pass of slab q of a pair: step 7.  The slab's N atoms go to out.pos64 / pos32 / Z in the contract's order.
SC_HD void sc_emit(const sc_seg& s, double symprec, int q, int bulk, const sc_out& out) {
    const int lane = SC_LANE();
    const sc_geo G = sc_load_geo(s, symprec);
    const int nkept = s.ri[SC_NKEPT], ncut = s.ri[SC_NCUT], N = G.np * G.nslab;
    const bool flipped = q >= nkept;
    int c = -1, seen = 0;
    for (int e = 0; e < ncut && c < 0; ++e) {
        const int f = s.flag[e];
        if (!(f & 1) || (flipped && (f & 2))) continue;
        if (seen == (flipped ? q - nkept : q)) c = e;
        ++seen;
    }
    if (c < 0) return;
    const double cut = s.cut[c], height = (double)(G.nslab + s.ri[SC_NVAC]) * G.d;
    double lo, hi;
    sc_slab_range(s, G, cut, lo, hi);
    const double zc = 0.5 * (lo + hi);
    // the cell: a flipped slab's second vector is negated after the turn and, where that leaves an acute pair, lowered by the first
    const double c0x = G.p1x;
    double c1x = flipped ? -G.p2x : G.p2x;
    const double c1y = G.p2y;
    if (flipped) c1x += sc_obtuse_shift(c0x * c0x, c0x * c1x) * c0x;
    struct key { double z, f1, f2; };
    auto key_of = [&](int i, int& Z) {
        double x, y, z;
        sc_slab_atom(s, G, cut, i, x, y, z, Z);
        z = z - zc + 0.5 * height;
        if (flipped) { y = -y; z = height - z; }
        key k;
        k.z = z;
        k.f2 = y / c1y;
        k.f1 = (x - k.f2 * c1x) / c0x;
        k.f1 -= floor(k.f1 + SC_FTOL);
        k.f2 -= floor(k.f2 + SC_FTOL);
        return k;
    };
    for (int i = lane; i < N; i += SC_NL) {
        int Zi, Zk;
        const key a = key_of(i, Zi);
        int rank = 0;
        for (int k = 0; k < N; ++k) {
            if (k == i) continue;
            const key b = key_of(k, Zk);
            bool before;
            if (b.z < a.z - symprec) before = true;
            else if (b.z > a.z + symprec) before = false;
            else if (b.f1 < a.f1 - SC_FTOL) before = true;
            else if (b.f1 > a.f1 + SC_FTOL) before = false;
            else if (b.f2 < a.f2 - SC_FTOL) before = true;
            else if (b.f2 > a.f2 + SC_FTOL) before = false;
            else before = k < i;
            rank += before ? 1 : 0;
        }
        if (rank >= N) rank = N - 1;
        const double px = a.f1 * c0x + a.f2 * c1x, py = a.f2 * c1y, pz = a.z;
        out.pos64[3 * (size_t)rank] = px; out.pos64[3 * (size_t)rank + 1] = py; out.pos64[3 * (size_t)rank + 2] = pz;
        out.pos32[3 * (size_t)rank] = (float)px; out.pos32[3 * (size_t)rank + 1] = (float)py; out.pos32[3 * (size_t)rank + 2] = (float)pz;
        out.Z[rank] = Zi;
    }
    if (lane == 0) {
        for (int k = 0; k < 9; ++k) out.cell[k] = 0.0;
        out.cell[0] = c0x; out.cell[3] = c1x; out.cell[4] = c1y; out.cell[8] = height;
        for (int k = 0; k < 3; ++k) out.millers[k] = s.ri[SC_H + k];
        *out.shift = cut;
        *out.top = flipped ? 0 : 1;
        *out.bulk_index = bulk;
        *out.natoms = N;
    }
}

// ---- the point group of one bulk: integer W with entries in {-1, 0, 1} and rows a'_i = sum_j W_ij a_j of the old lengths
// (the three edges and the three face diagonals, within symprec), then the atoms: f -> f W + t for some t.
// ops: SC_GROUP_WORDS ints, nine per operation, ascending code; frac: 3 n doubles.  Returns the order, or -1 - an error bit.
SC_HD int sc_group(const double* pos, const double* cell, const int32_t* Z, int a0, int n, double symprec, int32_t* ops,
                   double* frac) {
    const int lane = SC_LANE();
    double A[9];
    for (int k = 0; k < 9; ++k) A[k] = cell[k];
    double bc[3];
    sc_cross(A + 3, A + 6, bc);
    const double V = sc_dot(A, bc);
    const double la2 = sc_dot(A, A), lb2 = sc_dot(A + 3, A + 3), lc2 = sc_dot(A + 6, A + 6);
    if (!(V > 1e-9 * sqrt(la2 * lb2 * lc2)) || !(fmax(la2, fmax(lb2, lc2)) < 1e30)) return -1 - SC_E_CELL;
    if (n <= 0) return -1 - SC_E_EMPTY;
    double len[6];
    for (int p = 0, q = 0; p < 3; ++p)
        for (int r = p; r < 3; ++r, ++q) {
            double v[3];
            for (int k = 0; k < 3; ++k) v[k] = p == r ? A[3 * p + k] : A[3 * p + k] + A[3 * r + k];
            len[q] = sqrt(sc_dot(v, v));
        }
    int nc = 0;
    for (int c0 = 0; c0 < 19683; c0 += SC_NL) {
        const int code = c0 + lane;
        bool ok = code < 19683;
        int W[9];
        if (ok) {
            int t = code;
            for (int k = 8; k >= 0; --k) { W[k] = t % 3 - 1; t /= 3; }
            double B[9];
            for (int i = 0; i < 3; ++i)
                for (int k = 0; k < 3; ++k) B[3 * i + k] = W[3 * i] * A[k] + W[3 * i + 1] * A[3 + k] + W[3 * i + 2] * A[6 + k];
            for (int p = 0, q = 0; p < 3 && ok; ++p)
                for (int r = p; r < 3 && ok; ++r, ++q) {
                    double v[3];
                    for (int k = 0; k < 3; ++k) v[k] = p == r ? B[3 * p + k] : B[3 * p + k] + B[3 * r + k];
                    ok = fabs(sqrt(sc_dot(v, v)) - len[q]) <= symprec;
                }
        }
        const int at = sc_slot(ok, nc);
        if (ok && at < SC_MAX_OPS)
            for (int k = 0; k < 9; ++k) ops[9 * at + k] = W[k];
    }
    if (nc > SC_MAX_OPS) nc = SC_MAX_OPS;
    // fractional coordinates f = r A^-1
    {
        double ca[3], ab[3];
        sc_cross(A + 6, A, ca);
        sc_cross(A, A + 3, ab);
        for (int i = lane; i < n; i += SC_NL) {
            const double* r = pos + 3 * (size_t)(a0 + i);
            frac[3 * i] = sc_dot(r, bc) / V; frac[3 * i + 1] = sc_dot(r, ca) / V; frac[3 * i + 2] = sc_dot(r, ab) / V;
        }
    }
    SC_SYNC();
    const int anchor = sc_anchor(Z + a0, n);
    const double s2 = symprec * symprec;
    int order = 0;
    for (int o0 = 0; o0 < nc; o0 += SC_NL) {
        const int o = o0 + lane;
        bool ok = false;
        int W[9];
        if (o < nc) {
            for (int k = 0; k < 9; ++k) W[k] = ops[9 * o + k];
            double ga[3];
            for (int k = 0; k < 3; ++k) ga[k] = frac[3 * anchor] * W[k] + frac[3 * anchor + 1] * W[3 + k] + frac[3 * anchor + 2] * W[6 + k];
            for (int j = 0; j < n && !ok; ++j) {
                if (Z[a0 + j] != Z[a0 + anchor]) continue;
                const double t[3] = {frac[3 * j] - ga[0], frac[3 * j + 1] - ga[1], frac[3 * j + 2] - ga[2]};
                bool all = true;
                for (int i = 0; i < n && all; ++i) {
                    double gi[3];
                    for (int k = 0; k < 3; ++k) gi[k] = frac[3 * i] * W[k] + frac[3 * i + 1] * W[3 + k] + frac[3 * i + 2] * W[6 + k] + t[k];
                    bool found = false;
                    for (int m = 0; m < n && !found; ++m) {
                        if (Z[a0 + m] != Z[a0 + i]) continue;
                        double df[3];
                        for (int k = 0; k < 3; ++k) { df[k] = gi[k] - frac[3 * m + k]; df[k] -= rint(df[k]); }
                        double e[3];
                        for (int k = 0; k < 3; ++k) e[k] = df[0] * A[k] + df[1] * A[3 + k] + df[2] * A[6 + k];
                        found = sc_dot(e, e) <= s2;
                    }
                    all = found;
                }
                ok = all;
            }
        }
        SC_SYNC();                                                     // every lane has read its operation before the list is packed
        const int at = sc_slot(ok, order);
        if (ok)
            for (int k = 0; k < 9; ++k) ops[9 * at + k] = W[k];
        SC_SYNC();
    }
    return order;
}

// Miller index e of the box |h|, |k|, |l| <= mm in descending lexicographic order; is it the representative of its class?
SC_HD bool sc_representative(const int32_t* ops, int order, int mm, int e, int* h) {
    const int wd = 2 * mm + 1;
    h[0] = mm - e / (wd * wd); h[1] = mm - (e / wd) % wd; h[2] = mm - e % wd;
    if (sc_gcd(sc_gcd(h[0], h[1]), h[2]) != 1) return false;
    for (int o = 0; o < order; ++o)
        for (int sg = -1; sg <= 1; sg += 2) {
            int g[3];
            for (int i = 0; i < 3; ++i) g[i] = sg * (ops[9 * o + 3 * i] * h[0] + ops[9 * o + 3 * i + 1] * h[1] + ops[9 * o + 3 * i + 2] * h[2]);
            if (abs(g[0]) <= mm && abs(g[1]) <= mm && abs(g[2]) <= mm && sc_lex_greater(g, h)) return false;
        }
    {   // (the identity may be missing from a refused group; -h always counts)
        const int g[3] = {-h[0], -h[1], -h[2]};
        if (sc_lex_greater(g, h)) return false;
    }
    return true;
}
// the representatives of one bulk: counted, and written to `millers` (3 ints each) where it is given and has room
SC_HD int sc_millers(const int32_t* ops, int order, int mm, int32_t* millers, int room) {
    const int lane = SC_LANE(), wd = 2 * mm + 1, total = wd * wd * wd;
    int count = 0;
    for (int e0 = 0; e0 < total; e0 += SC_NL) {
        const int e = e0 + lane;
        int h[3] = {0, 0, 0};
        const bool ok = e < total && sc_representative(ops, order, mm, e, h);
        const int at = sc_slot(ok, count);
        if (ok && millers && at < room)
            for (int k = 0; k < 3; ++k) millers[3 * at + k] = h[k];
    }
    return count;
}

// ---- kernels
struct sc_scratch {
    double *X, *Y, *H, *hs, *cut, *rd;
    int32_t *Z, *flag, *aux, *ri, *err;
    size_t bytes;
};
static sc_scratch sc_carve(void* scratch, int64_t atoms, int32_t pairs) {
    adf_carver c(scratch, 256);
    sc_scratch s;
    const size_t n = (size_t)atoms, p = (size_t)pairs;
    s.X = c.take<double>(n); s.Y = c.take<double>(n); s.H = c.take<double>(n); s.hs = c.take<double>(n); s.cut = c.take<double>(n);
    s.rd = c.take<double>(p * SC_RD);
    s.Z = c.take<int32_t>(n); s.flag = c.take<int32_t>(n); s.aux = c.take<int32_t>(n);
    s.ri = c.take<int32_t>(p * SC_RI);
    s.err = c.take<int32_t>(2);
    s.bytes = c.bytes();
    return s;
}
__host__ __device__ inline sc_seg sc_segment(const sc_scratch& w, int p, int64_t at) {
    sc_seg s;
    s.X = w.X + at; s.Y = w.Y + at; s.H = w.H + at; s.hs = w.hs + at; s.cut = w.cut + at;
    s.Z = w.Z + at; s.flag = w.flag + at; s.aux = w.aux + at;
    s.rd = w.rd + (size_t)p * SC_RD; s.ri = w.ri + (size_t)p * SC_RI;
    return s;
}

// counts [3 P]: slabs of the pair, atoms of each, error bits.  A pair whose bulk index or segment is out of range, or whose
// segment is shorter than its bulk, is an error of the caller (bit 32) and touches nothing.
__global__ __launch_bounds__(SC_THREADS) void sc_count_kernel(
    const double* __restrict__ pos, const double* __restrict__ cell, const int32_t* __restrict__ Z,
    const int32_t* __restrict__ atom_offset, int num_atoms, int num_bulks, const int32_t* __restrict__ pair_bulk,
    const int32_t* __restrict__ pair_miller, const int64_t* __restrict__ pair_atom_offset, int num_pairs, long long seg_atoms,
    sc_params P, sc_scratch w, int32_t* __restrict__ counts) {
    const int p = blockIdx.x * SC_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= num_pairs) return;
    const int b = pair_bulk[p];
    const long long at = pair_atom_offset[p], end = pair_atom_offset[p + 1];
    bool bad = b < 0 || b >= num_bulks || at < 0 || end < at || end > seg_atoms;
    int a0 = 0, n = 0;
    if (!bad) {
        a0 = atom_offset[b];
        n = atom_offset[b + 1] - a0;
        bad = a0 < 0 || n < 0 || (long long)a0 + n > num_atoms || end - at < n;
    }
    if (bad) {
        if (lane == 0) { counts[3 * p] = 0; counts[3 * p + 1] = 0; counts[3 * p + 2] = 32; }
        return;
    }
    const sc_seg s = sc_segment(w, p, at);
    sc_analyze(pos, cell + 9 * (size_t)b, Z, a0, n, pair_miller + 3 * (size_t)p, P, s);
    SC_SYNC();
    if (lane == 0) {
        const int err = s.ri[SC_ERR];
        counts[3 * p] = err ? 0 : s.ri[SC_NOUT];
        counts[3 * p + 1] = err ? 0 : s.ri[SC_NP] * s.ri[SC_NSLAB];
        counts[3 * p + 2] = err;
    }
}

// Do the caller's offsets say what the count pass found, and do they fit the buffers?  One thread; err[0] = 1 + the first
// pair that does not (0: all is well).
__global__ void sc_capacity_kernel(const int32_t* __restrict__ pair_slab_offset, const int64_t* __restrict__ pair_out_offset,
                                   int num_pairs, int slab_cap, long long atom_cap, sc_scratch w) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int bad = 0;
    if (pair_slab_offset[0] != 0 || pair_out_offset[0] != 0) bad = 1;
    for (int p = 0; p < num_pairs && !bad; ++p) {
        const int32_t* ri = w.ri + (size_t)p * SC_RI;
        const long long ns = ri[SC_ERR] ? 0 : ri[SC_NOUT], na = ns * ri[SC_NP] * ri[SC_NSLAB];
        if (pair_slab_offset[p + 1] - (long long)pair_slab_offset[p] != ns || pair_out_offset[p + 1] - pair_out_offset[p] != na ||
            pair_slab_offset[p + 1] > slab_cap || pair_out_offset[p + 1] > atom_cap)
            bad = p + 1;
    }
    w.err[0] = bad;
}

__global__ __launch_bounds__(SC_THREADS) void sc_fill_kernel(
    const int32_t* __restrict__ pair_bulk, const int64_t* __restrict__ pair_atom_offset, const int32_t* __restrict__ pair_slab_offset,
    const int64_t* __restrict__ pair_out_offset, int num_pairs, double symprec, sc_scratch w,
    double* __restrict__ pos64, float* __restrict__ pos32, int32_t* __restrict__ Zout, double* __restrict__ cell,
    int32_t* __restrict__ millers, double* __restrict__ shift, int32_t* __restrict__ top, int32_t* __restrict__ bulk_index,
    int32_t* __restrict__ natoms) {
    if (w.err[0] != 0) return;
    const int p = blockIdx.x;
    const sc_seg s = sc_segment(w, p, pair_atom_offset[p]);
    if (s.ri[SC_ERR] != 0) return;
    const int nout = s.ri[SC_NOUT];
    for (int q = blockIdx.y * SC_WAVES + (threadIdx.x >> 6); q < nout; q += gridDim.y * SC_WAVES) {
        const size_t slab = (size_t)pair_slab_offset[p] + q;
        const size_t at = (size_t)pair_out_offset[p] + (size_t)q * s.ri[SC_NP] * s.ri[SC_NSLAB];
        sc_out o;
        o.pos64 = pos64 + 3 * at; o.pos32 = pos32 + 3 * at; o.Z = Zout + at;
        o.cell = cell + 9 * slab; o.millers = millers + 3 * slab; o.shift = shift + slab; o.top = top + slab;
        o.bulk_index = bulk_index + slab; o.natoms = natoms + slab;
        sc_emit(s, symprec, q, pair_bulk[p], o);
    }
}

// found [3 B]: Miller indices, order of the point group, error bits
__global__ __launch_bounds__(SC_THREADS) void sc_group_kernel(
    const double* __restrict__ pos, const double* __restrict__ cell, const int32_t* __restrict__ Z,
    const int32_t* __restrict__ atom_offset, int num_atoms, int num_bulks, int max_miller, double symprec,
    int32_t* __restrict__ ops, double* __restrict__ frac, int32_t* __restrict__ found) {
    const int b = blockIdx.x * SC_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= num_bulks) return;
    const int a0 = atom_offset[b], n = atom_offset[b + 1] - a0;
    if (a0 < 0 || n < 0 || (long long)a0 + n > num_atoms) {
        if (lane == 0) { found[3 * b] = 0; found[3 * b + 1] = 0; found[3 * b + 2] = 32; }
        return;
    }
    int32_t* mine = ops + (size_t)b * SC_GROUP_WORDS;
    const int order = sc_group(pos, cell + 9 * (size_t)b, Z, a0, n, symprec, mine, frac + 3 * (size_t)a0);
    SC_SYNC();
    const int count = order > 0 ? sc_millers(mine, order, max_miller, nullptr, 0) : 0;
    if (lane == 0) {
        found[3 * b] = count;
        found[3 * b + 1] = order > 0 ? order : 0;
        found[3 * b + 2] = order < 0 ? -1 - order : order == 0 ? SC_E_TRANS : 0;
    }
}

__global__ __launch_bounds__(SC_THREADS) void sc_millers_kernel(const int32_t* __restrict__ ops, const int32_t* __restrict__ found,
                                                                const int32_t* __restrict__ miller_offset, int num_bulks,
                                                                int max_miller, int capacity, int32_t* __restrict__ millers) {
    const int b = blockIdx.x * SC_WAVES + (threadIdx.x >> 6);
    if (b >= num_bulks) return;
    const int at = miller_offset[b], room = miller_offset[b + 1] - at;
    if (at < 0 || room < 0 || (long long)at + room > capacity || found[3 * b + 2] != 0 || room != found[3 * b]) return;
    (void)sc_millers(ops + (size_t)b * SC_GROUP_WORDS, found[3 * b + 1], max_miller, millers + 3 * (size_t)at, room);
}

// ---- host side
static bool sc_positive(double v) { return v > 0.0 && v < 1e30; }

static const char* sc_reason(int32_t bits) {
    return bits & 32 ? "its offsets are out of range" : bits & SC_E_ZERO ? "Miller index (0,0,0)" :
           bits & SC_E_CELL ? "a singular, left-handed or non-finite cell" : bits & SC_E_EMPTY ? "no atoms" :
           bits & SC_E_SIZE ? "the slab would exceed 2^20 atoms" :
           "the translations (operations) found at this symprec do not form a group";
}

struct sc_millers_scratch {
    int32_t* ops;
    double* frac;
    size_t bytes;
};
static sc_millers_scratch sc_millers_carve(void* scratch, int32_t num_atoms, int32_t num_bulks) {
    adf_carver c(scratch, 256);
    sc_millers_scratch s;
    s.ops = c.take<int32_t>((size_t)num_bulks * SC_GROUP_WORDS);
    s.frac = c.take<double>(3 * (size_t)num_atoms);
    s.bytes = c.bytes();
    return s;
}

extern "C" int64_t adf_distinct_millers_scratch(int32_t num_atoms, int32_t num_bulks) {
    if (num_atoms < 0 || num_bulks < 0) return 0;
    return (int64_t)sc_millers_carve(nullptr, num_atoms, num_bulks).bytes;
}

extern "C" int32_t adf_distinct_millers_count(const double* pos, const double* cell, const int32_t* atomic_numbers,
                                              const int32_t* atom_offset, int32_t num_atoms, int32_t num_bulks,
                                              int32_t max_miller, double symprec, void* scratch, int32_t* found,
                                              int32_t* found_host, void* stream) {
    if (!pos || !cell || !atomic_numbers || !atom_offset || !scratch || !found || !found_host) {
        adf_set_error("distinct_millers_count: null argument");
        return ADF_EINVAL;
    }
    if (num_atoms <= 0 || num_bulks <= 0 || max_miller < 1 || max_miller > 4 || !sc_positive(symprec)) {
        adf_set_error("distinct_millers_count: %d atoms, %d bulks, max_miller %d (1 .. 4), symprec %g (finite, positive)",
                      num_atoms, num_bulks, max_miller, symprec);
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const sc_millers_scratch w = sc_millers_carve(scratch, num_atoms, num_bulks);
    hipLaunchKernelGGL(sc_group_kernel, dim3((num_bulks + SC_WAVES - 1) / SC_WAVES), dim3(SC_THREADS), 0, s, pos, cell,
                       atomic_numbers, atom_offset, num_atoms, num_bulks, max_miller, symprec, w.ops, w.frac, found);
    ADF_HIP_CHECK(hipGetLastError());
    ADF_HIP_CHECK(hipMemcpyAsync(found_host, found, 3 * (size_t)num_bulks * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ADF_HIP_CHECK(hipStreamSynchronize(s));
    for (int32_t b = 0; b < num_bulks; ++b)
        if (found_host[3 * b + 2] != 0) {
            adf_set_error("distinct_millers_count: bulk %d: %s", b, sc_reason(found_host[3 * b + 2]));
            return ADF_EINVAL;
        }
    return ADF_OK;
}

extern "C" int32_t adf_distinct_millers_fill(const void* scratch, const int32_t* found, const int32_t* found_host,
                                             const int32_t* miller_offset, int32_t num_atoms, int32_t num_bulks,
                                             int32_t max_miller, int32_t capacity, int32_t* millers, void* stream) {
    if (!scratch || !found || !found_host || !miller_offset || !millers) {
        adf_set_error("distinct_millers_fill: null argument");
        return ADF_EINVAL;
    }
    if (num_atoms <= 0 || num_bulks <= 0 || max_miller < 1 || max_miller > 4 || capacity < 0) {
        adf_set_error("distinct_millers_fill: %d atoms, %d bulks, max_miller %d, capacity %d", num_atoms, num_bulks, max_miller,
                      capacity);
        return ADF_EINVAL;
    }
    long long total = 0;
    for (int32_t b = 0; b < num_bulks; ++b) {
        total += found_host[3 * b];
        if (total > capacity) {
            adf_set_error("distinct_millers_fill: bulk %d: %lld Miller indices up to it, room for %d", b, total, capacity);
            return ADF_EOVERFLOW;
        }
    }
    const sc_millers_scratch w = sc_millers_carve(const_cast<void*>(scratch), num_atoms, num_bulks);
    hipLaunchKernelGGL(sc_millers_kernel, dim3((num_bulks + SC_WAVES - 1) / SC_WAVES), dim3(SC_THREADS), 0, (hipStream_t)stream,
                       w.ops, found, miller_offset, num_bulks, max_miller, capacity, millers);
    ADF_HIP_CHECK(hipGetLastError());
    return ADF_OK;
}

extern "C" int64_t adf_slab_cut_scratch(int64_t segment_atoms, int32_t num_pairs) {
    if (segment_atoms < 0 || num_pairs < 0) return 0;
    return (int64_t)sc_carve(nullptr, segment_atoms, num_pairs).bytes;
}

extern "C" int32_t adf_slab_cut_count(const double* pos, const double* cell, const int32_t* atomic_numbers,
                                      const int32_t* atom_offset, int32_t num_atoms, int32_t num_bulks, const int32_t* pair_bulk,
                                      const int32_t* pair_miller, const int64_t* pair_atom_offset, int32_t num_pairs,
                                      int64_t segment_atoms, double min_slab_size, double min_vacuum_size, double tol,
                                      double symprec, void* scratch, int32_t* counts, int32_t* counts_host, void* stream) {
    if (!pos || !cell || !atomic_numbers || !atom_offset || !pair_bulk || !pair_miller || !pair_atom_offset || !scratch ||
        !counts || !counts_host) {
        adf_set_error("slab_cut_count: null argument");
        return ADF_EINVAL;
    }
    if (num_atoms <= 0 || num_bulks <= 0 || num_pairs <= 0 || segment_atoms <= 0) {
        adf_set_error("slab_cut_count: %d atoms, %d bulks, %d pairs, %lld segment atoms", num_atoms, num_bulks, num_pairs,
                      (long long)segment_atoms);
        return ADF_EINVAL;
    }
    if (!sc_positive(min_slab_size) || !sc_positive(min_vacuum_size) || !sc_positive(tol) || !sc_positive(symprec)) {
        adf_set_error("slab_cut_count: min_slab_size %g, min_vacuum_size %g, tol %g, symprec %g: finite and positive expected",
                      min_slab_size, min_vacuum_size, tol, symprec);
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const sc_scratch w = sc_carve(scratch, segment_atoms, num_pairs);
    sc_params P;
    P.min_slab = min_slab_size; P.min_vac = min_vacuum_size; P.tol = tol; P.symprec = symprec;
    hipLaunchKernelGGL(sc_count_kernel, dim3((num_pairs + SC_WAVES - 1) / SC_WAVES), dim3(SC_THREADS), 0, s, pos, cell,
                       atomic_numbers, atom_offset, num_atoms, num_bulks, pair_bulk, pair_miller, pair_atom_offset, num_pairs,
                       (long long)segment_atoms, P, w, counts);
    ADF_HIP_CHECK(hipGetLastError());
    ADF_HIP_CHECK(hipMemcpyAsync(counts_host, counts, 3 * (size_t)num_pairs * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ADF_HIP_CHECK(hipStreamSynchronize(s));
    for (int32_t p = 0; p < num_pairs; ++p)
        if (counts_host[3 * p + 2] != 0) {
            int32_t b = -1;
            (void)hipMemcpy(&b, pair_bulk + p, sizeof(int32_t), hipMemcpyDeviceToHost);
            adf_set_error("slab_cut_count: bulk %d (pair %d): %s", b, p, sc_reason(counts_host[3 * p + 2]));
            return ADF_EINVAL;
        }
    return ADF_OK;
}

extern "C" int32_t adf_slab_cut_fill(const void* scratch, const int32_t* pair_bulk, const int64_t* pair_atom_offset,
                                     const int32_t* pair_slab_offset, const int64_t* pair_out_offset, int32_t num_pairs,
                                     int64_t segment_atoms, double symprec, int32_t slab_capacity, int64_t atom_capacity,
                                     double* pos64, float* pos32, int32_t* atomic_numbers, double* cell, int32_t* millers,
                                     double* shift, int32_t* top, int32_t* bulk_index, int32_t* natoms, void* stream) {
    if (!scratch || !pair_bulk || !pair_atom_offset || !pair_slab_offset || !pair_out_offset || !pos64 || !pos32 ||
        !atomic_numbers || !cell || !millers || !shift || !top || !bulk_index || !natoms) {
        adf_set_error("slab_cut_fill: null argument");
        return ADF_EINVAL;
    }
    if (num_pairs <= 0 || segment_atoms <= 0 || slab_capacity < 0 || atom_capacity < 0 || !sc_positive(symprec)) {
        adf_set_error("slab_cut_fill: %d pairs, %lld segment atoms, room for %d slabs and %lld atoms, symprec %g", num_pairs,
                      (long long)segment_atoms, slab_capacity, (long long)atom_capacity, symprec);
        return ADF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const sc_scratch w = sc_carve(const_cast<void*>(scratch), segment_atoms, num_pairs);
    hipLaunchKernelGGL(sc_capacity_kernel, dim3(1), dim3(64), 0, s, pair_slab_offset, pair_out_offset, num_pairs, slab_capacity,
                       (long long)atom_capacity, w);
    ADF_HIP_CHECK(hipGetLastError());
    // the second axis: two workgroups of four waves per pair, each wave walks the pair's slabs from its own
    hipLaunchKernelGGL(sc_fill_kernel, dim3(num_pairs, 2), dim3(SC_THREADS), 0, s, pair_bulk, pair_atom_offset, pair_slab_offset,
                       pair_out_offset, num_pairs, symprec, w, pos64, pos32, atomic_numbers, cell, millers, shift, top, bulk_index,
                       natoms);
    ADF_HIP_CHECK(hipGetLastError());
    int32_t bad = 0;
    ADF_HIP_CHECK(hipMemcpyAsync(&bad, w.err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ADF_HIP_CHECK(hipStreamSynchronize(s));
    if (bad != 0) {
        int32_t b = -1;
        (void)hipMemcpy(&b, pair_bulk + (bad - 1), sizeof(int32_t), hipMemcpyDeviceToHost);
        adf_set_error("slab_cut_fill: bulk %d (pair %d): its slabs do not fit the output (room for %d slabs, %lld atoms) or the "
                      "offsets are not the count pass's", b, bad - 1, slab_capacity, (long long)atom_capacity);
        return ADF_EOVERFLOW;
    }
    return ADF_OK;
}
