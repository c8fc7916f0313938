// The element building blocks every solid element kernel includes; each exists here once.
//
//   material      lame / dmat: the Lame pair and the three distinct entries of the reference's isotropic D
//   indexing      sym_blk: the upper-triangle block index of the packed symmetric element matrices
//   arithmetic    dop / dot3c: compensated a b - c d and 3-term dot (det F and the cofactors of F); inv3
//   c3d4          tet4_grads*: P1 gradients and signed det; tet4_det_sorted: the order-independent |det| of the mass;
//                 tet4_disp_grad: H = sum_a u_a (x) g_a
//   isoparametric ISO_MAX_IP, the point limit of every staged rule table
//   stress        point_stress / store_tensor: strain -> stress -> von Mises, the thermal strain a compile-time option
//   c3d4 tangent  tet4_tangent_index / tet4_tangent_store / tet4_force_store: the shell that writes a 64-element
//                 block's records out as packed or full tangents and element forces (nonlinear.hip, plasticity.hip)
//
// What is NOT shared, on purpose: the degeneracy predicates (`fabs(det) < 1e-12` lets a NaN pass, `!(fabs(det) >=
// 1e-12)` does not; each kernel keeps its own), the volume forms, and which callers run under fp contract(off). A
// helper here carries its own contraction: one with the pragma gives every caller unfused arithmetic, one without it
// the compiler's default, whatever the caller's setting. The isoparametric chain J -> inv3 -> g = J^-1 dN also stays
// written out in its thread-per-element kernels: as a function here it changed which loads the compiler merges and,
// through that, how point_stress's sums are contracted -- the last bits of the c3d6 / c3d8 / c3d10 stresses.
#pragma once
#include "common.hpp"

namespace fem {

constexpr int ISO_MAX_IP = 32;   // quadrature points per rule: the size of the dN / N / w tables staged in LDS

struct Lame {
    double lam, mu;
};

__host__ __device__ inline Lame lame(double E, double nu) {
    // same coefficient the reference forms: coef = E/((1+nu)(1-2nu)); D33 = coef*(1-2nu)/2
    double c = E / ((1.0 + nu) * (1.0 - 2.0 * nu));
    return Lame{c * nu, c * ((1.0 - 2.0 * nu) / 2.0)};
}

struct Dmat {
    double d0, d1, g;   // D[0][0] = c(1-nu), D[0][1] = c nu, D[3][3] = c (1-2nu)/2 (`solver/element.py:282-306`)
};

__host__ __device__ inline Dmat dmat(double E, double nu) {
    const double c = E / ((1.0 + nu) * (1.0 - 2.0 * nu));
    return Dmat{c * (1.0 - nu), c * nu, c * ((1.0 - 2.0 * nu) / 2.0)};
}

// index of block (a, b), a <= b, in the row-major walk over the upper triangle of an npe x npe block matrix
__host__ __device__ constexpr int sym_blk(int npe, int a, int b) { return a * npe - a * (a - 1) / 2 + (b - a); }

// a b - c d with the rounding error of c d carried along (Kahan): within 1.5 ulp of the exact difference, where the
// plain form loses every digit the two products share
__device__ __forceinline__ double dop(double a, double b, double c, double d) {
#pragma clang fp contract(off)
    const double w = c * d;
    const double e = fma(-c, d, w);
    const double f = fma(a, b, -w);
    return f + e;
}

// x0 y0 + x1 y1 + x2 y2 with the errors of the products and of the two sums collected and added once
__device__ __forceinline__ double dot3c(double x0, double y0, double x1, double y1, double x2, double y2) {
#pragma clang fp contract(off)
    const double p0 = x0 * y0, p1 = x1 * y1, p2 = x2 * y2;
    const double e0 = fma(x0, y0, -p0), e1 = fma(x1, y1, -p1), e2 = fma(x2, y2, -p2);
    const double s = p0 + p1;
    const double b1 = s - p0;
    const double t1 = (p0 - (s - b1)) + (p1 - b1);
    const double s2 = s + p2;
    const double b2 = s2 - s;
    const double t2 = (s - (s2 - b2)) + (p2 - b2);
    return s2 + ((t1 + t2) + ((e0 + e1) + e2));
}

// gradients of the P1 shape functions (rows 1..3 of inv([1 x y z])) and the signed det of the edge matrix, from the
// 4 vertices' coordinates
__device__ __forceinline__ double tet4_grads_p(const double p[4][3], double g[4][3]) {
    double e1[3], e2[3], e3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e1[k] = p[1][k] - p[0][k];
        e2[k] = p[2][k] - p[0][k];
        e3[k] = p[3][k] - p[0][k];
    }
    double c23[3] = {e2[1] * e3[2] - e2[2] * e3[1], e2[2] * e3[0] - e2[0] * e3[2], e2[0] * e3[1] - e2[1] * e3[0]};
    double c31[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
    double c12[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    double det = e1[0] * c23[0] + e1[1] * c23[1] + e1[2] * c23[2];
    double inv = 1.0 / det;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g[1][k] = c23[k] * inv;
        g[2][k] = c31[k] * inv;
        g[3][k] = c12[k] * inv;
        g[0][k] = -(g[1][k] + g[2][k] + g[3][k]);
    }
    return det;
}

// the same from the element's node ids (already loaded)
__device__ __forceinline__ double tet4_grads_n(const double* __restrict__ X, const int64_t c[4], double g[4][3]) {
    double p[4][3];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int64_t n = c[a];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[a][k] = X[3 * n + k];
    }
    return tet4_grads_p(p, g);
}

__device__ __forceinline__ double tet4_grads(const double* __restrict__ X, const int64_t* __restrict__ c,
                                             double g[4][3]) {
    const int64_t n[4] = {c[0], c[1], c[2], c[3]};
    return tet4_grads_n(X, n, g);
}

// signed det of the edge matrix with the 4 nodes taken in ascending global id. |det| is a symmetric function of the
// nodes; formed from the local order it rounds differently in the last bit when an element is renumbered (other
// edges are differenced). Sorted, any local order of the same nodes gives the same |det| bit for bit (the c3d4 mass).
__device__ __forceinline__ double tet4_det_sorted(const double* __restrict__ X, const int64_t* __restrict__ c) {
    int64_t n[4] = {c[0], c[1], c[2], c[3]};
#define FEM_CSWAP(i, j)                \
    if (n[j] < n[i]) {                 \
        const int64_t t_ = n[i];       \
        n[i] = n[j];                   \
        n[j] = t_;                     \
    }
    FEM_CSWAP(0, 1) FEM_CSWAP(2, 3) FEM_CSWAP(0, 2) FEM_CSWAP(1, 3) FEM_CSWAP(1, 2)
#undef FEM_CSWAP
    double e1[3], e2[3], e3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double p0 = X[3 * n[0] + k];
        e1[k] = X[3 * n[1] + k] - p0;
        e2[k] = X[3 * n[2] + k] - p0;
        e3[k] = X[3 * n[3] + k] - p0;
    }
    return e1[0] * (e2[1] * e3[2] - e2[2] * e3[1]) + e1[1] * (e2[2] * e3[0] - e2[0] * e3[2]) +
           e1[2] * (e2[0] * e3[1] - e2[1] * e3[0]);
}

// displacement gradient H = sum_a u_a (x) g_a of a c3d4 element, every entry summed over a in ascending order and no
// product fused into a sum (the callers' TAN on / off and packed / full outputs agree bit for bit through it)
__device__ __forceinline__ void tet4_disp_grad(const double u[4][3], const double g[4][3], double H[3][3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) H[i][j] = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) H[i][j] += u[a][i] * g[a][j];
}

// inverse of a row-major 3x3 Jacobian (cofactors), returns det
__device__ __forceinline__ double inv3(const double J[9], double Ji[9]) {
    const double c00 = J[4] * J[8] - J[5] * J[7], c01 = J[5] * J[6] - J[3] * J[8], c02 = J[3] * J[7] - J[4] * J[6];
    const double det = J[0] * c00 + J[1] * c01 + J[2] * c02;
    const double id = 1.0 / det;
    Ji[0] = c00 * id;
    Ji[1] = (J[2] * J[7] - J[1] * J[8]) * id;
    Ji[2] = (J[1] * J[5] - J[2] * J[4]) * id;
    Ji[3] = c01 * id;
    Ji[4] = (J[0] * J[8] - J[2] * J[6]) * id;
    Ji[5] = (J[2] * J[3] - J[0] * J[5]) * id;
    Ji[6] = c02 * id;
    Ji[7] = (J[1] * J[6] - J[0] * J[7]) * id;
    Ji[8] = (J[0] * J[4] - J[1] * J[3]) * id;
    return det;
}

// strain from gradients g[a][k] and displacements u[a][k] (Voigt xx, yy, zz, xy, yz, xz, engineering shear) ->
// stress (6) -> von Mises. TH: the thermal strain eth = alpha dT is taken off the normal entries before D; without
// it eth is not read and nothing is subtracted.
template <int NPE, bool TH>
__device__ __forceinline__ double point_stress(const double g[NPE][3], const double u[NPE][3], const Dmat& D,
                                               double eth, double s[6]) {
    double e[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < NPE; ++a) {
        e[0] += g[a][0] * u[a][0];
        e[1] += g[a][1] * u[a][1];
        e[2] += g[a][2] * u[a][2];
        e[3] += g[a][1] * u[a][0] + g[a][0] * u[a][1];
        e[4] += g[a][2] * u[a][1] + g[a][1] * u[a][2];
        e[5] += g[a][2] * u[a][0] + g[a][0] * u[a][2];
    }
    if constexpr (TH) {
        e[0] -= eth;
        e[1] -= eth;
        e[2] -= eth;
    }
    s[0] = D.d0 * e[0] + D.d1 * e[1] + D.d1 * e[2];
    s[1] = D.d1 * e[0] + D.d0 * e[1] + D.d1 * e[2];
    s[2] = D.d1 * e[0] + D.d1 * e[1] + D.d0 * e[2];
    s[3] = D.g * e[3];
    s[4] = D.g * e[4];
    s[5] = D.g * e[5];
    const double a = s[0] - s[1], b = s[1] - s[2], c = s[2] - s[0];
    return sqrt((a * a + b * b + c * c + 6.0 * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5])) / 2.0);
}

// symmetric tensor rows (xx xy xz / xy yy yz / xz yz zz) with Voigt (xx, yy, zz, xy, yz, xz)
__device__ __forceinline__ void store_tensor(double* __restrict__ out, const double s[6]) {
    out[0] = s[0];
    out[1] = s[3];
    out[2] = s[5];
    out[3] = s[3];
    out[4] = s[1];
    out[5] = s[4];
    out[6] = s[5];
    out[7] = s[4];
    out[8] = s[2];
}

// ---------------------------------------------------------------- c3d4 record -> tangent shell
// The c3d4 tangent kernels take 64 elements per 256-thread block: 64 lanes form one record of REC doubles per element
// in LDS (what the material's block formula reads, then the 12 element forces), and after a barrier all 256 threads
// write the block's contiguous tangent values and forces coalesced through the three functions below.

// value q of an element's tangent -> upper block (a, b), a <= b, and entry (i, k) in it. PACKED: fem_iso_ke_sym's
// layout for npe = 4 (blocks in sym_blk order, 9 doubles each; 90 per element); else the full row-major [12, 12],
// where a lower block comes back as its upper one with (a, i) and (b, k) exchanged. Both forms reach the entry
// function with the same arguments for the same value, which is what makes the full matrix the packed one mirrored
// bit for bit, and exactly symmetric.
template <bool PACKED>
__device__ __forceinline__ void tet4_tangent_index(int q, int& a, int& b, int& i, int& k) {
    if (PACKED) {
        const int blk = q / 9, rc = q - 9 * (q / 9);
        a = blk < 4 ? 0 : (blk < 7 ? 1 : (blk < 9 ? 2 : 3));
        b = blk - sym_blk(4, a, a) + a;
        i = rc / 3;
        k = rc - 3 * i;
    } else {
        const int row = q / 12, col = q - 12 * (q / 12);
        a = row / 3;
        i = row - 3 * a;
        b = col / 3;
        k = col - 3 * b;
        if (a > b) {   // a lower block: the transpose of its upper one
            const int ta = a, ti = i;
            a = b;
            b = ta;
            i = k;
            k = ti;
        }
    }
}

// the tangents of the block's nel elements (the first is element e0) from their records: entry(record, a, b, i, k)
// is the material's block formula
template <int REC, bool PACKED, class Entry>
__device__ __forceinline__ void tet4_tangent_store(const double* rec_s, int64_t e0, int nel, double* __restrict__ Kt,
                                                   Entry entry) {
    constexpr int PS = PACKED ? 90 : 144;
    const int nval = nel * PS;
    double* out = Kt + e0 * PS;
    for (int t = threadIdx.x; t < nval; t += 256) {
        const int le = t / PS;
        int a, b, i, k;
        tet4_tangent_index<PACKED>(t - le * PS, a, b, i, k);
        out[t] = entry(rec_s + le * REC, a, b, i, k);
    }
}

// the element forces [nel, 4, 3], kept at offset FE0 of each record
template <int REC, int FE0>
__device__ __forceinline__ void tet4_force_store(const double* rec_s, int64_t e0, int nel, double* __restrict__ fe) {
    double* out = fe + e0 * 12;
    for (int t = threadIdx.x; t < nel * 12; t += 256) {
        const int le = t / 12;
        out[t] = rec_s[le * REC + FE0 + (t - 12 * le)];
    }
}

}  // namespace fem
