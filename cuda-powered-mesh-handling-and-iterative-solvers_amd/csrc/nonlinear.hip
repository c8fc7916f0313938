// Geometrically nonlinear (total-Lagrangian) c3d4 elasticity on gfx950: internal force, consistent tangent stiffness,
// strain energy and Cauchy stress of every tet from the current displacement, for two hyperelastic materials.
//
// With the reference gradients g_a and volume V of tet4_grads (element.hpp), H = sum_a u_a (x) g_a, F = I + H,
// J = det F and the Lame constants of lame(E, nu):
//   St. Venant-Kirchhoff  W = lam/2 (tr E)^2 + mu E:E, E = (H + H^T + H^T H)/2, S = lam tr(E) I + 2 mu E, P = F S
//     block (a,b)(i,k) / V = (g_a.S g_b) d_ik + lam (F g_a)_i (F g_b)_k + mu (F g_b)_i (F g_a)_k + mu (g_a.g_b)(F F^T)_ik
//   compressible neo-Hooke W = mu/2 (F:F - 3) - mu ln J + lam/2 (ln J)^2, P = mu (F - F^-T) + lam ln J F^-T, h_a = F^-T g_a
//     block (a,b)(i,k) / V = mu (g_a.g_b) d_ik + (mu - lam ln J) h_b,i h_a,k + lam h_a,i h_b,k
// element force on node a: V P g_a; Cauchy stress J^-1 P F^T. Both reduce to k_tet4_ke's linear block at u = 0.
// The strains are formed from H (not from F^T F - I), so u = 0 gives exactly zero force for both materials.
#include <math.h>

#include "common.hpp"
#include "element.hpp"

namespace fem {

// per-element record in LDS (doubles): what the block formula reads, then the element forces
constexpr int NL_X = 0;     // [4][3] F g_a (svk) / h_a (neo-Hooke)
constexpr int NL_GG = 12;   // [10] g_a.g_b, a <= b, at sym_blk(4, a, b)
constexpr int NL_C = 22;    // [10] the d_ik factor: g_a.S g_b (svk) / mu g_a.g_b (neo-Hooke)
constexpr int NL_FF = 32;   // [6] F F^T (xx, yy, zz, xy, yz, xz), svk only
constexpr int NL_V = 38;    // V (0 for an element whose outputs are zero)
constexpr int NL_COEF = 39; // mu - lam ln J (neo-Hooke)
constexpr int NL_TAN = 40;  // record length of the tangent part
constexpr int NL_REC_T = 53;   // tangent part + 12 forces, odd stride
constexpr int NL_REC_F = 13;   // forces only

// entry (i, k) of the upper block (a, b), a <= b, from the element's record. The packed and the full form both come
// through here with the same arguments (the full form's lower blocks with (a, i) and (b, k) exchanged), and no product
// is fused into a sum, so the two agree bit for bit and the full matrix is exactly symmetric.
template <int MAT>
__device__ __forceinline__ double nl_entry(const double* __restrict__ r, int a, int b, int i, int k, double lam,
                                           double mu) {
#pragma clang fp contract(off)
    const int blk = sym_blk(4, a, b);
    const double* xa = r + NL_X + 3 * a;
    const double* xb = r + NL_X + 3 * b;
    const double p = xa[i] * xb[k];
    const double q = xb[i] * xa[k];
    double s = (i == k) ? r[NL_C + blk] : 0.0;
    if (MAT == FEM_MAT_SVK) {
        const int ik = (i == k) ? i : (i + k == 1 ? 3 : (i + k == 3 ? 4 : 5));
        s = ((s + lam * p) + mu * q) + mu * (r[NL_GG + blk] * r[NL_FF + ik]);
    } else {
        s = (s + r[NL_COEF] * q) + lam * p;
    }
    return s * r[NL_V];
}

// One lane: everything of element e that does not depend on the output entry, into the record r and the per-element
// outputs. det F and the cofactors of F are formed by dop / dot3c (element.hpp): a deformation gradient with entries far above
// its determinant (a sliver mesh carrying a finite strain: F ~ 1e3, J ~ 1) left the plain cofactor expansion 35 x
// less accurate than the rounding of F itself allows (tests/test_gpu_hard_geometry_nl.py). An inverted element (det F <= 0) or a degenerate reference element gets a zero record, zero stress and
// energy +inf; no logarithm of a non-positive number is taken and no NaN is stored. Products are not fused into sums
// here either, so the TAN = false build gives the forces and energies of the TAN = true build bit for bit.
template <int MAT, bool TAN>
__device__ __forceinline__ void nl_element(const double* __restrict__ X, const int64_t* __restrict__ conn, int64_t e,
                                           const double* __restrict__ U, double lam, double mu, double* __restrict__ r,
                                           double* __restrict__ we, double* __restrict__ sigma,
                                           double* __restrict__ detF, int64_t* __restrict__ bad,
                                           int64_t* __restrict__ inverted) {
#pragma clang fp contract(off)
    constexpr int FE0 = TAN ? NL_TAN : 0;
    const int64_t n[4] = {conn[4 * e], conn[4 * e + 1], conn[4 * e + 2], conn[4 * e + 3]};
    double g[4][3];
    const double det = tet4_grads_n(X, n, g);
    const bool degenerate = !(fabs(det) >= 1e-12);
    if (degenerate) atomicMin((unsigned long long*)bad, (unsigned long long)e);
    const double V = fabs(det) / 6.0;
    double u[4][3], H[3][3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) u[a][k] = U[3 * n[a] + k];
    tet4_disp_grad(u, g, H);
    double F[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) F[i][j] = (i == j ? 1.0 : 0.0) + H[i][j];
    // cofactors of F (Cf[i][j] = cofactor of F[i][j]); det F by the first row
    double Cf[3][3];
    Cf[0][0] = dop(F[1][1], F[2][2], F[1][2], F[2][1]);
    Cf[0][1] = dop(F[1][2], F[2][0], F[1][0], F[2][2]);
    Cf[0][2] = dop(F[1][0], F[2][1], F[1][1], F[2][0]);
    const double J = dot3c(F[0][0], Cf[0][0], F[0][1], Cf[0][1], F[0][2], Cf[0][2]);
    const bool ok = !degenerate && J > 0.0;   // false for a NaN as well
    if (detF) detF[e] = (degenerate || J != J) ? 0.0 : J;
    if (!ok) {
        if (!degenerate) atomicMin((unsigned long long*)inverted, (unsigned long long)e);
#pragma unroll
        for (int t = 0; t < FE0 + 12; ++t) r[t] = 0.0;
        if (we) we[e] = INFINITY;
        if (sigma) {
#pragma unroll
            for (int t = 0; t < 6; ++t) sigma[6 * e + t] = 0.0;
        }
        return;
    }
    // F g_a
    double Fg[4][3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int i = 0; i < 3; ++i) Fg[a][i] = (F[i][0] * g[a][0] + F[i][1] * g[a][1]) + F[i][2] * g[a][2];
    double sg[6];   // Cauchy stress (xx, yy, zz, xy, yz, xz)
    double W;
    const double iJ = 1.0 / J;
    if (MAT == FEM_MAT_SVK) {
        // Green-Lagrange strain (xx, yy, zz, xy, yz, xz) from H
        double Ed[6];
        Ed[0] = H[0][0] + 0.5 * ((H[0][0] * H[0][0] + H[1][0] * H[1][0]) + H[2][0] * H[2][0]);
        Ed[1] = H[1][1] + 0.5 * ((H[0][1] * H[0][1] + H[1][1] * H[1][1]) + H[2][1] * H[2][1]);
        Ed[2] = H[2][2] + 0.5 * ((H[0][2] * H[0][2] + H[1][2] * H[1][2]) + H[2][2] * H[2][2]);
        Ed[3] = 0.5 * ((H[0][1] + H[1][0]) + ((H[0][0] * H[0][1] + H[1][0] * H[1][1]) + H[2][0] * H[2][1]));
        Ed[4] = 0.5 * ((H[1][2] + H[2][1]) + ((H[0][1] * H[0][2] + H[1][1] * H[1][2]) + H[2][1] * H[2][2]));
        Ed[5] = 0.5 * ((H[0][2] + H[2][0]) + ((H[0][0] * H[0][2] + H[1][0] * H[1][2]) + H[2][0] * H[2][2]));
        const double trE = (Ed[0] + Ed[1]) + Ed[2];
        const double Sm[3][3] = {{lam * trE + 2.0 * mu * Ed[0], 2.0 * mu * Ed[3], 2.0 * mu * Ed[5]},
                                 {2.0 * mu * Ed[3], lam * trE + 2.0 * mu * Ed[1], 2.0 * mu * Ed[4]},
                                 {2.0 * mu * Ed[5], 2.0 * mu * Ed[4], lam * trE + 2.0 * mu * Ed[2]}};
        W = 0.5 * lam * trE * trE + mu * (((Ed[0] * Ed[0] + Ed[1] * Ed[1]) + Ed[2] * Ed[2]) +
                                          2.0 * ((Ed[3] * Ed[3] + Ed[4] * Ed[4]) + Ed[5] * Ed[5]));
        double Sg[4][3];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int i = 0; i < 3; ++i) Sg[a][i] = (Sm[i][0] * g[a][0] + Sm[i][1] * g[a][1]) + Sm[i][2] * g[a][2];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int i = 0; i < 3; ++i)
                r[FE0 + 3 * a + i] = V * ((F[i][0] * Sg[a][0] + F[i][1] * Sg[a][1]) + F[i][2] * Sg[a][2]);
        double FFt[6];
        FFt[0] = (F[0][0] * F[0][0] + F[0][1] * F[0][1]) + F[0][2] * F[0][2];
        FFt[1] = (F[1][0] * F[1][0] + F[1][1] * F[1][1]) + F[1][2] * F[1][2];
        FFt[2] = (F[2][0] * F[2][0] + F[2][1] * F[2][1]) + F[2][2] * F[2][2];
        FFt[3] = (F[0][0] * F[1][0] + F[0][1] * F[1][1]) + F[0][2] * F[1][2];
        FFt[4] = (F[1][0] * F[2][0] + F[1][1] * F[2][1]) + F[1][2] * F[2][2];
        FFt[5] = (F[0][0] * F[2][0] + F[0][1] * F[2][1]) + F[0][2] * F[2][2];
        if (TAN) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = a; b < 4; ++b)
                    r[NL_C + sym_blk(4, a, b)] = (g[a][0] * Sg[b][0] + g[a][1] * Sg[b][1]) + g[a][2] * Sg[b][2];
#pragma unroll
            for (int t = 0; t < 6; ++t) r[NL_FF + t] = FFt[t];
            r[NL_COEF] = 0.0;
        }
        if (sigma) {   // J^-1 F S F^T
            double FS[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) FS[i][j] = (F[i][0] * Sm[0][j] + F[i][1] * Sm[1][j]) + F[i][2] * Sm[2][j];
            sg[0] = iJ * ((FS[0][0] * F[0][0] + FS[0][1] * F[0][1]) + FS[0][2] * F[0][2]);
            sg[1] = iJ * ((FS[1][0] * F[1][0] + FS[1][1] * F[1][1]) + FS[1][2] * F[1][2]);
            sg[2] = iJ * ((FS[2][0] * F[2][0] + FS[2][1] * F[2][1]) + FS[2][2] * F[2][2]);
            sg[3] = iJ * ((FS[0][0] * F[1][0] + FS[0][1] * F[1][1]) + FS[0][2] * F[1][2]);
            sg[4] = iJ * ((FS[1][0] * F[2][0] + FS[1][1] * F[2][1]) + FS[1][2] * F[2][2]);
            sg[5] = iJ * ((FS[0][0] * F[2][0] + FS[0][1] * F[2][1]) + FS[0][2] * F[2][2]);
        }
        if (TAN) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int i = 0; i < 3; ++i) r[NL_X + 3 * a + i] = Fg[a][i];
        }
    } else {
        Cf[1][0] = dop(F[0][2], F[2][1], F[0][1], F[2][2]);
        Cf[1][1] = dop(F[0][0], F[2][2], F[0][2], F[2][0]);
        Cf[1][2] = dop(F[0][1], F[2][0], F[0][0], F[2][1]);
        Cf[2][0] = dop(F[0][1], F[1][2], F[0][2], F[1][1]);
        Cf[2][1] = dop(F[0][2], F[1][0], F[0][0], F[1][2]);
        Cf[2][2] = dop(F[0][0], F[1][1], F[0][1], F[1][0]);
        const double lnJ = log(J);
        // h_a = F^-T g_a = (cofactor matrix) g_a / J
        double h[4][3];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int i = 0; i < 3; ++i) h[a][i] = iJ * ((Cf[i][0] * g[a][0] + Cf[i][1] * g[a][1]) + Cf[i][2] * g[a][2]);
        const double ll = lam * lnJ;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int i = 0; i < 3; ++i) r[FE0 + 3 * a + i] = V * (mu * (Fg[a][i] - h[a][i]) + ll * h[a][i]);
        // F:F - 3 = 2 tr H + H:H
        double hh = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) hh += H[i][j] * H[i][j];
        const double ff3 = 2.0 * ((H[0][0] + H[1][1]) + H[2][2]) + hh;
        W = (0.5 * mu * ff3 - mu * lnJ) + 0.5 * lam * lnJ * lnJ;
        if (sigma) {   // J^-1 (mu (F F^T - I) + lam ln J I), F F^T - I = H + H^T + H H^T
            const double b0 = 2.0 * H[0][0] + ((H[0][0] * H[0][0] + H[0][1] * H[0][1]) + H[0][2] * H[0][2]);
            const double b1 = 2.0 * H[1][1] + ((H[1][0] * H[1][0] + H[1][1] * H[1][1]) + H[1][2] * H[1][2]);
            const double b2 = 2.0 * H[2][2] + ((H[2][0] * H[2][0] + H[2][1] * H[2][1]) + H[2][2] * H[2][2]);
            const double b3 = (H[0][1] + H[1][0]) + ((H[0][0] * H[1][0] + H[0][1] * H[1][1]) + H[0][2] * H[1][2]);
            const double b4 = (H[1][2] + H[2][1]) + ((H[1][0] * H[2][0] + H[1][1] * H[2][1]) + H[1][2] * H[2][2]);
            const double b5 = (H[0][2] + H[2][0]) + ((H[0][0] * H[2][0] + H[0][1] * H[2][1]) + H[0][2] * H[2][2]);
            sg[0] = iJ * (mu * b0 + ll);
            sg[1] = iJ * (mu * b1 + ll);
            sg[2] = iJ * (mu * b2 + ll);
            sg[3] = iJ * (mu * b3);
            sg[4] = iJ * (mu * b4);
            sg[5] = iJ * (mu * b5);
        }
        if (TAN) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int i = 0; i < 3; ++i) r[NL_X + 3 * a + i] = h[a][i];
#pragma unroll
            for (int t = 0; t < 6; ++t) r[NL_FF + t] = 0.0;
            r[NL_COEF] = mu - ll;
        }
    }
    if (TAN) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = a; b < 4; ++b) {
                const double gg = (g[a][0] * g[b][0] + g[a][1] * g[b][1]) + g[a][2] * g[b][2];
                r[NL_GG + sym_blk(4, a, b)] = gg;
                if (MAT != FEM_MAT_SVK) r[NL_C + sym_blk(4, a, b)] = mu * gg;
            }
        r[NL_V] = V;
    }
    if (we) we[e] = V * W;
    if (sigma) {
#pragma unroll
        for (int t = 0; t < 6; ++t) sigma[6 * e + t] = sg[t];
    }
}

// 64 elements per 256-thread block: 64 lanes form the records into LDS, then all 256 threads write them out through
// the c3d4 tangent shell of element.hpp. TAN = false (Kt == NULL, the line search's trial evaluations) has no tangent
// record and no tangent store. PACKED: fem_iso_ke_sym's layout for npe = 4 (90 doubles per element), else the full
// [12, 12].
template <int MAT, bool TAN, bool PACKED>
__global__ void __launch_bounds__(256) k_tet4_nl(const double* __restrict__ X, const int64_t* __restrict__ conn,
                                                 int64_t M, const double* __restrict__ U, double E, double nu,
                                                 double* __restrict__ Kt, double* __restrict__ fe,
                                                 double* __restrict__ we, double* __restrict__ sigma,
                                                 double* __restrict__ detF, int64_t* __restrict__ bad,
                                                 int64_t* __restrict__ inverted) {
    constexpr int REC = TAN ? NL_REC_T : NL_REC_F;
    constexpr int FE0 = TAN ? NL_TAN : 0;
    __shared__ double rec_s[64 * REC];
    const Lame L = lame(E, nu);
    const int64_t e0 = (int64_t)blockIdx.x * 64;
    if (threadIdx.x < 64) {
        const int64_t e = e0 + threadIdx.x;
        if (e < M)
            nl_element<MAT, TAN>(X, conn, e, U, L.lam, L.mu, rec_s + threadIdx.x * REC, we, sigma, detF, bad, inverted);
    }
    __syncthreads();
    const int nel = (int)min((int64_t)64, M - e0);
    if (TAN)
        tet4_tangent_store<REC, PACKED>(rec_s, e0, nel, Kt, [&](const double* r, int a, int b, int i, int k) {
            return nl_entry<MAT>(r, a, b, i, k, L.lam, L.mu);
        });
    if (fe) tet4_force_store<REC, FE0>(rec_s, e0, nel, fe);
}

// one thread per node dof: the node's incidence list in ascending (element, local) order (k_ebe_apply's order), so
// fint is the same bits on every run and no atomics are used
__global__ void __launch_bounds__(256) k_tet4_nl_gather(const double* __restrict__ fe,
                                                        const int32_t* __restrict__ inc_ptr,
                                                        const int32_t* __restrict__ inc, int64_t N,
                                                        const double* __restrict__ fext, double load_factor,
                                                        const uint8_t* __restrict__ mask, double* __restrict__ fint,
                                                        double* __restrict__ r) {
    const int64_t n3 = 3 * N;
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n3; d += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = d / 3;
        const int c = (int)(d - 3 * i);
        double acc = 0.0;
        for (int t = inc_ptr[i]; t < inc_ptr[i + 1]; ++t) acc += fe[(int64_t)inc[t] * 3 + c];
        if (fint) fint[d] = acc;
        if (r) r[d] = (mask && mask[d]) ? 0.0 : load_factor * fext[d] - acc;
    }
}

}  // namespace fem

using namespace fem;

extern "C" {

int fem_tet4_nl(const double* coords, const int64_t* conn, int64_t M, const double* u, double E, double nu,
                int material, int packed, double* Kt, double* fe, double* we, double* sigma, double* detF,
                int64_t* bad_idx, int64_t* inverted_idx, fem_stream_t stream) {
    if (material != FEM_MAT_SVK && material != FEM_MAT_NEO_HOOKEAN) {
        set_error("fem_tet4_nl: unknown material %d", material);
        return FEM_EARG;
    }
    if (M <= 0) return FEM_OK;
    if (!bad_idx || !inverted_idx) {
        set_error("fem_tet4_nl: bad_idx and inverted_idx are required");
        return FEM_EARG;
    }
    const dim3 g((unsigned)cdiv(M, 64));
#define FEM_NL(MAT_, TAN_, PK_)                                                                                        \
    hipLaunchKernelGGL((k_tet4_nl<MAT_, TAN_, PK_>), g, dim3(256), 0, S(stream), coords, conn, M, u, E, nu, Kt, fe, we, \
                       sigma, detF, bad_idx, inverted_idx)
    if (material == FEM_MAT_SVK) {
        if (!Kt) FEM_NL(FEM_MAT_SVK, false, false);
        else if (packed) FEM_NL(FEM_MAT_SVK, true, true);
        else FEM_NL(FEM_MAT_SVK, true, false);
    } else {
        if (!Kt) FEM_NL(FEM_MAT_NEO_HOOKEAN, false, false);
        else if (packed) FEM_NL(FEM_MAT_NEO_HOOKEAN, true, true);
        else FEM_NL(FEM_MAT_NEO_HOOKEAN, true, false);
    }
#undef FEM_NL
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_tet4_nl_gather(const double* fe, const int32_t* inc_ptr, const int32_t* inc, int64_t N, const double* fext,
                       double load_factor, const uint8_t* mask, double* fint, double* r, fem_stream_t stream) {
    if (N <= 0) return FEM_OK;
    if (r && !fext) {
        set_error("fem_tet4_nl_gather: the residual needs fext");
        return FEM_EARG;
    }
    hipLaunchKernelGGL(k_tet4_nl_gather, dim3(stream_grid(3 * N, 256)), dim3(256), 0, S(stream), fe, inc_ptr, inc, N,
                       fext, load_factor, mask, fint, r);
    FEM_LAUNCHED();
    return FEM_OK;
}

}  // extern "C"
