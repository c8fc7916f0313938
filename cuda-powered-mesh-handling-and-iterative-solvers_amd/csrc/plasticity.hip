// Small-strain J2 (von Mises) plasticity with linear isotropic hardening on c3d4 for gfx950: per tet the radial-return
// stress update from the committed state (plastic strain ep_n, accumulated plastic strain alpha_n), the internal force,
// the consistent (algorithmic) tangent, the incremental potential and the trial state.
//
// With the gradients g_a and volume V of tet4_grads (element.hpp), eps = sym(sum_a u_a (x) g_a), mu = E / (2 (1 + nu)),
// kappa = E / (3 (1 - 2 nu)); all tensors as (xx, yy, zz, xy, yz, xz) tensor components (no engineering factor):
//   e = dev eps, s_tr = 2 mu (e - ep_n), q_tr = sqrt(3/2) |s_tr|, f_tr = q_tr - (sigma_y + H alpha_n)
//   f_tr <= 0: s = s_tr, the state is kept, C = kappa 1(x)1 + 2 mu P_dev
//   f_tr >  0: dgamma = f_tr / (3 mu + H), n = s_tr / |s_tr|, beta = 1 - 3 mu dgamma / q_tr, s = beta s_tr,
//              ep_n+1 = ep_n + sqrt(3/2) dgamma n, alpha_n+1 = alpha_n + dgamma,
//              C = kappa 1(x)1 + 2 mu beta P_dev - 2 mu (3 mu / (3 mu + H) - (1 - beta)) n(x)n
//   sigma = kappa tr(eps) 1 + s, force on node a: V sigma g_a, tangent V B^T C B:
//     block (a,b)(i,k) / V = (kappa - 2 mu beta / 3) g_a,i g_b,k + mu beta ((g_a.g_b) d_ik + g_b,i g_a,k)
//                            - c_n (n g_a)_i (n g_b)_k
//   we = V [kappa/2 tr(eps)^2 + mu |e - ep_n+1|^2 + H/2 alpha_n+1^2 + sigma_y dgamma], d we / d u = the element force
//   while the committed state is fixed.
#include <math.h>

#include "common.hpp"
#include "element.hpp"

namespace fem {

// per-element record in LDS (doubles): what the block formula reads, then the element forces
constexpr int J2_G = 0;      // [4][3] g_a
constexpr int J2_NG = 12;    // [4][3] n g_a (0 for an elastic element)
constexpr int J2_GG = 24;    // [10] g_a.g_b, a <= b, at sym_blk(4, a, b)
constexpr int J2_CL = 34;    // kappa - 2 mu beta / 3
constexpr int J2_CM = 35;    // mu beta
constexpr int J2_CN = 36;    // the n(x)n factor (0 for an elastic element)
constexpr int J2_V = 37;     // V (0 for an element whose outputs are zero)
constexpr int J2_TAN = 38;   // record length of the tangent part
constexpr int J2_REC_T = 51;   // tangent part + 12 forces, padded to an odd stride
constexpr int J2_REC_F = 13;   // forces only

// entry (i, k) of the upper block (a, b), a <= b, from the element's record. The packed and the full form both come
// through here with the same arguments (the full form's lower blocks with (a, i) and (b, k) exchanged), and no product
// is fused into a sum, so the two agree bit for bit and the full matrix is exactly symmetric.
__device__ __forceinline__ double j2_entry(const double* __restrict__ r, int a, int b, int i, int k) {
#pragma clang fp contract(off)
    const double* ga = r + J2_G + 3 * a;
    const double* gb = r + J2_G + 3 * b;
    const double p = ga[i] * gb[k];
    const double q = gb[i] * ga[k];
    const double m = r[J2_NG + 3 * a + i] * r[J2_NG + 3 * b + k];
    double s = r[J2_CL] * p + r[J2_CM] * q;
    if (i == k) s = s + r[J2_CM] * r[J2_GG + sym_blk(4, a, b)];
    s = s - r[J2_CN] * m;
    return s * r[J2_V];
}

// One lane: everything of element e that does not depend on the output entry, into the record r and the per-element
// outputs. ep_in / alpha_in are read before ep_out / alpha_out are written and only at slot e, so the outputs may alias
// the inputs. A degenerate reference element gets a zero record, zero stress and energy and its input state copied
// through. Products are not fused into sums, so the TAN = false build gives every output of the TAN = true build bit
// for bit.
template <bool TAN>
__device__ __forceinline__ void j2_element(const double* __restrict__ X, const int64_t* __restrict__ conn, int64_t e,
                                           const double* __restrict__ U, double kappa, double mu, double sy, double Hh,
                                           const double* ep_in, const double* alpha_in, double* __restrict__ r,
                                           double* __restrict__ we, double* __restrict__ sigma, double* ep_out,
                                           double* alpha_out, uint8_t* __restrict__ plastic,
                                           int64_t* __restrict__ bad) {
#pragma clang fp contract(off)
    constexpr int FE0 = TAN ? J2_TAN : 0;
    const int64_t nd[4] = {conn[4 * e], conn[4 * e + 1], conn[4 * e + 2], conn[4 * e + 3]};
    double g[4][3];
    const double det = tet4_grads_n(X, nd, g);
    const bool degenerate = !(fabs(det) >= 1e-12);
    double ep[6] = {0, 0, 0, 0, 0, 0};
    double al = 0.0;
    if (ep_in) {
#pragma unroll
        for (int t = 0; t < 6; ++t) ep[t] = ep_in[6 * e + t];
        al = alpha_in[e];
    }
    if (degenerate) {
        if (bad) atomicMin((unsigned long long*)bad, (unsigned long long)e);
#pragma unroll
        for (int t = 0; t < FE0 + 12; ++t) r[t] = 0.0;
        if (we) we[e] = 0.0;
        if (sigma) {
#pragma unroll
            for (int t = 0; t < 6; ++t) sigma[6 * e + t] = 0.0;
        }
        if (ep_out) {
#pragma unroll
            for (int t = 0; t < 6; ++t) ep_out[6 * e + t] = ep[t];
        }
        if (alpha_out) alpha_out[e] = al;
        if (plastic) plastic[e] = 0;
        return;
    }
    const double V = fabs(det) / 6.0;
    double u[4][3], Hm[3][3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) u[a][k] = U[3 * nd[a] + k];
    tet4_disp_grad(u, g, Hm);
    const double tr = (Hm[0][0] + Hm[1][1]) + Hm[2][2];
    const double tm = tr / 3.0;
    // deviatoric strain minus the committed plastic strain, then the trial stress deviator
    double d[6];
    d[0] = (Hm[0][0] - tm) - ep[0];
    d[1] = (Hm[1][1] - tm) - ep[1];
    d[2] = (Hm[2][2] - tm) - ep[2];
    d[3] = 0.5 * (Hm[0][1] + Hm[1][0]) - ep[3];
    d[4] = 0.5 * (Hm[1][2] + Hm[2][1]) - ep[4];
    d[5] = 0.5 * (Hm[0][2] + Hm[2][0]) - ep[5];
    double s[6];
#pragma unroll
    for (int t = 0; t < 6; ++t) s[t] = 2.0 * mu * d[t];
    const double sn = sqrt(((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]) +
                           2.0 * ((s[3] * s[3] + s[4] * s[4]) + s[5] * s[5]));
    const double r32 = sqrt(1.5);
    const double q = r32 * sn;
    const double f = q - (sy + Hh * al);
    const bool yields = f > 0.0;
    double nn[6] = {0, 0, 0, 0, 0, 0};
    double beta = 1.0, cn = 0.0, dg = 0.0;
    if (yields) {
        dg = f / (3.0 * mu + Hh);
        beta = 1.0 - 3.0 * mu * dg / q;
        cn = 2.0 * mu * (3.0 * mu / (3.0 * mu + Hh) - (1.0 - beta));
        const double c = r32 * dg;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            nn[t] = s[t] / sn;
            s[t] = beta * s[t];
            ep[t] = ep[t] + c * nn[t];
        }
        al = al + dg;
    }
    const double p = kappa * tr;
    const double sg[6] = {p + s[0], p + s[1], p + s[2], s[3], s[4], s[5]};
    const double Sm[3][3] = {{sg[0], sg[3], sg[5]}, {sg[3], sg[1], sg[4]}, {sg[5], sg[4], sg[2]}};
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int i = 0; i < 3; ++i)
            r[FE0 + 3 * a + i] = V * ((Sm[i][0] * g[a][0] + Sm[i][1] * g[a][1]) + Sm[i][2] * g[a][2]);
    if (TAN) {
        const double Nm[3][3] = {{nn[0], nn[3], nn[5]}, {nn[3], nn[1], nn[4]}, {nn[5], nn[4], nn[2]}};
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                r[J2_G + 3 * a + i] = g[a][i];
                r[J2_NG + 3 * a + i] = (Nm[i][0] * g[a][0] + Nm[i][1] * g[a][1]) + Nm[i][2] * g[a][2];
            }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = a; b < 4; ++b)
                r[J2_GG + sym_blk(4, a, b)] = (g[a][0] * g[b][0] + g[a][1] * g[b][1]) + g[a][2] * g[b][2];
        r[J2_CL] = kappa - 2.0 * mu * beta / 3.0;
        r[J2_CM] = mu * beta;
        r[J2_CN] = cn;
        r[J2_V] = V;
    }
    if (we) {
        // e - ep_n+1 = (e - ep_n) - sqrt(3/2) dgamma n
        double dd = 0.0, ds = 0.0;
        const double c = r32 * dg;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const double x = d[t] - c * nn[t];
            if (t < 3) dd += x * x;
            else ds += x * x;
        }
        we[e] = V * (((0.5 * kappa * tr * tr + mu * (dd + 2.0 * ds)) + 0.5 * Hh * al * al) + sy * dg);
    }
    if (sigma) {
#pragma unroll
        for (int t = 0; t < 6; ++t) sigma[6 * e + t] = sg[t];
    }
    if (ep_out) {
#pragma unroll
        for (int t = 0; t < 6; ++t) ep_out[6 * e + t] = ep[t];
    }
    if (alpha_out) alpha_out[e] = al;
    if (plastic) plastic[e] = yields ? 1 : 0;
}

// 64 elements per 256-thread block: 64 lanes form the records into LDS, then all 256 threads write them out through
// the c3d4 tangent shell of element.hpp. TAN = false (Kt == NULL, the line search's trial evaluations) has no tangent
// record and no tangent store. PACKED: fem_iso_ke_sym's layout for npe = 4 (90 doubles per element), else the full
// [12, 12].
template <bool TAN, bool PACKED>
__global__ void __launch_bounds__(256) k_tet4_j2(const double* __restrict__ X, const int64_t* __restrict__ conn,
                                                 int64_t M, const double* __restrict__ U, double kappa, double mu,
                                                 double sy, double Hh, const double* ep_in, const double* alpha_in,
                                                 double* __restrict__ Kt, double* __restrict__ fe,
                                                 double* __restrict__ we, double* __restrict__ sigma, double* ep_out,
                                                 double* alpha_out, uint8_t* __restrict__ plastic,
                                                 int64_t* __restrict__ bad) {
    constexpr int REC = TAN ? J2_REC_T : J2_REC_F;
    constexpr int FE0 = TAN ? J2_TAN : 0;
    __shared__ double rec_s[64 * REC];
    const int64_t e0 = (int64_t)blockIdx.x * 64;
    if (threadIdx.x < 64) {
        const int64_t e = e0 + threadIdx.x;
        if (e < M)
            j2_element<TAN>(X, conn, e, U, kappa, mu, sy, Hh, ep_in, alpha_in, rec_s + threadIdx.x * REC, we, sigma,
                            ep_out, alpha_out, plastic, bad);
    }
    __syncthreads();
    const int nel = (int)min((int64_t)64, M - e0);
    if (TAN) tet4_tangent_store<REC, PACKED>(rec_s, e0, nel, Kt, j2_entry);
    if (fe) tet4_force_store<REC, FE0>(rec_s, e0, nel, fe);
}

}  // namespace fem

using namespace fem;

extern "C" {

int fem_tet4_j2(const double* coords, const int64_t* conn, int64_t M, const double* u, double E, double nu,
                double sigma_y, double H, const double* ep_in, const double* alpha_in, int packed, double* Kt,
                double* fe, double* we, double* sigma, double* ep_out, double* alpha_out, uint8_t* plastic,
                int64_t* bad_idx, fem_stream_t stream) {
    if (!(sigma_y > 0.0)) {
        set_error("fem_tet4_j2: sigma_y must be > 0, got %g", sigma_y);
        return FEM_EARG;
    }
    if (!(H >= 0.0)) {
        set_error("fem_tet4_j2: H must be >= 0, got %g", H);
        return FEM_EARG;
    }
    if (!(nu > -1.0 && nu < 0.5)) {
        set_error("fem_tet4_j2: nu must lie in (-1, 0.5), got %g", nu);
        return FEM_EARG;
    }
    if ((ep_in == nullptr) != (alpha_in == nullptr)) {
        set_error("fem_tet4_j2: ep_in and alpha_in are given together or both NULL (the virgin state)");
        return FEM_EARG;
    }
    if (M <= 0) return FEM_OK;
    const double mu = E / (2.0 * (1.0 + nu));
    const double kappa = E / (3.0 * (1.0 - 2.0 * nu));
    const dim3 g((unsigned)cdiv(M, 64));
#define FEM_J2(TAN_, PK_)                                                                                              \
    hipLaunchKernelGGL((k_tet4_j2<TAN_, PK_>), g, dim3(256), 0, S(stream), coords, conn, M, u, kappa, mu, sigma_y, H,  \
                       ep_in, alpha_in, Kt, fe, we, sigma, ep_out, alpha_out, plastic, bad_idx)
    if (!Kt) FEM_J2(false, false);
    else if (packed) FEM_J2(true, true);
    else FEM_J2(true, false);
#undef FEM_J2
    FEM_LAUNCHED();
    return FEM_OK;
}

}  // extern "C"
