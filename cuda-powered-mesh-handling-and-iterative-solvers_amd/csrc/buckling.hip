// Geometric (initial-stress) stiffness of the solid elements (linear buckling) on gfx950.
//
// K_g,e = Gs_e (x) I3 with the scalar factor
//   Gs_e[a][b] = sum_q w_q |detJ_q| grad N_a(q)^T sigma_q grad N_b(q),
// sigma_q = D(E, nu) B_q u_e (+ a per-element constant sigma0_e). The reference project has no buckling analysis:
// the formulas are the classical initial-stress matrix, the quadrature tables are element.py's.
//
// One THREAD forms an element, as k_iso_mass_s (assemble.hip) does for the scalar mass: the only per-point data are the
// 3x3 Jacobian, the 3x3 natural displacement gradient and a symmetric 3x3 tensor. With g_a = J^-1 dN_a,
//   g_a^T sigma g_b = dN_a^T (J^-T sigma J^-1) dN_b = dN_a^T T dN_b,
// so the global gradients are never stored: per point the thread forms T (scaled by w_q |detJ_q|) and takes the
// NPE (NPE + 1) / 2 upper-triangle forms against the natural derivative table in LDS (every lane reads the same
// address: a broadcast). The stress is formed in registers at the very points that integrate Gs. A wave per element
// would hand J, detJ and sigma from lane to lane at every point, which is what made the wave form of the scalar mass
// slower than the thread form. The block is written as the full symmetric NPE x NPE matrix from the upper triangle
// (bit-symmetric) in 16-byte stores over the element's contiguous 8 NPE^2 bytes. No atomics: a degenerate element sets
// its own byte of `bad`.
#include <algorithm>

#include "element.hpp"

namespace fem {

template <int NPE, bool HAS_U>
__global__ void __launch_bounds__(256) k_geo_s(const double* __restrict__ X, const int64_t* __restrict__ conn,
                                               int64_t M, const double* __restrict__ U, Lame L,
                                               const double* __restrict__ S0, const double* __restrict__ dN,
                                               const double* __restrict__ w, int n_ip, double* __restrict__ Gs,
                                               uint8_t* __restrict__ bad) {
    __shared__ double dn_s[ISO_MAX_IP * NPE * 3];
    __shared__ double w_s[ISO_MAX_IP];
    for (int t = threadIdx.x; t < n_ip * NPE * 3; t += 256) dn_s[t] = dN[t];
    for (int t = threadIdx.x; t < n_ip; t += 256) w_s[t] = w[t];
    __syncthreads();
    constexpr int NS = NPE * (NPE + 1) / 2;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < M; e += (int64_t)gridDim.x * 256) {
        double x[NPE][3], u[HAS_U ? NPE : 1][3];
#pragma unroll
        for (int j = 0; j < NPE; ++j) {
            const int64_t c = conn[e * NPE + j];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                x[j][k] = X[3 * c + k];
                if (HAS_U) u[HAS_U ? j : 0][k] = U[3 * c + k];
            }
        }
        // Voigt (xx, yy, zz, xy, yz, xz) of the element's constant prestress: the upper triangle of sigma0[e]
        double s0[6] = {0, 0, 0, 0, 0, 0};
        if (S0) {
            const double* s = S0 + 9 * e;
            s0[0] = s[0];
            s0[1] = s[4];
            s0[2] = s[8];
            s0[3] = s[1];
            s0[4] = s[5];
            s0[5] = s[2];
        }
        double m[NS];
#pragma unroll
        for (int t = 0; t < NS; ++t) m[t] = 0.0;
        bool degenerate = false;
#pragma unroll 1
        for (int q = 0; q < n_ip; ++q) {
            const double* dq = dn_s + q * NPE * 3;
            // J[i][k] = sum_j dN[j][i] x_j[k] (node j ascending, as k_iso_mass_s); H[c][i] = sum_j u_j[c] dN[j][i]
            double J[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < NPE; ++j) {
                const double d[3] = {dq[j * 3], dq[j * 3 + 1], dq[j * 3 + 2]};
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        J[3 * i + k] += d[i] * x[j][k];
                        if (HAS_U) H[3 * k + i] += u[HAS_U ? j : 0][k] * d[i];
                    }
            }
            double Ji[9];
            const double det = inv3(J, Ji);
            if (!(fabs(det) > 0.0) || !(fabs(det) < INFINITY)) degenerate = true;   // 0, NaN or Inf
            double s[6] = {s0[0], s0[1], s0[2], s0[3], s0[4], s0[5]};
            if (HAS_U) {
                // du_c / dx_k = sum_l H[c][l] Ji[k][l]
                double G[9];
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        G[3 * c + k] = H[3 * c] * Ji[3 * k] + H[3 * c + 1] * Ji[3 * k + 1] + H[3 * c + 2] * Ji[3 * k + 2];
                const double tr = L.lam * (G[0] + G[4] + G[8]);
                s[0] += tr + 2.0 * L.mu * G[0];
                s[1] += tr + 2.0 * L.mu * G[4];
                s[2] += tr + 2.0 * L.mu * G[8];
                s[3] += L.mu * (G[1] + G[3]);
                s[4] += L.mu * (G[5] + G[7]);
                s[5] += L.mu * (G[2] + G[6]);
            }
            // T = c_q Ji^T sigma Ji (symmetric; the upper triangle is formed): A = sigma Ji, T[l][n] = sum_i Ji[i][l] A[i][n]
            const double sg[9] = {s[0], s[3], s[5], s[3], s[1], s[4], s[5], s[4], s[2]};
            double A[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int n = 0; n < 3; ++n)
                    A[3 * i + n] = sg[3 * i] * Ji[n] + sg[3 * i + 1] * Ji[3 + n] + sg[3 * i + 2] * Ji[6 + n];
            const double cq = fabs(det) * w_s[q];
            double T[9];
#pragma unroll
            for (int l = 0; l < 3; ++l)
#pragma unroll
                for (int n = l; n < 3; ++n) {
                    T[3 * l + n] = (Ji[l] * A[n] + Ji[3 + l] * A[3 + n] + Ji[6 + l] * A[6 + n]) * cq;
                    T[3 * n + l] = T[3 * l + n];
                }
#pragma unroll
            for (int b = 0; b < NPE; ++b) {
                const double d[3] = {dq[b * 3], dq[b * 3 + 1], dq[b * 3 + 2]};
                const double t0 = T[0] * d[0] + T[1] * d[1] + T[2] * d[2];
                const double t1 = T[3] * d[0] + T[4] * d[1] + T[5] * d[2];
                const double t2 = T[6] * d[0] + T[7] * d[1] + T[8] * d[2];
#pragma unroll
                for (int a = 0; a <= b; ++a)
                    m[sym_blk(NPE, a, b)] += dq[a * 3] * t0 + dq[a * 3 + 1] * t1 + dq[a * 3 + 2] * t2;
            }
        }
        if (degenerate) bad[e] = 1;
        double2* out = reinterpret_cast<double2*>(Gs + e * NPE * NPE);   // NPE^2 even: 16-byte aligned blocks
#pragma unroll
        for (int p = 0; p < NPE * NPE / 2; ++p) {
            double v2[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int i = 2 * p + h, a = i / NPE, b = i - NPE * (i / NPE);
                const int lo = a < b ? a : b, hi = a < b ? b : a;
                v2[h] = m[sym_blk(NPE, lo, hi)];
            }
            out[p] = make_double2(v2[0], v2[1]);
        }
    }
}

template <int NPE>
static void geo_launch(const double* coords, const int64_t* conn, int64_t M, const double* u, Lame L,
                       const double* sigma0, const double* dN, const double* w, int n_ip, double* Gs, uint8_t* bad,
                       hipStream_t st) {
    const dim3 g((unsigned)std::min<int64_t>(cdiv(M, 256), 65536));
    if (u)
        hipLaunchKernelGGL((k_geo_s<NPE, true>), g, dim3(256), 0, st, coords, conn, M, u, L, sigma0, dN, w, n_ip, Gs, bad);
    else
        hipLaunchKernelGGL((k_geo_s<NPE, false>), g, dim3(256), 0, st, coords, conn, M, u, L, sigma0, dN, w, n_ip, Gs, bad);
}

}  // namespace fem

using namespace fem;

extern "C" {

int fem_geo_scalar(const double* coords, const int64_t* conn, int64_t M, int npe, const double* u, double E, double nu,
                   const double* sigma0, const double* dN, const double* w, int n_ip, double* Gs, uint8_t* bad,
                   fem_stream_t stream) {
    if (!u && !sigma0) {
        set_error("fem_geo_scalar: a displacement, a prestress or both are needed");
        return FEM_EARG;
    }
    if (M > 0 && (!coords || !conn || !dN || !w || !Gs || !bad)) {
        set_error("fem_geo_scalar: coords, conn, dN, w, Gs and bad may not be NULL");
        return FEM_EARG;
    }
    if (n_ip < 1 || n_ip > ISO_MAX_IP) {
        set_error("fem_geo_scalar: n_ip = %d out of range [1, %d]", n_ip, ISO_MAX_IP);
        return FEM_EARG;
    }
    if (npe != 4 && npe != 6 && npe != 8 && npe != 10) {
        set_error("fem_geo_scalar: unsupported nodes per element %d (4, 6, 8, 10)", npe);
        return FEM_EBADTYPE;
    }
    if (M <= 0) return FEM_OK;
    const Lame L = u ? lame(E, nu) : Lame{0.0, 0.0};
    switch (npe) {
        case 4: geo_launch<4>(coords, conn, M, u, L, sigma0, dN, w, n_ip, Gs, bad, S(stream)); break;
        case 6: geo_launch<6>(coords, conn, M, u, L, sigma0, dN, w, n_ip, Gs, bad, S(stream)); break;
        case 8: geo_launch<8>(coords, conn, M, u, L, sigma0, dN, w, n_ip, Gs, bad, S(stream)); break;
        default: geo_launch<10>(coords, conn, M, u, L, sigma0, dN, w, n_ip, Gs, bad, S(stream)); break;
    }
    FEM_LAUNCHED();
    return FEM_OK;
}

}  // extern "C"
