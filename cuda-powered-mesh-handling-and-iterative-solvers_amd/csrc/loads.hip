// Distributed loads on gfx950: body force, thermal strain and surface pressure / traction turned into nodal forces
// (the stress recovery that subtracts the thermal strain is stress.hip's). No reference function exists for
// any of them (the reference's solvers take a finished force array): the formulas are the consistent ones for the
// element matrices this library already forms.
//
//   body     f_a = rho int N_a a dV          c3d4: rho V/4 g, or rho V/20 (a_a + sum_b a_b) for a nodal field
//                                            c3d8 / c3d6 / c3d10: rho sum_q w_q |detJ_q| N_a(q) a(q)
//   thermal  f_a = int B_a^T D (alpha dT m)  m = (1,1,1,0,0,0); D m = (D00 + 2 D01) m, so f_a = c (D00 + 2 D01)
//                                            alpha dT grad N_a with the volume factor c of the family's K_e
//   surface  f_a = -int N_a p n dA  or  int N_a t dA   over tri3 (one point) / quad4 (2x2 Gauss on x_xi x x_eta)
//
// Every nodal sum is a gather over the sorted node -> element incidence in ascending order: no atomics, the same bits
// on every run, zero rows for nodes without elements. All arithmetic fp64.
#include "element.hpp"

namespace fem {

// (D alpha m)'s normal entry: the thermal load per unit dT and unit gradient
static inline double thermal_beta(double E, double nu, double alpha) {
    const Dmat D = dmat(E, nu);
    return (D.d0 + D.d1 + D.d1) * alpha;
}

// ---------------------------------------------------------------- c3d4 volume loads
struct Tet4LoadArgs {
    const double* X;
    const int64_t* conn;
    double rho;
    const double* accel;   // [3] (FEM_LOAD_UNIFORM) or [N,3] (FEM_LOAD_NODAL)
    double beta;           // thermal_beta
    const double* T;       // [1], [N] or [M]
    double Tref;
    int64_t* bad;
};

// element el's scalars: sb the body factor (rho V/4 uniform, rho V/20 nodal), asum = sum_b a_b (nodal), st = V beta
// dT_e, g the gradients. V = |det|/6 (the mass kernel's), g from the signed det (K's): a uniform dT gives K_e times
// the linear expansion field
template <int AM, int TM>
__device__ __forceinline__ void tet4_load_terms(const Tet4LoadArgs& A, int64_t el, const int64_t nd[4],
                                                double g[4][3], double& sb, double asum[3], double& st) {
    const double det = tet4_grads_n(A.X, nd, g);
    if (A.bad && fabs(det) < 1e-12) atomicMin((unsigned long long*)A.bad, (unsigned long long)el);
    const double V = fabs(det) / 6.0;
    sb = 0.0;
    st = 0.0;
    if (AM == FEM_LOAD_UNIFORM) sb = A.rho * V / 4.0;
    if (AM == FEM_LOAD_NODAL) {
        sb = A.rho * V / 20.0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            asum[k] = ((A.accel[3 * nd[0] + k] + A.accel[3 * nd[1] + k]) + A.accel[3 * nd[2] + k]) +
                      A.accel[3 * nd[3] + k];
    }
    if (TM != FEM_LOAD_NONE) {
        double dT;
        if (TM == FEM_LOAD_UNIFORM) dT = A.T[0] - A.Tref;
        else if (TM == FEM_LOAD_ELEMENT) dT = A.T[el] - A.Tref;
        else
            dT = ((((A.T[nd[0]] - A.Tref) + (A.T[nd[1]] - A.Tref)) + (A.T[nd[2]] - A.Tref)) + (A.T[nd[3]] - A.Tref)) /
                 4.0;
        st = V * A.beta * dT;
    }
}

// node-centred form: one thread per node walks its incident tets in ascending incidence order and recomputes each
// one's geometry from coordinates and connectivity (no [M,4,3] intermediate). Body and thermal sums are kept apart
// and added once, so a call with both parts equals the sum of the two separate calls bit for bit. The walk goes in
// chunks of TL_CH entries: their ids, then their connectivity rows, are loaded before any is used, so the dependent
// chain inc -> conn -> coordinates of one tet overlaps the others' (10M tets, gravity: 1.42 ms unchunked, 0.71 ms at
// 4, 0.68 ms at 8).
constexpr int TL_CH = 8;

template <int AM, int TM>
__global__ void __launch_bounds__(256) k_tet4_loads(Tet4LoadArgs A, const int32_t* __restrict__ inc_ptr,
                                                    const int32_t* __restrict__ inc, int64_t N,
                                                    double* __restrict__ F) {
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        double fb[3] = {0.0, 0.0, 0.0}, ft[3] = {0.0, 0.0, 0.0}, an[3] = {0.0, 0.0, 0.0};
        if (AM == FEM_LOAD_UNIFORM)
            for (int k = 0; k < 3; ++k) an[k] = A.accel[k];
        if (AM == FEM_LOAD_NODAL)
            for (int k = 0; k < 3; ++k) an[k] = A.accel[3 * n + k];
        const int b = inc_ptr[n], e = inc_ptr[n + 1];
        for (int t0 = b; t0 < e; t0 += TL_CH) {
            int id[TL_CH];
            int64_t nd[TL_CH][4];
#pragma unroll
            for (int j = 0; j < TL_CH; ++j) id[j] = t0 + j < e ? inc[t0 + j] : -1;
#pragma unroll
            for (int j = 0; j < TL_CH; ++j)
                if (id[j] >= 0) {
                    const int64_t* c = A.conn + 4 * (int64_t)(id[j] >> 2);
#pragma unroll
                    for (int a = 0; a < 4; ++a) nd[j][a] = c[a];
                }
#pragma unroll
            for (int j = 0; j < TL_CH; ++j)
                if (id[j] >= 0) {   // the adds stay in incidence order
                    const int a = id[j] & 3;
                    double g[4][3], sb, st, asum[3] = {0.0, 0.0, 0.0};
                    tet4_load_terms<AM, TM>(A, (int64_t)(id[j] >> 2), nd[j], g, sb, asum, st);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        if (AM == FEM_LOAD_UNIFORM) fb[k] += sb * an[k];
                        if (AM == FEM_LOAD_NODAL) fb[k] += sb * (an[k] + asum[k]);
                        if (TM != FEM_LOAD_NONE) {
                            const double ga = a == 0 ? g[0][k] : a == 1 ? g[1][k] : a == 2 ? g[2][k] : g[3][k];
                            ft[k] += st * ga;
                        }
                    }
                }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) F[3 * n + k] = fb[k] + ft[k];
    }
}

// two-pass form, first pass: element vectors fe [M,4,3] (body + thermal per entry), summed by the incidence gather
template <int AM, int TM>
__global__ void __launch_bounds__(256) k_tet4_loads_elem(Tet4LoadArgs A, int64_t M, double* __restrict__ fe) {
    for (int64_t el = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; el < M; el += (int64_t)gridDim.x * blockDim.x) {
        int64_t nd[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) nd[a] = A.conn[4 * el + a];
        double g[4][3], sb, st, asum[3] = {0.0, 0.0, 0.0};
        tet4_load_terms<AM, TM>(A, el, nd, g, sb, asum, st);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                double fb = 0.0, ft = 0.0;
                if (AM == FEM_LOAD_UNIFORM) fb = sb * A.accel[k];
                if (AM == FEM_LOAD_NODAL) fb = sb * (A.accel[3 * nd[a] + k] + asum[k]);
                if (TM != FEM_LOAD_NONE) ft = st * g[a][k];
                fe[el * 12 + a * 3 + k] = fb + ft;
            }
    }
}

// ---------------------------------------------------------------- isoparametric volume loads (thread per element)
template <int NPE>
__global__ void __launch_bounds__(256) k_iso_loads(const double* __restrict__ X, const int64_t* __restrict__ conn,
                                                   int64_t M, const double* __restrict__ Nv,
                                                   const double* __restrict__ dN, const double* __restrict__ w,
                                                   int n_ip, int mode, double rho, const double* __restrict__ accel,
                                                   int amode, double beta, const double* __restrict__ T, int tmode,
                                                   double Tref, double* __restrict__ fe) {
    __shared__ double dn_s[ISO_MAX_IP * NPE * 3];
    __shared__ double nv_s[ISO_MAX_IP * NPE];
    __shared__ double w_s[ISO_MAX_IP];
    for (int t = threadIdx.x; t < n_ip * NPE * 3; t += blockDim.x) dn_s[t] = dN[t];
    for (int t = threadIdx.x; t < n_ip * NPE; t += blockDim.x) nv_s[t] = Nv[t];
    for (int t = threadIdx.x; t < n_ip; t += blockDim.x) w_s[t] = w[t];
    __syncthreads();
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < M; e += (int64_t)gridDim.x * blockDim.x) {
        int64_t nd[NPE];
        double x[NPE][3], f[NPE][3];
#pragma unroll
        for (int a = 0; a < NPE; ++a) {
            nd[a] = conn[(int64_t)NPE * e + a];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                x[a][k] = X[3 * nd[a] + k];
                f[a][k] = 0.0;
            }
        }
        double vol = 0.0;
        if (NPE == 6 && mode == FEM_ISO_VOLUME) {   // wedge volume: 3 sub-tets (`solver/element.py:2198-2232`)
            constexpr int S[3][4] = {{0, 1, 2, 3}, {1, 2, 4, 3}, {2, 4, 5, 3}};
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                double u[3], v[3], d[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    u[k] = x[S[s][1]][k] - x[S[s][0]][k];
                    v[k] = x[S[s][2]][k] - x[S[s][0]][k];
                    d[k] = x[S[s][3]][k] - x[S[s][0]][k];
                }
                const double cx = u[1] * v[2] - u[2] * v[1], cy = u[2] * v[0] - u[0] * v[2],
                             cz = u[0] * v[1] - u[1] * v[0];
                vol += fabs(cx * d[0] + cy * d[1] + cz * d[2]) / 6.0;
            }
        }
        for (int q = 0; q < n_ip; ++q) {
            const double* dq = dn_s + q * NPE * 3;
            const double* nq = nv_s + q * NPE;
            double J[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // J[i][k] = sum_j dN[j][i] x[j][k]
#pragma unroll
            for (int j = 0; j < NPE; ++j)
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int k = 0; k < 3; ++k) J[3 * i + k] += dq[j * 3 + i] * x[j][k];
            double Ji[9];
            const double det = inv3(J, Ji);
            if (amode != FEM_LOAD_NONE) {
                double aq[3] = {0.0, 0.0, 0.0};
                if (amode == FEM_LOAD_UNIFORM) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) aq[k] = accel[k];
                } else {
#pragma unroll
                    for (int b = 0; b < NPE; ++b)
#pragma unroll
                        for (int k = 0; k < 3; ++k) aq[k] += nq[b] * accel[3 * nd[b] + k];
                }
                const double wd = rho * (w_s[q] * fabs(det));
#pragma unroll
                for (int a = 0; a < NPE; ++a)
#pragma unroll
                    for (int k = 0; k < 3; ++k) f[a][k] += (wd * nq[a]) * aq[k];
            }
            if (tmode != FEM_LOAD_NONE) {
                double dT = 0.0;
                if (tmode == FEM_LOAD_UNIFORM) dT = T[0] - Tref;
                else if (tmode == FEM_LOAD_ELEMENT) dT = T[e] - Tref;
                else {
#pragma unroll
                    for (int b = 0; b < NPE; ++b) dT += nq[b] * (T[nd[b]] - Tref);
                }
                const double s = (mode == FEM_ISO_VOLUME ? vol : w_s[q] * det) * (beta * dT);
#pragma unroll
                for (int a = 0; a < NPE; ++a)
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        f[a][i] += s * (Ji[3 * i] * dq[a * 3] + Ji[3 * i + 1] * dq[a * 3 + 1] +
                                        Ji[3 * i + 2] * dq[a * 3 + 2]);
            }
        }
#pragma unroll
        for (int a = 0; a < NPE; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k) fe[((int64_t)NPE * e + a) * 3 + k] = f[a][k];
    }
}

// ---------------------------------------------------------------- surface loads (thread per face)
__device__ __forceinline__ void load_cross3(const double a[3], const double b[3], double c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// fv [F,NF,3]. The face normal is the right-hand normal of the node order, flipped when it points towards the
// `extra` node (measured from the face centroid); pressure acts against it. A face with a repeated node gives zeros
// (a zero-area face does so by its arithmetic).
template <int NF>
__global__ void __launch_bounds__(256) k_face_loads(const double* __restrict__ X, const int64_t* __restrict__ faces,
                                                    const int64_t* __restrict__ extra, int64_t F,
                                                    const double* __restrict__ p, int pmode,
                                                    const double* __restrict__ tr, int tmode,
                                                    double* __restrict__ fv) {
    for (int64_t fc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; fc < F; fc += (int64_t)gridDim.x * blockDim.x) {
        int64_t nd[NF];
        double x[NF][3], f[NF][3], cen[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < NF; ++a) {
            nd[a] = faces[(int64_t)NF * fc + a];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                x[a][k] = X[3 * nd[a] + k];
                f[a][k] = 0.0;
                cen[k] += x[a][k];
            }
        }
        bool repeated = false;
#pragma unroll
        for (int a = 0; a < NF; ++a)
#pragma unroll
            for (int b = a + 1; b < NF; ++b) repeated = repeated || nd[a] == nd[b];
        double to_extra[3] = {0.0, 0.0, 0.0};
        if (extra) {
            const int64_t xn = extra[fc];
#pragma unroll
            for (int k = 0; k < 3; ++k) to_extra[k] = X[3 * xn + k] - cen[k] / (double)NF;
        }
        const double pv = pmode == FEM_LOAD_NONE ? 0.0 : (pmode == FEM_LOAD_UNIFORM ? p[0] : p[fc]);
        double tv[3] = {0.0, 0.0, 0.0};
        if (tmode != FEM_LOAD_NONE) {
#pragma unroll
            for (int k = 0; k < 3; ++k) tv[k] = tmode == FEM_LOAD_UNIFORM ? tr[k] : tr[3 * fc + k];
        }
        if (!repeated) {
            if constexpr (NF == 3) {
                double e1[3], e2[3], An[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    e1[k] = x[1][k] - x[0][k];
                    e2[k] = x[2][k] - x[0][k];
                }
                load_cross3(e1, e2, An);
#pragma unroll
                for (int k = 0; k < 3; ++k) An[k] = An[k] / 2.0;
                if (An[0] * to_extra[0] + An[1] * to_extra[1] + An[2] * to_extra[2] > 0.0) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) An[k] = -An[k];
                }
                const double area = sqrt(An[0] * An[0] + An[1] * An[1] + An[2] * An[2]);
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        f[a][k] = pmode != FEM_LOAD_NONE ? -(pv / 3.0) * An[k] : (area / 3.0) * tv[k];
            } else {
                constexpr double SX[4] = {-1.0, 1.0, 1.0, -1.0}, SY[4] = {-1.0, -1.0, 1.0, 1.0};
                double xx[3] = {0.0, 0.0, 0.0}, xe[3] = {0.0, 0.0, 0.0}, nc[3];
#pragma unroll
                for (int a = 0; a < NF; ++a)
#pragma unroll
                    for (int k = 0; k < 3; ++k) {   // tangents at the centre
                        xx[k] += (0.25 * SX[a]) * x[a][k];
                        xe[k] += (0.25 * SY[a]) * x[a][k];
                    }
                load_cross3(xx, xe, nc);
                const bool flip = nc[0] * to_extra[0] + nc[1] * to_extra[1] + nc[2] * to_extra[2] > 0.0;
                const double gp = 0.57735026918962576451;   // 1/sqrt(3), weights 1
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double xi = (q & 2) ? gp : -gp, eta = (q & 1) ? gp : -gp;
                    double Nq[4];
#pragma unroll
                    for (int k = 0; k < 3; ++k) xx[k] = xe[k] = 0.0;
#pragma unroll
                    for (int a = 0; a < NF; ++a) {
                        const double sx = SX[a], sy = SY[a];
                        Nq[a] = 0.25 * (1.0 + sx * xi) * (1.0 + sy * eta);
                        const double dx = 0.25 * sx * (1.0 + sy * eta), dy = 0.25 * sy * (1.0 + sx * xi);
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            xx[k] += dx * x[a][k];
                            xe[k] += dy * x[a][k];
                        }
                    }
                    double nA[3];
                    load_cross3(xx, xe, nA);
                    if (flip) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) nA[k] = -nA[k];
                    }
                    const double dA = sqrt(nA[0] * nA[0] + nA[1] * nA[1] + nA[2] * nA[2]);
#pragma unroll
                    for (int a = 0; a < NF; ++a)
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            f[a][k] += pmode != FEM_LOAD_NONE ? -(pv * Nq[a]) * nA[k] : (Nq[a] * dA) * tv[k];
                }
            }
        }
#pragma unroll
        for (int a = 0; a < NF; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k) fv[((int64_t)NF * fc + a) * 3 + k] = f[a][k];
    }
}

static bool mode_ok(int mode, bool element_ok) {
    return mode == FEM_LOAD_NONE || mode == FEM_LOAD_UNIFORM || mode == FEM_LOAD_NODAL ||
           (element_ok && mode == FEM_LOAD_ELEMENT);
}

}  // namespace fem

using namespace fem;

extern "C" {

int fem_tet4_loads(const double* coords, const int64_t* conn, int64_t M, const int32_t* inc_ptr, const int32_t* inc,
                   int64_t N, double rho, const double* accel, int accel_mode, double E, double nu, double alpha,
                   const double* T, int t_mode, double T_ref, double* fe, double* F, int64_t* bad_idx,
                   fem_stream_t stream) {
    if (!mode_ok(accel_mode, false) || !mode_ok(t_mode, true) || (accel_mode != FEM_LOAD_NONE && !accel) ||
        (t_mode != FEM_LOAD_NONE && !T)) {
        set_error("fem_tet4_loads: accel_mode %d / t_mode %d invalid, or a mode without its array", accel_mode, t_mode);
        return FEM_EARG;
    }
    if (N <= 0) return FEM_OK;
    if (M <= 0 || (accel_mode == FEM_LOAD_NONE && t_mode == FEM_LOAD_NONE)) {
        FEM_HIP(hipMemsetAsync(F, 0, sizeof(double) * 3 * (size_t)N, S(stream)));
        return FEM_OK;
    }
    const Tet4LoadArgs A{coords, conn, rho, accel, thermal_beta(E, nu, alpha), T, T_ref, bad_idx};
#define FEM_TL(AM_, TM_)                                                                                              \
    do {                                                                                                              \
        if (fe)                                                                                                       \
            hipLaunchKernelGGL((k_tet4_loads_elem<AM_, TM_>), dim3(stream_grid(M, 256)), dim3(256), 0, S(stream), A, \
                               M, fe);                                                                                \
        else                                                                                                          \
            hipLaunchKernelGGL((k_tet4_loads<AM_, TM_>), dim3(stream_grid(N, 256)), dim3(256), 0, S(stream), A,      \
                               inc_ptr, inc, N, F);                                                                   \
    } while (0)
#define FEM_TL_T(AM_)                                                  \
    switch (t_mode) {                                                  \
        case FEM_LOAD_NONE: FEM_TL(AM_, FEM_LOAD_NONE); break;         \
        case FEM_LOAD_UNIFORM: FEM_TL(AM_, FEM_LOAD_UNIFORM); break;   \
        case FEM_LOAD_NODAL: FEM_TL(AM_, FEM_LOAD_NODAL); break;       \
        default: FEM_TL(AM_, FEM_LOAD_ELEMENT); break;                 \
    }
    switch (accel_mode) {
        case FEM_LOAD_NONE: FEM_TL_T(FEM_LOAD_NONE); break;
        case FEM_LOAD_UNIFORM: FEM_TL_T(FEM_LOAD_UNIFORM); break;
        default: FEM_TL_T(FEM_LOAD_NODAL); break;
    }
#undef FEM_TL_T
#undef FEM_TL
    FEM_LAUNCHED();
    if (fe) return fem_tet4_nl_gather(fe, inc_ptr, inc, N, nullptr, 0.0, nullptr, F, nullptr, stream);
    return FEM_OK;
}

int fem_iso_loads(const double* coords, const int64_t* conn, int64_t M, int npe, const double* Nv, const double* dN,
                  const double* w, int n_ip, int mode, double rho, const double* accel, int accel_mode, double E,
                  double nu, double alpha, const double* T, int t_mode, double T_ref, double* fe,
                  fem_stream_t stream) {
    if (!mode_ok(accel_mode, false) || !mode_ok(t_mode, true) || (accel_mode != FEM_LOAD_NONE && !accel) ||
        (t_mode != FEM_LOAD_NONE && !T)) {
        set_error("fem_iso_loads: accel_mode %d / t_mode %d invalid, or a mode without its array", accel_mode, t_mode);
        return FEM_EARG;
    }
    if (mode != FEM_ISO_SUM && !(mode == FEM_ISO_VOLUME && npe == 6 && n_ip == 1)) {
        set_error("fem_iso_loads: mode %d (FEM_ISO_SUM, or FEM_ISO_VOLUME for npe 6 at one point)", mode);
        return FEM_EARG;
    }
    if (n_ip < 1 || n_ip > ISO_MAX_IP) {
        set_error("fem_iso_loads: n_ip = %d out of range [1, %d]", n_ip, ISO_MAX_IP);
        return FEM_EARG;
    }
    if (npe != 6 && npe != 8 && npe != 10) {
        set_error("fem_iso_loads: npe %d not supported (6, 8, 10)", npe);
        return FEM_EBADTYPE;
    }
    if (M <= 0) return FEM_OK;
    const dim3 g(stream_grid(M, 256)), b(256);
    const double beta = thermal_beta(E, nu, alpha);
#define FEM_IL(NPE_)                                                                                                 \
    hipLaunchKernelGGL(k_iso_loads<NPE_>, g, b, 0, S(stream), coords, conn, M, Nv, dN, w, n_ip, mode, rho, accel,   \
                       accel_mode, beta, T, t_mode, T_ref, fe)
    switch (npe) {
        case 6: FEM_IL(6); break;
        case 8: FEM_IL(8); break;
        default: FEM_IL(10); break;
    }
#undef FEM_IL
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_face_loads(const double* coords, const int64_t* faces, int64_t F, int nf, const int64_t* extra,
                   const double* p, int p_mode, const double* t, int t_mode, double* fv, fem_stream_t stream) {
    const bool has_p = p_mode != FEM_LOAD_NONE, has_t = t_mode != FEM_LOAD_NONE;
    if (has_p == has_t || (has_p && (!p || (p_mode != FEM_LOAD_UNIFORM && p_mode != FEM_LOAD_ELEMENT))) ||
        (has_t && (!t || (t_mode != FEM_LOAD_UNIFORM && t_mode != FEM_LOAD_ELEMENT)))) {
        set_error("fem_face_loads: exactly one of pressure / traction, each FEM_LOAD_UNIFORM or FEM_LOAD_ELEMENT");
        return FEM_EARG;
    }
    if (nf != 3 && nf != 4) {
        set_error("fem_face_loads: %d nodes per face not supported (3, 4)", nf);
        return FEM_EBADTYPE;
    }
    if (F <= 0) return FEM_OK;
    const dim3 g(stream_grid(F, 256)), b(256);
    if (nf == 3)
        hipLaunchKernelGGL(k_face_loads<3>, g, b, 0, S(stream), coords, faces, extra, F, p, p_mode, t, t_mode, fv);
    else
        hipLaunchKernelGGL(k_face_loads<4>, g, b, 0, S(stream), coords, faces, extra, F, p, p_mode, t, t_mode, fv);
    FEM_LAUNCHED();
    return FEM_OK;
}

}  // extern "C"
