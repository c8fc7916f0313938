// Explicit dynamics: central-difference (leapfrog) time stepping of M a + alpha M v + f_int(u) = amp(t) f_ext on c3d4
// meshes with the lumped mass, the internal force formed on the element chunks of the matrix-free operator
// (matfree.hpp: one workgroup per chunk, the chunk's nodes in LDS, fixed-order node sums into slots, no atomics).
//
//   k_xd_force   : per chunk, slots <- the chunk's share of f_int(u) for the material
//                    linear       f_a = V sigma(H) g_a, the arithmetic of mf_element<3, MF_APPLY>
//                    svk          f_a = V F S g_a, S = lam tr(E) I + 2 mu E, E = (H + H^T + H^T H) / 2
//                    neo_hookean  f_a = V P g_a, P = mu (F - F^-T) + lam ln J F^-T
//                  with H = sum_a u_a (x) g_a (formed from the differences u_b - u_0, so a translation adds nothing),
//                  F = I + H; det F and the cofactors of F in the compensated forms dop / dot3c of element.hpp. An
//                  element with det F <= 0 or a degenerate reference element adds zero force and lowers the status
//                  word to the step; on energy steps the workgroup's strain energy goes to epart[chunk].
//   k_xd_update  : per dof, f_int = the node's slots in ascending chunk order, then
//                    v_{n+1/2} = ((1 - alpha dt/2) v_{n-1/2} + dt (amp_n f_ext - f_int) / m) / (1 + alpha dt/2)
//                    u_{n+1}   = u_n + dt v_{n+1/2}
//                  (the first step after a start or a change of dt: v_{1/2} = v_0 + (dt/2) a_0), the record rows
//                  (u_n, v_n = (v_{n-1/2} + v_{n+1/2}) / 2, a_n = (amp_n f_ext - f_int) / m - alpha v_n), the partials
//                  of the kinetic energy, the external power and the external work term, and the non-finite word.
//                  The same kernel without the advance gives v_n and a_n at the end of a run.
//   k_xd_update_c: k_xd_update per node with the penalty contact force of up to 8 rigid surfaces (planes, spheres,
//                  cylinders; normal force kappa m / dt^2 p, capped Coulomb friction in surface order), used in its
//                  place when a contact set is attached; on history steps the per-surface partials, summed by
//                  k_xd_csum (one workgroup, workgroup order).
//   k_xd_sum     : one workgroup: the partials summed in workgroup order.
//   k_xd_mass    : lumped mass, per chunk the rho V_e / 4 of every (element, corner) summed per local node in the
//                  layout's order; the nodes' slots are then summed by k_mf_gather<1>.
//   k_xd_dt      : per element dt_e = 1 / (c_d sqrt(sum_a |g_a|^2)), c_d^2 = (max(lam, 0) + 2 mu) / rho, and the minimum
//                  by per-workgroup partials. x^T K_e x = V (lam (tr H)^2 + 2 mu |sym H|^2) and both (tr H)^2 and
//                  |sym H|^2 are <= sum|g_a|^2 sum|x_a|^2 (Cauchy-Schwarz), so with the lumped element mass rho V / 4
//                  the largest element eigenvalue is <= 4 c_d^2 sum|g_a|^2 and dt_e <= 2 / omega_max of the mesh.
// The rules of modal.hip and transient.hip hold: plain launches, no workgroup waits on another, no floating-point
// atomics (the two status words are integer minima), every reduction is per-workgroup partials summed in workgroup
// order by a one-workgroup launch, nothing is read or stored past N or M, results are bit-reproducible.
#include <math.h>

#include "matfree.hpp"

namespace fem {

constexpr int XD_BLOCK = 256;
constexpr unsigned long long XD_NONE = ~0ull;
constexpr int XD_NE = 4;   // values per energy row: kinetic, strain, external power, external work term

// signed det of the edge matrix and the unscaled cofactors c_1..c_3 (g_b = c_b / det), as mf_element forms them
__device__ __forceinline__ double xd_cofactors(const double xc[4][3], double c[4][3]) {
    double e[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e[0][k] = xc[1][k] - xc[0][k];
        e[1][k] = xc[2][k] - xc[0][k];
        e[2][k] = xc[3][k] - xc[0][k];
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const double* u = e[(b + 1) % 3];
        const double* v = e[(b + 2) % 3];
        c[b + 1][0] = u[1] * v[2] - u[2] * v[1];
        c[b + 1][1] = u[2] * v[0] - u[0] * v[2];
        c[b + 1][2] = u[0] * v[1] - u[1] * v[0];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) c[0][k] = -(c[1][k] + c[2][k] + c[3][k]);
    return e[0][0] * c[1][0] + e[0][1] * c[1][1] + e[0][2] * c[1][2];
}

// The four corner forces f and the strain energy V W of one element. Returns false (f = 0, w = 0) for a degenerate
// reference element or, for the nonlinear materials, det F <= 0 (a NaN included): no logarithm of a non-positive
// number is taken and no NaN leaves the function.
template <int MAT, bool ENERGY>
__device__ __forceinline__ bool xd_element(const double xc[4][3], const double uv[4][3], double lam, double mu,
                                           double f[4][3], double& w) {
    double c[4][3];
    const double det = xd_cofactors(xc, c);
    w = 0.0;
    // every value is formed on every path and a rejected element's are dropped by the selects at the end (forces
    // written under two branches kept part of f in scratch)
    bool ok = fabs(det) >= 1e-12;
    if constexpr (MAT == FEM_MAT_LINEAR) {
        mf_element<3, MF_APPLY>(xc, uv, lam, mu, 0.0, f);
        if constexpr (ENERGY) {   // u_e . K_e u_e / 2 = V sigma : eps / 2
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int q = 0; q < 3; ++q) s += uv[a][q] * f[a][q];
            w = 0.5 * s;
        }
    } else {
        const double inv = mf_rcp(det);
        const double V = fabs(det) * (1.0 / 6.0);
        double g[4][3];   // g[1..3] used
#pragma unroll
        for (int b = 1; b < 4; ++b)
#pragma unroll
            for (int k = 0; k < 3; ++k) g[b][k] = c[b][k] * inv;
        double H[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double d1 = uv[1][i] - uv[0][i], d2 = uv[2][i] - uv[0][i], d3 = uv[3][i] - uv[0][i];
#pragma unroll
            for (int j = 0; j < 3; ++j) H[i][j] = d1 * g[1][j] + d2 * g[2][j] + d3 * g[3][j];
        }
        double F[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) F[i][j] = (i == j ? 1.0 : 0.0) + H[i][j];
        double Cf[3][3];   // cofactors of F
        Cf[0][0] = dop(F[1][1], F[2][2], F[1][2], F[2][1]);
        Cf[0][1] = dop(F[1][2], F[2][0], F[1][0], F[2][2]);
        Cf[0][2] = dop(F[1][0], F[2][1], F[1][1], F[2][0]);
        const double J = dot3c(F[0][0], Cf[0][0], F[0][1], Cf[0][1], F[0][2], Cf[0][2]);
        ok = ok && J > 0.0;   // false for a NaN as well
        const double Js = ok ? J : 1.0;
        double P[3][3];   // first Piola-Kirchhoff stress
        if constexpr (MAT == FEM_MAT_SVK) {
            // Green-Lagrange strain from H (xx, yy, zz, xy, yz, xz): exactly zero at u = 0
            double Ed[6];
            Ed[0] = H[0][0] + 0.5 * (H[0][0] * H[0][0] + H[1][0] * H[1][0] + H[2][0] * H[2][0]);
            Ed[1] = H[1][1] + 0.5 * (H[0][1] * H[0][1] + H[1][1] * H[1][1] + H[2][1] * H[2][1]);
            Ed[2] = H[2][2] + 0.5 * (H[0][2] * H[0][2] + H[1][2] * H[1][2] + H[2][2] * H[2][2]);
            Ed[3] = 0.5 * ((H[0][1] + H[1][0]) + (H[0][0] * H[0][1] + H[1][0] * H[1][1] + H[2][0] * H[2][1]));
            Ed[4] = 0.5 * ((H[1][2] + H[2][1]) + (H[0][1] * H[0][2] + H[1][1] * H[1][2] + H[2][1] * H[2][2]));
            Ed[5] = 0.5 * ((H[0][2] + H[2][0]) + (H[0][0] * H[0][2] + H[1][0] * H[1][2] + H[2][0] * H[2][2]));
            const double trE = (Ed[0] + Ed[1]) + Ed[2];
            const double lt = lam * trE, m2 = 2.0 * mu;
            const double S[3][3] = {{lt + m2 * Ed[0], m2 * Ed[3], m2 * Ed[5]},
                                    {m2 * Ed[3], lt + m2 * Ed[1], m2 * Ed[4]},
                                    {m2 * Ed[5], m2 * Ed[4], lt + m2 * Ed[2]}};
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) P[i][j] = F[i][0] * S[0][j] + F[i][1] * S[1][j] + F[i][2] * S[2][j];
            if constexpr (ENERGY)
                w = V * (0.5 * lam * trE * trE + mu * ((Ed[0] * Ed[0] + Ed[1] * Ed[1] + Ed[2] * Ed[2]) +
                                                       2.0 * (Ed[3] * Ed[3] + Ed[4] * Ed[4] + Ed[5] * Ed[5])));
        } else {
            Cf[1][0] = dop(F[0][2], F[2][1], F[0][1], F[2][2]);
            Cf[1][1] = dop(F[0][0], F[2][2], F[0][2], F[2][0]);
            Cf[1][2] = dop(F[0][1], F[2][0], F[0][0], F[2][1]);
            Cf[2][0] = dop(F[0][1], F[1][2], F[0][2], F[1][1]);
            Cf[2][1] = dop(F[0][2], F[1][0], F[0][0], F[1][2]);
            Cf[2][2] = dop(F[0][0], F[1][1], F[0][1], F[1][0]);
            const double lnJ = log(Js);
            // P = mu F + (lam ln J - mu) F^-T, F^-T = Cf / J; mu (F - F^-T) is formed entry by entry so that the
            // two cancel at F = I
            const double iJ = 1.0 / Js;
            const double ll = lam * lnJ;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double t = iJ * Cf[i][j];
                    P[i][j] = mu * (F[i][j] - t) + ll * t;
                }
            if constexpr (ENERGY) {
                double hh = 0.0;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) hh += H[i][j] * H[i][j];
                const double ff3 = 2.0 * ((H[0][0] + H[1][1]) + H[2][2]) + hh;   // F:F - 3
                w = V * ((0.5 * mu * ff3 - mu * lnJ) + 0.5 * lam * lnJ * lnJ);
            }
        }
#pragma unroll
        for (int a = 1; a < 4; ++a)
#pragma unroll
            for (int i = 0; i < 3; ++i) f[a][i] = V * (P[i][0] * g[a][0] + P[i][1] * g[a][1] + P[i][2] * g[a][2]);
#pragma unroll
        for (int q = 0; q < 3; ++q) f[0][q] = -(f[1][q] + f[2][q] + f[3][q]);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int q = 0; q < 3; ++q) f[a][q] = ok ? f[a][q] : 0.0;
    w = ok ? w : 0.0;
    return ok;
}

// One workgroup per chunk (grid = nchunks): the chunk's local nodes (coordinates, u) and pairs into LDS, the element
// forces MF_PASS elements at a time, every local node's pairs summed in the layout's order into its slot.
template <int MAT, bool ENERGY>
__global__ void __launch_bounds__(XD_BLOCK) k_xd_force(MfOp op, const double* __restrict__ u,
                                                       double* __restrict__ slots, double* __restrict__ epart,
                                                       unsigned long long* __restrict__ status,
                                                       unsigned long long step) {
    static_assert(XD_BLOCK == MF_PASS && MF_NC <= XD_BLOCK, "a thread per element of a pass and per local node");
    __shared__ MfLds<3> L;
    __shared__ double red[4];
    const int64_t c = blockIdx.x;
    if (c >= op.nchunks) return;
    const int tid = threadIdx.x;
    const int e0 = op.cptr[c], ne = op.cptr[c + 1] - e0;
    const int s0 = op.sbase[c], nn = op.sbase[c + 1] - s0;
    const bool own = tid < nn;
    int pos = 0, end = 0, sp = 0;
    if (own) {
        const int64_t g = op.cnode[s0 + tid];
        pos = op.lptr[s0 + c + tid];
        end = op.lptr[s0 + c + tid + 1];
        sp = op.spos ? op.spos[s0 + tid] : s0 + tid;
        double* r = reinterpret_cast<double*>(L.nd_row(tid));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r[k] = op.X[3 * g + k];
            r[3 + k] = u[3 * g + k];
        }
    }
    if (8 * tid < 4 * ne)
        reinterpret_cast<mf_u32x4*>(L.ent)[tid] = reinterpret_cast<const mf_u32x4*>(op.lent + 4 * (int64_t)e0)[tid];
    __syncthreads();
    // the node's pairs split at the pass boundary (pairs ascend by element): lower bound of 4 MF_PASS
    int mid = end;
    if (ne > MF_PASS) {
        int lo = pos, len = end - pos;
        while (len > 0) {
            const int half = len >> 1;
            if (L.ent[lo + half] < 4 * MF_PASS) {
                lo += half + 1;
                len -= half + 1;
            } else {
                len = half;
            }
        }
        mid = lo;
    }
    double acc[3] = {0.0, 0.0, 0.0};
    double wsum = 0.0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < MF_EC / MF_PASS; ++j) {
        const int h = MF_PASS * j;
        if (h >= ne) break;
        if (h + tid < ne) {
            const uint32_t w = op.eloc[e0 + h + tid];
            double xc[4][3], uv[4][3], f[4][3], we;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double2* r = L.nd_row((w >> (8 * b)) & 0xff);
                const double2 a0 = r[0], a1 = r[1], a2 = r[2];
                xc[b][0] = a0.x;
                xc[b][1] = a0.y;
                xc[b][2] = a1.x;
                uv[b][0] = a1.y;
                uv[b][1] = a2.x;
                uv[b][2] = a2.y;
            }
            bad |= !xd_element<MAT, ENERGY>(xc, uv, op.lam, op.mu, f, we);
            wsum += we;
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int q = 0; q < 3; ++q) L.fs[b * 3 + q][tid] = f[b][q];
        }
        __syncthreads();
        const int stop = j == 0 ? mid : end;
        for (; pos + MF_U <= stop; pos += MF_U) {
            int pe[MF_U];
#pragma unroll
            for (int t = 0; t < MF_U; ++t) pe[t] = L.ent[pos + t];
            double v[MF_U][3];
#pragma unroll
            for (int t = 0; t < MF_U; ++t) mf_pair_value<3>(L, pe[t], h, v[t]);
#pragma unroll
            for (int t = 0; t < MF_U; ++t)
#pragma unroll
                for (int q = 0; q < 3; ++q) acc[q] += v[t][q];
        }
        for (; pos < stop; ++pos) {
            double v[3];
            mf_pair_value<3>(L, L.ent[pos], h, v);
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[q] += v[q];
        }
        __syncthreads();
    }
    if (own) {
#pragma unroll
        for (int q = 0; q < 3; ++q) slots[(int64_t)sp * 3 + q] = acc[q];
    }
    if (bad) atomicMin(status, step);
    if constexpr (ENERGY) {
        const double t = block_sum256(wsum, red);
        if (tid == 0) epart[c] = t;
    }
}

// what one launch of the update does
struct XdUpd {
    int64_t n3;
    double dt, c1, c2, alpha, amp;   // c1 = 1 - alpha dt / 2, c2 = 1 / (1 + alpha dt / 2)
    unsigned long long step;
    const double* fext;      // [3N] or null
    const double* mass;      // [N]
    const uint8_t* mask;     // [3N] or null
    double *u, *vh, *v, *a;  // [3N]
    const int32_t* recmap;   // [3N] record column of the dof (-1: none) or null
    double *ru, *rv, *ra;    // this step's record rows
    double* kpart;           // [grid, 3] energy partials
    unsigned long long* status;   // [2]: first inverted step, first non-finite step
};

// FROMV: the velocity is the full-step v (after a start or a change of dt), else the half-step vh. ADV: advance u and
// vh (a time step), else write v_n and a_n only (the state at the end of a run; after a start also the masked zeros).
template <bool FROMV, bool ADV, bool ENERGY>
__global__ void __launch_bounds__(XD_BLOCK) k_xd_update(MfOp op, XdUpd p, const double* __restrict__ slots) {
    // no product is fused into a sum: every variant of this kernel then forms v_n and a_n with the same roundings (a
    // recorded row of a long run equals the state a run ending at that step returns, bit for bit)
#pragma clang fp contract(off)
    __shared__ double red[4];
    double ke = 0.0, pw = 0.0, wk = 0.0;
    for (int64_t d = (int64_t)blockIdx.x * XD_BLOCK + threadIdx.x; d < p.n3; d += (int64_t)gridDim.x * XD_BLOCK) {
        const int64_t i = d / 3;
        const int q = (int)(d - 3 * i);
        const double m = p.mass[i];
        const bool fixed = (p.mask && p.mask[d]) || !(m > 0.0);   // a node of no element has no mass: it stays put
        double un = 0.0, vn = 0.0, an = 0.0, vhn = 0.0, fx = 0.0;
        if (!fixed) {
            double fint = 0.0;
            const int k0 = op.nptr[i], k1 = op.nptr[i + 1];
            for (int k = k0; k < k1; ++k) fint += slots[(int64_t)(op.spos ? k : op.nslot[k]) * 3 + q];
            fx = p.fext ? p.amp * p.fext[d] : 0.0;
            const double rm = (fx - fint) / m;
            un = p.u[d];
            if (FROMV) {
                vn = p.v[d];
                an = rm - p.alpha * vn;
                vhn = vn + 0.5 * p.dt * an;
            } else {
                const double vho = p.vh[d];
                vhn = (p.c1 * vho + p.dt * rm) * p.c2;
                vn = 0.5 * (vho + vhn);
                an = rm - p.alpha * vn;
            }
        }
        if (ADV) {
            const double unew = fixed ? 0.0 : un + p.dt * vhn;
            p.u[d] = unew;
            p.vh[d] = vhn;
            if (!(fabs(unew) <= 1.79769313486231570815e308) || !(fabs(vhn) <= 1.79769313486231570815e308))
                atomicMin(p.status + 1, p.step);
            if (p.recmap) {
                const int col = p.recmap[d];
                if (col >= 0) {
                    p.ru[col] = un;
                    p.rv[col] = vn;
                    p.ra[col] = an;
                }
            }
            if (ENERGY) {
                ke += 0.5 * m * vn * vn;
                pw += fx * vn;
                wk += fx * un;
            }
        } else {
            p.v[d] = vn;
            p.a[d] = an;
            if (FROMV) {
                p.u[d] = un;
                p.vh[d] = 0.0;
            }
        }
    }
    if (ADV && ENERGY) {
        ke = block_sum256(ke, red);
        pw = block_sum256(pw, red);
        wk = block_sum256(wk, red);
        if (threadIdx.x == 0) {
            p.kpart[(int64_t)blockIdx.x * 3] = ke;
            p.kpart[(int64_t)blockIdx.x * 3 + 1] = pw;
            p.kpart[(int64_t)blockIdx.x * 3 + 2] = wk;
        }
    }
}

// ---------------------------------------------------------------- penalty contact with rigid surfaces
constexpr int XD_MAXS = 8;    // surfaces of a contact set
constexpr int XD_SV = 13;     // host values per surface: kind, inside, point, vector, radius, mu, velocity at a start
constexpr int XD_NH = 5;      // values per surface of a history row: reaction (3), nodes in contact, largest penetration
constexpr int XD_NCE = 3;     // values of a contact energy row: penalty energy, friction power, surface power
constexpr int XD_CP = XD_MAXS * XD_NH + XD_NCE;   // partials per workgroup of the contact update

struct XdSurf {
    double c[3], n[3], w[3];   // reference point at this step, unit normal or axis, velocity of this step
    double R, mu;
    int kind, inside;
};

// the contact set as one launch sees it (by value in the kernel arguments)
struct XdCon {
    int ns;
    double kappa;
    double dt;                 // the step of the penalty stiffness kappa m / dt^2 and of the friction cap
    const uint8_t* word;       // [N] or null: bit s set -> the node may touch surface s
    double* cpart;             // [grid, XD_CP]
    XdSurf s[XD_MAXS];
};

// penetration p = -g and the normal nu of surface S at x; false where S exerts nothing on the node: not penetrated
// (g = 0 included), a NaN, or |r| = 0 (a node at a sphere's centre or on a cylinder's axis has no normal)
__device__ __forceinline__ bool xd_gap(const XdSurf& S, const double x[3], double& pen, double nu[3]) {
#pragma clang fp contract(off)
    double r[3] = {x[0] - S.c[0], x[1] - S.c[1], x[2] - S.c[2]};
    const double dn = (r[0] * S.n[0] + r[1] * S.n[1]) + r[2] * S.n[2];
    double g;
    if (S.kind == FEM_SURF_PLANE) {
        g = dn;
#pragma unroll
        for (int q = 0; q < 3; ++q) nu[q] = S.n[q];
    } else {
        if (S.kind == FEM_SURF_CYLINDER) {
#pragma unroll
            for (int q = 0; q < 3; ++q) r[q] = r[q] - dn * S.n[q];
        }
        const double rr = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
        if (!(rr > 0.0)) return false;
        const double sg = S.inside ? -1.0 : 1.0;
        g = sg * (rr - S.R);
#pragma unroll
        for (int q = 0; q < 3; ++q) nu[q] = sg * (r[q] / rr);
    }
    pen = -g;
    return pen > 0.0;
}

__device__ __forceinline__ double xd_block_max256(double v, double* lds4) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(lds4[0], lds4[1]), fmax(lds4[2], lds4[3]));
}

// k_xd_update with a contact set: one thread per node (the gap, the normal and the friction cap need the node's three
// components together). Per dof the arithmetic of k_xd_update in its order, with rm = (amp f_ext - f_int + f_c) / m
// where the node touches a surface and (amp f_ext - f_int) / m where it does not: a run whose surfaces are never
// touched gives the bits of k_xd_update. f_c = sum over the touched surfaces in index order of
//   f_n = k p nu, k = kappa m / dt^2, and f_t = -min(mu |f_n|, m |vt| / sigma) vt / |vt|,
// vt the tangential part of v* - w, v* the new half-step velocity formed with all normal forces and the friction of the
// surfaces before this one (sigma = dt c2, dt / 2 for FROMV: what a unit force per unit mass adds to it); the
// components on held dofs are dropped, and v* is 0 there. HIST: the per-surface partials of a history row (the surface
// loop is then unrolled so that the sums stay in registers); ENERGY: also the three contact energy partials.
template <bool FROMV, bool ADV, bool ENERGY, bool HIST>
__global__ void __launch_bounds__(XD_BLOCK) k_xd_update_c(MfOp op, XdUpd p, XdCon ct, const double* __restrict__ slots) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    double ke = 0.0, pw = 0.0, wk = 0.0, ce = 0.0, fpw = 0.0, spw = 0.0;
    double hr[HIST ? XD_MAXS : 1][XD_NH];
#pragma unroll
    for (int s = 0; s < (HIST ? XD_MAXS : 1); ++s)
#pragma unroll
        for (int j = 0; j < XD_NH; ++j) hr[s][j] = 0.0;
    const int64_t N = p.n3 / 3;
    const double sigma = FROMV ? 0.5 * ct.dt : ct.dt * p.c2;
    constexpr int UNR = HIST ? XD_MAXS : 1;   // the surface loop of the friction pass: unrolled for the history sums
    for (int64_t i = (int64_t)blockIdx.x * XD_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * XD_BLOCK) {
        const double m = p.mass[i];
        const bool live = m > 0.0;   // a node of no element has no mass: it stays put and feels no surface
        bool fixed[3];
        double un[3], vo[3], num[3], fx[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int64_t d = 3 * i + q;
            fixed[q] = (p.mask && p.mask[d]) || !live;
            un[q] = vo[q] = num[q] = fx[q] = 0.0;
            if (!fixed[q]) {
                double fint = 0.0;
                const int k0 = op.nptr[i], k1 = op.nptr[i + 1];
                for (int k = k0; k < k1; ++k) fint += slots[(int64_t)(op.spos ? k : op.nslot[k]) * 3 + q];
                fx[q] = p.fext ? p.amp * p.fext[d] : 0.0;
                num[q] = fx[q] - fint;
                un[q] = p.u[d];
                vo[q] = FROMV ? p.v[d] : p.vh[d];
            }
        }
        double fc[3] = {0.0, 0.0, 0.0}, ft[3] = {0.0, 0.0, 0.0};   // contact force, its friction part
        double ftw = 0.0;                                           // sum f_t . w
        unsigned hit = 0;
        const unsigned word = live ? (ct.word ? ct.word[i] : 0xffu) : 0u;
        if (word) {
            const double x[3] = {op.X[3 * i] + un[0], op.X[3 * i + 1] + un[1], op.X[3 * i + 2] + un[2]};
            const double kp = ct.kappa * m / (ct.dt * ct.dt);
            double fn[3] = {0.0, 0.0, 0.0};
            for (int s = 0; s < ct.ns; ++s) {
                if (!((word >> s) & 1u)) continue;
                double pen, nu[3];
                if (!xd_gap(ct.s[s], x, pen, nu)) continue;
                hit |= 1u << s;
#pragma unroll
                for (int q = 0; q < 3; ++q) fn[q] += (kp * pen) * nu[q];
            }
            if (hit) {
                double vs[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const double rn = (num[q] + fn[q]) / m;
                    const double t = FROMV ? vo[q] + 0.5 * ct.dt * (rn - p.alpha * vo[q])
                                           : (p.c1 * vo[q] + ct.dt * rn) * p.c2;
                    vs[q] = fixed[q] ? 0.0 : t;
                }
#pragma unroll UNR
                for (int s = 0; s < XD_MAXS; ++s) {
                    if (s >= ct.ns || !((hit >> s) & 1u)) continue;
                    const XdSurf& S = ct.s[s];
                    double pen, nu[3];
                    (void)xd_gap(S, x, pen, nu);
                    const double fnm = kp * pen;
                    double fs[3], rel[3];
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        fs[q] = fixed[q] ? 0.0 : fnm * nu[q];
                        rel[q] = vs[q] - S.w[q];
                    }
                    const double vnn = (rel[0] * nu[0] + rel[1] * nu[1]) + rel[2] * nu[2];
                    double vt[3];
#pragma unroll
                    for (int q = 0; q < 3; ++q) vt[q] = rel[q] - vnn * nu[q];
                    const double vtm = sqrt((vt[0] * vt[0] + vt[1] * vt[1]) + vt[2] * vt[2]);
                    if (S.mu > 0.0 && vtm > 0.0) {
                        const double cap = fmin(S.mu * fnm, m * vtm / sigma);
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            const double f = fixed[q] ? 0.0 : -(cap * (vt[q] / vtm));
                            vs[q] += sigma * f / m;
                            fs[q] += f;
                            ft[q] += f;
                            ftw += f * S.w[q];
                        }
                    }
#pragma unroll
                    for (int q = 0; q < 3; ++q) fc[q] += fs[q];
                    if (ADV && HIST) {
#pragma unroll
                        for (int q = 0; q < 3; ++q) hr[HIST ? s : 0][q] -= fs[q];
                        hr[HIST ? s : 0][3] += 1.0;
                        hr[HIST ? s : 0][4] = fmax(hr[HIST ? s : 0][4], pen);
                    }
                    if (ADV && ENERGY) {
                        ce += 0.5 * kp * pen * pen;
                        spw += (fs[0] * S.w[0] + fs[1] * S.w[1]) + fs[2] * S.w[2];
                    }
                }
            }
        }
        double vnv[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int64_t d = 3 * i + q;
            double vn = 0.0, an = 0.0, vhn = 0.0;
            if (!fixed[q]) {
                const double rm = (hit ? num[q] + fc[q] : num[q]) / m;
                if (FROMV) {
                    vn = vo[q];
                    an = rm - p.alpha * vn;
                    vhn = vn + 0.5 * p.dt * an;
                } else {
                    vhn = (p.c1 * vo[q] + p.dt * rm) * p.c2;
                    vn = 0.5 * (vo[q] + vhn);
                    an = rm - p.alpha * vn;
                }
            }
            vnv[q] = vn;
            if (ADV) {
                const double unew = fixed[q] ? 0.0 : un[q] + p.dt * vhn;
                p.u[d] = unew;
                p.vh[d] = vhn;
                if (!(fabs(unew) <= 1.79769313486231570815e308) || !(fabs(vhn) <= 1.79769313486231570815e308))
                    atomicMin(p.status + 1, p.step);
                if (p.recmap) {
                    const int col = p.recmap[d];
                    if (col >= 0) {
                        p.ru[col] = un[q];
                        p.rv[col] = vn;
                        p.ra[col] = an;
                    }
                }
                if (ENERGY) {
                    ke += 0.5 * m * vn * vn;
                    pw += fx[q] * vn;
                    wk += fx[q] * un[q];
                }
            } else {
                p.v[d] = vn;
                p.a[d] = an;
                if (FROMV) {
                    p.u[d] = un[q];
                    p.vh[d] = 0.0;
                }
            }
        }
        if (ADV && ENERGY && hit) fpw += ((ft[0] * vnv[0] + ft[1] * vnv[1]) + ft[2] * vnv[2]) - ftw;
    }
    if (ADV && ENERGY) {
        ke = block_sum256(ke, red);
        pw = block_sum256(pw, red);
        wk = block_sum256(wk, red);
        ce = block_sum256(ce, red);
        fpw = block_sum256(fpw, red);
        spw = block_sum256(spw, red);
        if (threadIdx.x == 0) {
            p.kpart[(int64_t)blockIdx.x * 3] = ke;
            p.kpart[(int64_t)blockIdx.x * 3 + 1] = pw;
            p.kpart[(int64_t)blockIdx.x * 3 + 2] = wk;
            double* c = ct.cpart + (int64_t)blockIdx.x * XD_CP + XD_MAXS * XD_NH;
            c[0] = ce;
            c[1] = fpw;
            c[2] = spw;
        }
    }
    if (ADV && HIST) {
#pragma unroll
        for (int s = 0; s < XD_MAXS; ++s) {
            if (s >= ct.ns) break;
#pragma unroll
            for (int j = 0; j < XD_NH; ++j) {
                const double t = j == 4 ? xd_block_max256(hr[HIST ? s : 0][j], red)
                                        : block_sum256(hr[HIST ? s : 0][j], red);
                if (threadIdx.x == 0) ct.cpart[(int64_t)blockIdx.x * XD_CP + s * XD_NH + j] = t;
            }
        }
    }
}

// one workgroup: the contact partials of `nk` workgroups summed in workgroup order (the largest penetration: the
// maximum), wave w the values w, w + 4, ...; hist [ns, XD_NH] and en [XD_NCE] are each written where given
__global__ void __launch_bounds__(256) k_xd_csum(const double* __restrict__ cpart, int nk, int ns,
                                                 double* __restrict__ hist, double* __restrict__ en) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = wave; j < XD_CP; j += 4) {
        const bool energy = j >= XD_MAXS * XD_NH;
        const int s = j / XD_NH, c = j - s * XD_NH;
        if (energy ? en == nullptr : (hist == nullptr || s >= ns)) continue;   // the same in every lane
        const bool mx = !energy && c == 4;
        double v = 0.0;
        for (int i = lane; i < nk; i += 64) {
            const double t = cpart[(int64_t)i * XD_CP + j];
            v = mx ? fmax(v, t) : v + t;
        }
        if (mx) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
        } else {
            v = wave_sum(v);
        }
        if (lane == 0) {
            if (energy) en[j - XD_MAXS * XD_NH] = v;
            else hist[s * XD_NH + c] = v;
        }
    }
}

// one workgroup, a wave per value: lane l adds partials l, l + 64, ... in order, then the wave tree.
// out = (kinetic, strain, external power, external work term)
__global__ void __launch_bounds__(256) k_xd_sum(const double* __restrict__ kpart, int nk,
                                                const double* __restrict__ epart, int64_t ne,
                                                double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s = 0.0;
    if (wave == 1) {
        for (int64_t i = lane; i < ne; i += 64) s += epart[i];
    } else {
        const int col = wave == 0 ? 0 : wave - 1;
        for (int i = lane; i < nk; i += 64) s += kpart[(int64_t)i * 3 + col];
    }
    s = wave_sum(s);
    if (lane == 0) out[wave] = s;
}

__global__ void __launch_bounds__(256) k_xd_recmap(const int64_t* __restrict__ dofs, int64_t nrec,
                                                   int32_t* __restrict__ map) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nrec; k += (int64_t)gridDim.x * 256)
        map[dofs[k]] = (int32_t)k;
}

// ---------------------------------------------------------------- lumped mass
// per chunk: q_e = rho V_e / 4 of its elements in LDS, then every local node adds its pairs' q in the layout's order
__global__ void __launch_bounds__(XD_BLOCK) k_xd_mass(MfOp op, double rho, double* __restrict__ slots) {
    __shared__ double xs[MF_NC][3];
    __shared__ double qe[MF_EC];
    __shared__ alignas(16) uint16_t ent[4 * MF_EC];
    const int64_t c = blockIdx.x;
    if (c >= op.nchunks) return;
    const int tid = threadIdx.x;
    const int e0 = op.cptr[c], ne = op.cptr[c + 1] - e0;
    const int s0 = op.sbase[c], nn = op.sbase[c + 1] - s0;
    if (tid < nn) {
        const int64_t g = op.cnode[s0 + tid];
#pragma unroll
        for (int k = 0; k < 3; ++k) xs[tid][k] = op.X[3 * g + k];
    }
    if (8 * tid < 4 * ne)
        reinterpret_cast<mf_u32x4*>(ent)[tid] = reinterpret_cast<const mf_u32x4*>(op.lent + 4 * (int64_t)e0)[tid];
    __syncthreads();
    for (int e = tid; e < ne; e += XD_BLOCK) {
        const uint32_t w = op.eloc[e0 + e];
        // only |det| enters. A chunk's local nodes ascend by global id, so the four local ids sorted are the nodes
        // in ascending global id: det from them (the form of tet4_det_sorted) is the same bits for any local order
        // of the element's nodes
        int n[4] = {(int)(w & 0xff), (int)((w >> 8) & 0xff), (int)((w >> 16) & 0xff), (int)((w >> 24) & 0xff)};
#define XD_CSWAP(i, j)           \
    if (n[j] < n[i]) {           \
        const int t_ = n[i];     \
        n[i] = n[j];             \
        n[j] = t_;               \
    }
        XD_CSWAP(0, 1) XD_CSWAP(2, 3) XD_CSWAP(0, 2) XD_CSWAP(1, 3) XD_CSWAP(1, 2)
#undef XD_CSWAP
        double e1[3], e2[3], e3[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double p0 = xs[n[0]][k];
            e1[k] = xs[n[1]][k] - p0;
            e2[k] = xs[n[2]][k] - p0;
            e3[k] = xs[n[3]][k] - p0;
        }
        const double det = e1[0] * (e2[1] * e3[2] - e2[2] * e3[1]) + e1[1] * (e2[2] * e3[0] - e2[0] * e3[2]) +
                           e1[2] * (e2[0] * e3[1] - e2[1] * e3[0]);
        qe[e] = rho * (fabs(det) * (1.0 / 6.0)) * 0.25;
    }
    __syncthreads();
    if (tid < nn) {
        const int p0 = op.lptr[s0 + c + tid], p1 = op.lptr[s0 + c + tid + 1];
        double s = 0.0;
        for (int k = p0; k < p1; ++k) s += qe[ent[k] >> 2];
        slots[op.spos ? op.spos[s0 + tid] : s0 + tid] = s;
    }
}

// ---------------------------------------------------------------- stable step
__global__ void __launch_bounds__(256) k_xd_dt(const double* __restrict__ X, const int64_t* __restrict__ conn,
                                               int64_t M, double cd, double* __restrict__ dte,
                                               double* __restrict__ part) {
    __shared__ double red[256];
    double lo = INFINITY;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < M; e += (int64_t)gridDim.x * 256) {
        double g[4][3];
        (void)tet4_grads(X, conn + 4 * e, g);
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k) s += g[a][k] * g[a][k];
        double t = 1.0 / (cd * sqrt(s));
        if (!(t >= 0.0)) t = 0.0;   // a degenerate element admits no step
        if (dte) dte[e] = t;
        lo = fmin(lo, t);
    }
    red[threadIdx.x] = lo;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(256) k_xd_dt_min(const double* __restrict__ part, int n, double* __restrict__ out) {
    __shared__ double red[256];
    double lo = INFINITY;
    for (int i = threadIdx.x; i < n; i += 256) lo = fmin(lo, part[i]);
    red[threadIdx.x] = lo;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

}  // namespace fem

using namespace fem;

struct fem_xd {
    fem_mf* mf = nullptr;
    int mat = FEM_MAT_LINEAR;
    double rho = 0, alpha = 0;
    int64_t N = 0, nchunks = 0;
    const double* mass = nullptr;
    const uint8_t* mask = nullptr;
    double *u = nullptr, *v = nullptr, *a = nullptr;   // the caller's
    double* vh = nullptr;       // [3N] half-step velocity
    double* slots = nullptr;    // [3 nslots]
    double* epart = nullptr;    // [nchunks]
    double* kpart = nullptr;    // [3 ugrid]
    int32_t* recmap = nullptr;  // [3N], allocated with the first record
    unsigned long long* status = nullptr;   // [2]
    int ugrid = 1;
    int64_t step = 0;
    bool started = false, fresh = true;
    double last_dt = 0.0;
    // the contact set (fem_xd_contact): con.ns == 0 -> none; the surfaces hold their reference points and the
    // velocities a start uses, dt0 the step of a start's penalty stiffness
    XdCon con{};
    double dt0 = 0.0;
    int cgrid = 1;              // workgroups of the contact update (one thread per node)
    double* cpart = nullptr;    // [cgrid, XD_CP], allocated with the first contact set
};

static void xd_free(fem_xd* h) {
    if (!h) return;
    void* ps[] = {h->vh, h->slots, h->epart, h->kpart, h->recmap, h->status, h->cpart};
    for (void* p : ps)
        if (p) (void)hipFree(p);
    delete h;
}

template <bool ENERGY>
static void xd_force_launch(const fem_xd* h, const MfOp& op, const double* u, double* slots, unsigned long long step,
                            hipStream_t st) {
    if (h->nchunks == 0) return;
    const dim3 g((unsigned)h->nchunks), b(XD_BLOCK);
    if (h->mat == FEM_MAT_LINEAR)
        hipLaunchKernelGGL((k_xd_force<FEM_MAT_LINEAR, ENERGY>), g, b, 0, st, op, u, slots, h->epart, h->status, step);
    else if (h->mat == FEM_MAT_SVK)
        hipLaunchKernelGGL((k_xd_force<FEM_MAT_SVK, ENERGY>), g, b, 0, st, op, u, slots, h->epart, h->status, step);
    else
        hipLaunchKernelGGL((k_xd_force<FEM_MAT_NEO_HOOKEAN, ENERGY>), g, b, 0, st, op, u, slots, h->epart, h->status,
                           step);
}

static XdUpd xd_upd(const fem_xd* h, double dt, double amp, const double* fext, unsigned long long step) {
    XdUpd p{};
    p.n3 = 3 * h->N;
    p.dt = dt;
    p.c1 = 1.0 - 0.5 * h->alpha * dt;
    p.c2 = 1.0 / (1.0 + 0.5 * h->alpha * dt);
    p.alpha = h->alpha;
    p.amp = amp;
    p.step = step;
    p.fext = fext;
    p.mass = h->mass;
    p.mask = h->mask;
    p.u = h->u;
    p.vh = h->vh;
    p.v = h->v;
    p.a = h->a;
    p.kpart = h->kpart;
    p.status = h->status;
    return p;
}

// the contact set of one launch: the surfaces moved by off [ns, 3] (null: where they were attached) with the
// velocities vel [ns, 3] (null: those of the attach call)
static XdCon xd_con(const fem_xd* h, double dt, const double* off, const double* vel) {
    XdCon c = h->con;
    c.dt = dt;
    c.cpart = h->cpart;
    for (int s = 0; s < c.ns; ++s)
        for (int q = 0; q < 3; ++q) {
            if (off) c.s[s].c[q] = h->con.s[s].c[q] + off[3 * s + q];
            if (vel) c.s[s].w[q] = vel[3 * s + q];
        }
    return c;
}

template <bool FROMV>
static void xd_step_c_launch(const fem_xd* h, bool en, bool hist, const MfOp& op, const XdUpd& p, const XdCon& c,
                             hipStream_t st) {
    const dim3 g(h->cgrid), b(XD_BLOCK);
    const double* sl = h->slots;
    if (en && hist) hipLaunchKernelGGL((k_xd_update_c<FROMV, true, true, true>), g, b, 0, st, op, p, c, sl);
    else if (en) hipLaunchKernelGGL((k_xd_update_c<FROMV, true, true, false>), g, b, 0, st, op, p, c, sl);
    else if (hist) hipLaunchKernelGGL((k_xd_update_c<FROMV, true, false, true>), g, b, 0, st, op, p, c, sl);
    else hipLaunchKernelGGL((k_xd_update_c<FROMV, true, false, false>), g, b, 0, st, op, p, c, sl);
}

extern "C" {

int fem_xd_lumped_mass(fem_mf* mf, double rho, double* mass, fem_stream_t stream) {
    if (!mf || mf_bs(mf) != 3 || !(rho > 0.0) || (mf_nodes(mf) > 0 && !mass)) {
        set_error("fem_xd_lumped_mass: needs an elastic element-chunk layout, rho > 0 and mass [N]");
        return FEM_EARG;
    }
    const MfOp op = mf_op(mf);
    hipStream_t st = S(stream);
    if (op.nchunks > 0) {
        hipLaunchKernelGGL(k_xd_mass, dim3((unsigned)op.nchunks), dim3(XD_BLOCK), 0, st, op, rho, mf_slots(mf));
        FEM_LAUNCHED();
    }
    if (op.nnodes > 0) {
        hipLaunchKernelGGL(k_mf_gather<1>, dim3(stream_grid(op.nnodes, 256)), dim3(256), 0, st, op,
                           (const double*)mf_slots(mf), mass);
        FEM_LAUNCHED();
    }
    return FEM_OK;
}

int fem_xd_stable_dt(const double* coords, const int64_t* conn, int64_t M, double E, double nu, double rho,
                     double* dt_e, double* dt_min, fem_stream_t stream) {
    if (M < 0 || (M > 0 && (!coords || !conn)) || !dt_min || !(rho > 0.0) || !(E > 0.0) || !(nu > -1.0 && nu < 0.5)) {
        set_error("fem_xd_stable_dt: needs the mesh, dt_min, rho > 0, E > 0 and nu in (-1, 0.5)");
        return FEM_EARG;
    }
    hipStream_t st = S(stream);
    const Lame L = lame(E, nu);
    const double cd = sqrt(((L.lam > 0.0 ? L.lam : 0.0) + 2.0 * L.mu) / rho);   // lam < 0 (nu < 0): the bound holds with 2 mu
    const int grid = stream_grid(M, 256);
    void* part = nullptr;
    FEM_HIP(stream_scratch(&part, sizeof(double) * (size_t)grid, st));
    hipLaunchKernelGGL(k_xd_dt, dim3(grid), dim3(256), 0, st, coords, conn, M, cd, dt_e, (double*)part);
    FEM_LAUNCHED();
    hipLaunchKernelGGL(k_xd_dt_min, dim3(1), dim3(256), 0, st, (const double*)part, grid, dt_min);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_xd_create(fem_mf* mf, int material, double rho, const double* mass, const uint8_t* mask, double alpha,
                  double* u, double* v, double* a, fem_stream_t stream, fem_xd** out) {
    if (!out || !mf || mf_bs(mf) != 3) {
        set_error("fem_xd_create: needs an elastic element-chunk layout (fem_mf_create, FEM_KIND_ELASTIC)");
        return FEM_EARG;
    }
    *out = nullptr;
    if (material != FEM_MAT_LINEAR && material != FEM_MAT_SVK && material != FEM_MAT_NEO_HOOKEAN) {
        set_error("fem_xd_create: unknown material %d", material);
        return FEM_EARG;
    }
    const int64_t N = mf_nodes(mf);
    if (!(rho > 0.0) || !(alpha >= 0.0) || (N > 0 && (!mass || !u || !v || !a))) {
        set_error("fem_xd_create: needs rho > 0, alpha >= 0, the lumped mass [N] and the state u, v, a [3N]");
        return FEM_EARG;
    }
    fem_xd* h = new fem_xd();
    h->mf = mf;
    h->mat = material;
    h->rho = rho;
    h->alpha = alpha;
    h->N = N;
    h->nchunks = mf_op(mf).nchunks;
    h->mass = mass;
    h->mask = mask;
    h->u = u;
    h->v = v;
    h->a = a;
    h->ugrid = stream_grid(3 * N, XD_BLOCK);
    const size_t nsl = (size_t)mf_nslots(mf);
    hipError_t e = hipMalloc(&h->vh, sizeof(double) * (size_t)(3 * N > 0 ? 3 * N : 1));
    if (e == hipSuccess) e = hipMalloc(&h->slots, sizeof(double) * 3 * (nsl > 0 ? nsl : 1));
    if (e == hipSuccess) e = hipMalloc(&h->epart, sizeof(double) * (size_t)(h->nchunks > 0 ? h->nchunks : 1));
    if (e == hipSuccess) e = hipMalloc(&h->kpart, sizeof(double) * 3 * (size_t)h->ugrid);
    if (e == hipSuccess) e = hipMalloc(&h->status, sizeof(unsigned long long) * 2);
    if (e == hipSuccess) e = hipMemsetAsync(h->status, 0xff, sizeof(unsigned long long) * 2, S(stream));
    if (e == hipSuccess) e = hipMemsetAsync(h->vh, 0, sizeof(double) * (size_t)(3 * N > 0 ? 3 * N : 1), S(stream));
    if (e != hipSuccess) {
        set_error("fem_xd_create: %s", hipGetErrorString(e));
        xd_free(h);
        return FEM_EHIP;
    }
    *out = h;
    return FEM_OK;
}

int fem_xd_destroy(fem_xd* h) {
    xd_free(h);
    return FEM_OK;
}

int fem_xd_force(fem_xd* h, const double* u, double* fint, fem_stream_t stream) {
    if (!h || (h->N > 0 && (!u || !fint))) {
        set_error("fem_xd_force: bad arguments");
        return FEM_EARG;
    }
    hipStream_t st = S(stream);
    const MfOp op = mf_op(h->mf);
    xd_force_launch<false>(h, op, u, h->slots, h->started ? (unsigned long long)h->step : 0ull, st);
    FEM_LAUNCHED();
    if (h->N > 0) {
        hipLaunchKernelGGL(k_mf_gather<3>, dim3(stream_grid(h->N, 256)), dim3(256), 0, st, op,
                           (const double*)h->slots, fint);
        FEM_LAUNCHED();
    }
    return FEM_OK;
}

int fem_xd_start(fem_xd* h, const double* u0, const double* v0, const double* fext, double amp0,
                 fem_stream_t stream) {
    if (!h) {
        set_error("fem_xd_start: bad arguments");
        return FEM_EARG;
    }
    hipStream_t st = S(stream);
    const size_t bytes = sizeof(double) * (size_t)(3 * h->N);
    if (bytes) {
        if (u0) FEM_HIP(hipMemcpyAsync(h->u, u0, bytes, hipMemcpyDeviceToDevice, st));
        else FEM_HIP(hipMemsetAsync(h->u, 0, bytes, st));
        if (v0) FEM_HIP(hipMemcpyAsync(h->v, v0, bytes, hipMemcpyDeviceToDevice, st));
        else FEM_HIP(hipMemsetAsync(h->v, 0, bytes, st));
    }
    FEM_HIP(hipMemsetAsync(h->status, 0xff, sizeof(unsigned long long) * 2, st));
    h->step = 0;
    h->started = true;
    h->fresh = true;
    h->last_dt = 0.0;
    if (h->N == 0) return FEM_OK;
    const MfOp op = mf_op(h->mf);
    xd_force_launch<false>(h, op, h->u, h->slots, 0ull, st);
    FEM_LAUNCHED();
    const XdUpd p = xd_upd(h, 0.0, amp0, fext, 0ull);
    if (h->con.ns > 0)
        hipLaunchKernelGGL((k_xd_update_c<true, false, false, false>), dim3(h->cgrid), dim3(XD_BLOCK), 0, st, op, p,
                           xd_con(h, h->dt0, nullptr, nullptr), (const double*)h->slots);
    else
        hipLaunchKernelGGL((k_xd_update<true, false, false>), dim3(h->ugrid), dim3(XD_BLOCK), 0, st, op, p,
                           (const double*)h->slots);
    FEM_LAUNCHED();
    return FEM_OK;
}

}  // extern "C"

// fem_xd_run and fem_xd_run_contact (coff != null: the contact set's offsets and velocities per step)
static int xd_run(fem_xd* h, int64_t nsteps, double dt, const double* amps, const double* fext, int64_t nrec,
                  const int64_t* rec_dofs, double* rec_u, double* rec_v, double* rec_a, int64_t energy_every,
                  double* energies, const double* coff, const double* cvel, int64_t contact_every, double* chist,
                  double* cenergies, fem_stream_t stream) {
    const bool ct = coff != nullptr;
    if (!h || !h->started || nsteps < 0 || !(dt > 0.0) || nrec < 0 || energy_every < 0 ||
        (nsteps > 0 && fext && !amps) || (nrec > 0 && (!rec_dofs || !rec_u || !rec_v || !rec_a)) ||
        (energy_every > 0 && !energies)) {
        set_error("fem_xd_run: needs a started integrator, nsteps >= 0, dt > 0, amps [nsteps + 1] with a load, the "
                  "record arrays with nrec > 0 and the energy rows with energy_every > 0");
        return FEM_EARG;
    }
    if (nsteps == 0 || h->N == 0) {
        h->step += nsteps;
        return FEM_OK;
    }
    hipStream_t st = S(stream);
    const MfOp op = mf_op(h->mf);
    const int64_t n3 = 3 * h->N;
    if (nrec > 0) {
        if (!h->recmap) FEM_HIP(hipMalloc(&h->recmap, sizeof(int32_t) * (size_t)n3));
        FEM_HIP(hipMemsetAsync(h->recmap, 0xff, sizeof(int32_t) * (size_t)n3, st));
        hipLaunchKernelGGL(k_xd_recmap, dim3(stream_grid(nrec, 256)), dim3(256), 0, st, rec_dofs, nrec, h->recmap);
        FEM_LAUNCHED();
    }
    bool fromv = h->fresh || dt != h->last_dt;
    int64_t erow = 0, crow = 0;
    const int ns = h->con.ns;
    const dim3 ug(h->ugrid), ub(XD_BLOCK);
    const double* sl = h->slots;
    for (int64_t k = 0; k < nsteps; ++k) {
        const unsigned long long n = (unsigned long long)(h->step + k);
        const bool en = energy_every > 0 && (h->step + k) % energy_every == 0;
        if (en) xd_force_launch<true>(h, op, h->u, h->slots, n, st);
        else xd_force_launch<false>(h, op, h->u, h->slots, n, st);
        XdUpd p = xd_upd(h, dt, fext ? amps[k] : 0.0, fext, n);
        if (nrec > 0) {
            p.recmap = h->recmap;
            p.ru = rec_u + k * nrec;
            p.rv = rec_v + k * nrec;
            p.ra = rec_a + k * nrec;
        }
        if (ct) {
            const bool hist = contact_every > 0 && (h->step + k) % contact_every == 0;
            const XdCon c = xd_con(h, dt, coff + 3 * ns * k, cvel + 3 * ns * k);
            if (fromv) xd_step_c_launch<true>(h, en, hist, op, p, c, st);
            else xd_step_c_launch<false>(h, en, hist, op, p, c, st);
            if (en) hipLaunchKernelGGL(k_xd_sum, dim3(1), dim3(256), 0, st, (const double*)h->kpart, h->cgrid,
                                       (const double*)h->epart, h->nchunks, energies + XD_NE * erow);
            if (en || hist)
                hipLaunchKernelGGL(k_xd_csum, dim3(1), dim3(256), 0, st, (const double*)h->cpart, h->cgrid, ns,
                                   hist ? chist + XD_NH * ns * crow : nullptr,
                                   en ? cenergies + XD_NCE * erow : nullptr);
            if (en) ++erow;
            if (hist) ++crow;
            fromv = false;
            continue;
        }
        if (fromv) {
            if (en) hipLaunchKernelGGL((k_xd_update<true, true, true>), ug, ub, 0, st, op, p, sl);
            else hipLaunchKernelGGL((k_xd_update<true, true, false>), ug, ub, 0, st, op, p, sl);
        } else {
            if (en) hipLaunchKernelGGL((k_xd_update<false, true, true>), ug, ub, 0, st, op, p, sl);
            else hipLaunchKernelGGL((k_xd_update<false, true, false>), ug, ub, 0, st, op, p, sl);
        }
        if (en) {
            hipLaunchKernelGGL(k_xd_sum, dim3(1), dim3(256), 0, st, (const double*)h->kpart, h->ugrid,
                               (const double*)h->epart, h->nchunks, energies + XD_NE * erow);
            ++erow;
        }
        fromv = false;
    }
    FEM_LAUNCHED();
    h->step += nsteps;
    h->fresh = false;
    h->last_dt = dt;
    // v_n and a_n of the state reached (u and the half-step velocity stay as they are)
    xd_force_launch<false>(h, op, h->u, h->slots, (unsigned long long)h->step, st);
    const XdUpd p = xd_upd(h, dt, fext ? amps[nsteps] : 0.0, fext, (unsigned long long)h->step);
    if (ct)
        hipLaunchKernelGGL((k_xd_update_c<false, false, false, false>), dim3(h->cgrid), ub, 0, st, op, p,
                           xd_con(h, dt, coff + 3 * ns * nsteps, cvel + 3 * ns * nsteps), sl);
    else
        hipLaunchKernelGGL((k_xd_update<false, false, false>), ug, ub, 0, st, op, p, sl);
    FEM_LAUNCHED();
    return FEM_OK;
}

extern "C" {

int fem_xd_run(fem_xd* h, int64_t nsteps, double dt, const double* amps, const double* fext, int64_t nrec,
               const int64_t* rec_dofs, double* rec_u, double* rec_v, double* rec_a, int64_t energy_every,
               double* energies, fem_stream_t stream) {
    if (h && h->con.ns > 0 && h->N > 0) {
        set_error("fem_xd_run: a contact set is attached; fem_xd_run_contact takes its surface motion");
        return FEM_EARG;
    }
    return xd_run(h, nsteps, dt, amps, fext, nrec, rec_dofs, rec_u, rec_v, rec_a, energy_every, energies, nullptr,
                  nullptr, 0, nullptr, nullptr, stream);
}

int fem_xd_run_contact(fem_xd* h, int64_t nsteps, double dt, const double* amps, const double* fext, int64_t nrec,
                       const int64_t* rec_dofs, double* rec_u, double* rec_v, double* rec_a, int64_t energy_every,
                       double* energies, const double* offsets, const double* velocities, int64_t contact_every,
                       double* history, double* contact_energies, fem_stream_t stream) {
    if (!h || h->con.ns <= 0 || !offsets || !velocities || contact_every < 0 || (contact_every > 0 && !history) ||
        (energy_every > 0 && !contact_energies)) {
        set_error("fem_xd_run_contact: needs an integrator with a contact set (fem_xd_contact), the offsets and "
                  "velocities [nsteps + 1, surfaces, 3], the history rows with contact_every > 0 and the contact "
                  "energy rows with energy_every > 0");
        return FEM_EARG;
    }
    return xd_run(h, nsteps, dt, amps, fext, nrec, rec_dofs, rec_u, rec_v, rec_a, energy_every, energies, offsets,
                  velocities, contact_every, history, contact_energies, stream);
}

int fem_xd_contact(fem_xd* h, int64_t nsurf, const double* surfaces, double kappa, double dt0,
                   const uint8_t* node_word, fem_stream_t stream) {
    (void)stream;
    if (!h || nsurf < 0 || nsurf > XD_MAXS) {
        set_error("fem_xd_contact: needs an integrator and 0 .. %d surfaces", XD_MAXS);
        return FEM_EARG;
    }
    if (nsurf == 0) {
        h->con = XdCon{};
        return FEM_OK;
    }
    if (!surfaces || !(kappa > 0.0 && kappa < 4.0) || !(dt0 > 0.0)) {
        set_error("fem_xd_contact: needs the surface table [nsurf, %d], 0 < kappa < 4 and dt0 > 0", XD_SV);
        return FEM_EARG;
    }
    XdCon c{};
    c.ns = (int)nsurf;
    c.kappa = kappa;
    c.word = node_word;
    for (int s = 0; s < c.ns; ++s) {
        const double* r = surfaces + XD_SV * s;
        XdSurf& S = c.s[s];
        S.kind = (int)r[0];
        S.inside = r[1] != 0.0;
        double nn = 0.0;
        for (int q = 0; q < 3; ++q) {
            S.c[q] = r[2 + q];
            S.n[q] = r[5 + q];
            S.w[q] = r[10 + q];
            nn += S.n[q] * S.n[q];
        }
        S.R = r[8];
        S.mu = r[9];
        const bool round = S.kind == FEM_SURF_SPHERE || S.kind == FEM_SURF_CYLINDER;
        if ((S.kind != FEM_SURF_PLANE && !round) || (double)S.kind != r[0] || !(S.mu >= 0.0) ||
            (round && !(S.R > 0.0)) || (S.kind != FEM_SURF_SPHERE && !(fabs(nn - 1.0) <= 1e-12))) {
            set_error("fem_xd_contact: surface %d needs a known kind, a unit normal or axis, a radius > 0 and mu >= 0", s);
            return FEM_EARG;
        }
    }
    if (!h->cpart) {
        h->cgrid = stream_grid(h->N, XD_BLOCK);
        FEM_HIP(hipMalloc(&h->cpart, sizeof(double) * XD_CP * (size_t)h->cgrid));
    }
    h->con = c;
    h->dt0 = dt0;
    return FEM_OK;
}

int fem_xd_status(fem_xd* h, int64_t* out2, fem_stream_t stream) {
    if (!h || !out2) {
        set_error("fem_xd_status: bad arguments");
        return FEM_EARG;
    }
    unsigned long long w[2];
    FEM_HIP(hipMemcpyAsync(w, h->status, sizeof(w), hipMemcpyDeviceToHost, S(stream)));
    FEM_HIP(hipStreamSynchronize(S(stream)));
    out2[0] = w[0] == XD_NONE ? -1 : (int64_t)w[0];
    out2[1] = w[1] == XD_NONE ? -1 : (int64_t)w[1];
    return FEM_OK;
}

int fem_xd_info(fem_xd* h, int64_t* out4) {
    if (!h || !out4) {
        set_error("fem_xd_info: bad arguments");
        return FEM_EARG;
    }
    out4[0] = h->step;
    out4[1] = h->nchunks;
    out4[2] = h->ugrid;
    out4[3] = XD_NE;
    return FEM_OK;
}

}  // extern "C"
