// Flat shell elements s3 / s4 (6 dofs per node: u, v, w, thx, thy, thz) on gfx950 -- the element matrices, geometry,
// element-by-element operator and stress resultants of the reference's `solver/shell.py`, quirks included:
//   frame   node 0 is the origin, a = edge 0->1 normalised, b = edge 0->2 (s3) / 0->3 (s4) made orthogonal to a and
//           normalised, c = a x b; unit = [a; b; c]; local = (x - x0) unit^T, of which only x and y are used
//   grads   J = [[dx/dxi, dx/deta], [dy/dxi, dy/deta]], (dN/dx, dN/dy)_n = J^-1 (dN_n/dxi, dN_n/deta) -- the reference's
//           contraction, with J^-1 and not its transpose
//   B       membrane rows on local (u, v); bending rows on local (thx, thy) only: kx = -dN/dx thy, ky = dN/dy thx,
//           kxy = dN/dy thx + dN/dx thy. The columns of w and thz are zero: translations and rotations are uncoupled
//   K       s3: B^T D B detJ / 2 (signed detJ); s4: sum over the four 2x2 Gauss points of w detJ B^T D B
// B^T D B is never formed as a dense triple product: the element matrix is a membrane block on (u, v) and a bending
// block on (thx, thy), each 2 npe square, and every other entry is written as an exact zero.
#include <math.h>

#include "common.hpp"

namespace fem {

// the four factors (1 - xi, 1 + xi, 1 - eta, 1 + eta) of each s4 integration point, formed on the host the way the
// reference forms them (its K uses the fp32-rounded 1/sqrt(3) widened to fp64, its summed B rounds the factors to fp32)
struct ShellPts {
    double f[4][4];
};

// D = blockdiag(membrane, bending): (D00 = D11, D01, D22) of each 3x3 block
struct ShellD {
    double m[3];
    double b[3];
};

// frame and local coordinates of one element; false for a zero edge 0->1 or a collinear frame. Collinear: what is left
// of b after removing its part along a is below 1e-12 |b| (an exactly collinear b leaves rounding of ~1e-16 |b|).
template <int NPE>
__device__ __forceinline__ bool shell_frame(const double* __restrict__ X, const int64_t* __restrict__ n, double* U,
                                            double* lx, double* ly, double* lz) {
#pragma clang fp contract(off)
    double x[NPE][3];
#pragma unroll
    for (int a = 0; a < NPE; ++a)
#pragma unroll
        for (int j = 0; j < 3; ++j) x[a][j] = X[3 * n[a] + j];
    double av[3], bv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        av[j] = x[1][j] - x[0][j];
        bv[j] = x[NPE - 1][j] - x[0][j];
    }
    const double aa0 = (av[0] * av[0] + av[1] * av[1]) + av[2] * av[2];
    const double bb0 = (bv[0] * bv[0] + bv[1] * bv[1]) + bv[2] * bv[2];
    bool ok = aa0 > 0.0 && aa0 < INFINITY;
    if (NPE == 4) {   // s4 normalises a before the projection, s3 after it
        const double na = sqrt(aa0);
#pragma unroll
        for (int j = 0; j < 3; ++j) av[j] = av[j] / na;
    }
    const double ab = (av[0] * bv[0] + av[1] * bv[1]) + av[2] * bv[2];
    const double aa = (av[0] * av[0] + av[1] * av[1]) + av[2] * av[2];
    const double s = ab / aa;
#pragma unroll
    for (int j = 0; j < 3; ++j) bv[j] = bv[j] - s * av[j];
    if (NPE == 3) {
        const double na = sqrt(aa);
#pragma unroll
        for (int j = 0; j < 3; ++j) av[j] = av[j] / na;
    }
    const double bb = (bv[0] * bv[0] + bv[1] * bv[1]) + bv[2] * bv[2];
    ok = ok && bb > 1e-24 * bb0 && bb < INFINITY;
    const double nb = sqrt(bb);
#pragma unroll
    for (int j = 0; j < 3; ++j) bv[j] = bv[j] / nb;
    U[0] = av[0], U[1] = av[1], U[2] = av[2];
    U[3] = bv[0], U[4] = bv[1], U[5] = bv[2];
    U[6] = av[1] * bv[2] - av[2] * bv[1];
    U[7] = av[2] * bv[0] - av[0] * bv[2];
    U[8] = av[0] * bv[1] - av[1] * bv[0];
#pragma unroll
    for (int a = 0; a < NPE; ++a) {
        const double v0 = x[a][0] - x[0][0], v1 = x[a][1] - x[0][1], v2 = x[a][2] - x[0][2];
        lx[a] = (v0 * U[0] + v1 * U[1]) + v2 * U[2];
        ly[a] = (v0 * U[3] + v1 * U[4]) + v2 * U[5];
        if (lz) lz[a] = (v0 * U[6] + v1 * U[7]) + v2 * U[8];
    }
    return ok;
}

// J (row-major 2x2), dN/dx, dN/dy at one point (f: the point's four factors; unused for s3) -> det J
template <int NPE>
__device__ __forceinline__ double shell_grads(const double* lx, const double* ly, const double* f, double* J,
                                              double* dx, double* dy) {
#pragma clang fp contract(off)
    double dxi[NPE], det[NPE];
    if (NPE == 3) {
        dxi[0] = -1.0, dxi[1] = 1.0, dxi[2] = 0.0;
        det[0] = -1.0, det[1] = 0.0, det[2] = 1.0;
    } else {
        dxi[0] = 0.25 * -f[2], dxi[1] = 0.25 * f[2], dxi[2] = 0.25 * f[3], dxi[NPE - 1] = 0.25 * -f[3];
        det[0] = 0.25 * -f[0], det[1] = 0.25 * -f[1], det[2] = 0.25 * f[1], det[NPE - 1] = 0.25 * f[0];
    }
    double j00 = 0.0, j01 = 0.0, j10 = 0.0, j11 = 0.0;
#pragma unroll
    for (int a = 0; a < NPE; ++a) {
        j00 += dxi[a] * lx[a];
        j01 += det[a] * lx[a];
        j10 += dxi[a] * ly[a];
        j11 += det[a] * ly[a];
    }
    J[0] = j00, J[1] = j01, J[2] = j10, J[3] = j11;
    const double dj = j00 * j11 - j01 * j10;
    const double i00 = j11 / dj, i01 = -j01 / dj, i10 = -j10 / dj, i11 = j00 / dj;
#pragma unroll
    for (int a = 0; a < NPE; ++a) {
        dx[a] = i00 * dxi[a] + i01 * det[a];
        dy[a] = i10 * dxi[a] + i11 * det[a];
    }
    return dj;
}

__device__ __forceinline__ bool shell_det_ok(double dj) { return dj != 0.0 && fabs(dj) < INFINITY; }

// ------------------------------------------------------------------ element matrices
enum { SHELL_LOCAL = 0, SHELL_POINTS = 1, SHELL_GLOBAL = 2 };

template <int NPE>
struct ShellRec {
    static constexpr int NP = NPE == 3 ? 1 : 4;
    static constexpr int PT = 2 * NPE + 1;           // per point: dN/dx [NPE], dN/dy [NPE], weight * detJ
    static constexpr int UNIT = NP * PT;             // then unit [9]
    static constexpr int LEN = (UNIT + 9) | 1;       // odd stride
};

// the strain column of local dof c (0: u, 1: v, 3: thx, 4: thy) of a node with gradients (dx, dy), in its 3x3 block
__device__ __forceinline__ void shell_col(int c, double dx, double dy, double* v) {
    v[0] = c == 0 ? dx : (c == 4 ? -dx : 0.0);
    v[1] = (c == 1 || c == 3) ? dy : 0.0;
    v[2] = c == 0 ? dy : (c == 3 ? dy : dx);
}

// B_(a,c)^T D B_(b,d) at one point from the two nodes' gradients (Dm: the membrane or bending triple of D). Products
// are not fused into sums and every product and sum is symmetric in (a, c) <-> (b, d), so the element matrices are
// exactly symmetric.
__device__ __forceinline__ double shell_term(int c, int d, double dxa, double dya, double dxb, double dyb,
                                             const double* Dm) {
#pragma clang fp contract(off)
    double va[3], vb[3];
    shell_col(c, dxa, dya, va);
    shell_col(d, dxb, dyb, vb);
    return (Dm[0] * (va[0] * vb[0]) + Dm[1] * (va[0] * vb[1] + va[1] * vb[0])) +
           (Dm[0] * (va[1] * vb[1]) + Dm[2] * (va[2] * vb[2]));
}

// entry (6 a + c, 6 b + d) of the local element matrix from the element's record, points [p0, p1)
template <int NPE>
__device__ __forceinline__ double shell_entry(const double* __restrict__ r, const ShellD& D, int a, int c, int b, int d,
                                              int p0, int p1) {
#pragma clang fp contract(off)
    const bool mem = c < 2 && d < 2;
    const bool ben = (c == 3 || c == 4) && (d == 3 || d == 4);
    if (!mem && !ben) return 0.0;
    const double* Dm = mem ? D.m : D.b;
    double s = 0.0;
    for (int p = p0; p < p1; ++p) {
        const double* q = r + p * ShellRec<NPE>::PT;
        s += shell_term(c, d, q[a], q[NPE + a], q[b], q[NPE + b], Dm) * q[2 * NPE];
    }
    return s;
}

// Global-frame record: the summed 2x2 local blocks K[(a, c'), (b, d')] of the node pairs a <= b, membrane (h = 0,
// dofs u, v) then bending (h = 1, dofs thx, thy), at ((h NPAIR + pair) 4 + 2 c' + d'), then unit [9]. The values are
// shell_entry's bit for bit (same terms, same order over the points).
template <int NPE>
struct ShellGRec {
    static constexpr int NPAIR = NPE * (NPE + 1) / 2;
    static constexpr int UNIT = 8 * NPAIR;
    static constexpr int LEN = (UNIT + 9) | 1;
    __host__ __device__ static constexpr int pair(int a, int b) { return a * NPE - a * (a - 1) / 2 + (b - a); }
};

// 64 elements per 256-thread block (the shape of k_tet4_ke / k_tet4_nl): 64 lanes form the records into LDS, then all
// 256 threads write the block's contiguous values coalesced. The local forms keep the gradients and form each entry
// while writing; the global form keeps the summed 2x2 blocks (ShellGRec), so each of its entries is four products.
//   SHELL_LOCAL   Ke [M, d, d], d = 6 NPE, rows 6 n + (u, v, w, thx, thy, thz) in the element's frame
//   SHELL_POINTS  Ke [M, d, d, 4]: the four integration points' terms (s4)
//   SHELL_GLOBAL  Ke [M, d, d] = T^T K T in the block order of the 6-dof assembly: rows 3 (h NPE + n) + i, h = 0 the
//                 translations and h = 1 the rotations of node n, i the global axis
template <int NPE, int MODE>
__global__ void __launch_bounds__(256) k_shell_ke(const double* __restrict__ X, const int64_t* __restrict__ conn,
                                                  int64_t M, ShellD D, ShellPts P, double* __restrict__ Ke,
                                                  double* __restrict__ unit, int64_t* __restrict__ bad) {
    using R = ShellRec<NPE>;
    using G = ShellGRec<NPE>;
    constexpr int LEN = MODE == SHELL_GLOBAL ? G::LEN : R::LEN;
    constexpr int UNIT = MODE == SHELL_GLOBAL ? G::UNIT : R::UNIT;
    __shared__ double rec_s[64 * LEN];
    const int64_t e0 = (int64_t)blockIdx.x * 64;
    if (threadIdx.x < 64 && e0 + threadIdx.x < M) {
        const int64_t e = e0 + threadIdx.x;
        double* r = rec_s + threadIdx.x * LEN;
        int64_t n[NPE];
#pragma unroll
        for (int a = 0; a < NPE; ++a) n[a] = conn[NPE * e + a];
        double U[9], lx[NPE], ly[NPE];
        bool ok = shell_frame<NPE>(X, n, U, lx, ly, nullptr);
        double gx[R::NP][NPE], gy[R::NP][NPE], wd[R::NP];
#pragma unroll
        for (int p = 0; p < R::NP; ++p) {
            double J[4];
            const double dj = shell_grads<NPE>(lx, ly, P.f[p], J, gx[p], gy[p]);
            ok = ok && shell_det_ok(dj);
            wd[p] = NPE == 3 ? dj * 0.5 : dj;   // the s4 weights are 1
        }
        if (MODE == SHELL_GLOBAL) {
#pragma clang fp contract(off)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int a = 0; a < NPE; ++a)
#pragma unroll
                    for (int b = a; b < NPE; ++b)
#pragma unroll
                        for (int cd = 0; cd < 4; ++cd) {
                            double v = 0.0;
#pragma unroll
                            for (int p = 0; p < R::NP; ++p)
                                v += shell_term(3 * h + (cd >> 1), 3 * h + (cd & 1), gx[p][a], gy[p][a], gx[p][b],
                                                gy[p][b], h ? D.b : D.m) * wd[p];
                            r[(h * G::NPAIR + G::pair(a, b)) * 4 + cd] = v;
                        }
        } else {
#pragma unroll
            for (int p = 0; p < R::NP; ++p) {
#pragma unroll
                for (int a = 0; a < NPE; ++a) {
                    r[p * R::PT + a] = gx[p][a];
                    r[p * R::PT + NPE + a] = gy[p][a];
                }
                r[p * R::PT + 2 * NPE] = wd[p];
            }
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) r[UNIT + t] = U[t];
        if (!ok) {   // a degenerate element: reported, and zeros instead of inf / NaN in its outputs
            atomicMin((unsigned long long*)bad, (unsigned long long)e);
            for (int t = 0; t < UNIT + 9; ++t) r[t] = 0.0;
        }
    }
    __syncthreads();
    const int nel = (int)min((int64_t)64, M - e0);
    constexpr int DIM = 6 * NPE;
    constexpr int PS = DIM * DIM * (MODE == SHELL_POINTS ? 4 : 1);
    if (Ke) {
        double* out = Ke + e0 * PS;
        for (int t = threadIdx.x; t < nel * PS; t += 256) {
            const int le = t / PS;
            int q = t - le * PS;
            const double* r = rec_s + le * LEN;
            double v;
            if (MODE == SHELL_GLOBAL) {
#pragma clang fp contract(off)
                const int row = q / DIM, col = q - DIM * (q / DIM);
                const int ra = row / 3, i = row - 3 * ra, cb = col / 3, k = col - 3 * cb;
                const int ha = ra / NPE, a = ra - NPE * ha, hb = cb / NPE, b = cb - NPE * hb;
                v = 0.0;
                if (ha == hb) {   // a block below the diagonal reads its transpose's record
                    const bool low = a > b;
                    const double* kb = r + (ha * G::NPAIR + (low ? G::pair(b, a) : G::pair(a, b))) * 4;
                    const double* U = r + UNIT;
                    const double t00 = (U[i] * U[k]) * kb[0];
                    const double t01 = (U[i] * U[3 + k]) * kb[low ? 2 : 1];
                    const double t10 = (U[3 + i] * U[k]) * kb[low ? 1 : 2];
                    const double t11 = (U[3 + i] * U[3 + k]) * kb[3];
                    v = (t00 + (t01 + t10)) + t11;
                }
            } else {
                int p0 = 0, p1 = R::NP;
                if (MODE == SHELL_POINTS) {
                    p0 = q & 3;
                    p1 = p0 + 1;
                    q >>= 2;
                }
                const int row = q / DIM, col = q - DIM * (q / DIM);
                const int a = row / 6, b = col / 6;
                v = shell_entry<NPE>(r, D, a, row - 6 * a, b, col - 6 * b, p0, p1);
            }
            out[t] = v;
        }
    }
    if (unit) {
        double* out = unit + e0 * 9;
        for (int t = threadIdx.x; t < nel * 9; t += 256) {
            const int le = t / 9;
            out[t] = rec_s[le * LEN + UNIT + (t - 9 * le)];
        }
    }
}

// ------------------------------------------------------------------ geometry at one parametric point
// unit [M,3,3], local [M,NPE,3], J [M,2,2], grads [M,NPE,2], B [M,6,6 NPE]; every output may be NULL
template <int NPE>
__global__ void __launch_bounds__(256) k_shell_geom(const double* __restrict__ X, const int64_t* __restrict__ conn,
                                                    int64_t M, ShellPts P, double* __restrict__ unit,
                                                    double* __restrict__ local, double* __restrict__ Jo,
                                                    double* __restrict__ grads, double* __restrict__ B,
                                                    int64_t* __restrict__ bad) {
    constexpr int DIM = 6 * NPE;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < M; e += (int64_t)gridDim.x * blockDim.x) {
        int64_t n[NPE];
#pragma unroll
        for (int a = 0; a < NPE; ++a) n[a] = conn[NPE * e + a];
        double U[9], lx[NPE], ly[NPE], lz[NPE], J[4], dx[NPE], dy[NPE];
        bool ok = shell_frame<NPE>(X, n, U, lx, ly, lz);
        const double dj = shell_grads<NPE>(lx, ly, P.f[0], J, dx, dy);
        if (Jo || grads || B) ok = ok && shell_det_ok(dj);
        if (!ok) {
            if (bad) atomicMin((unsigned long long*)bad, (unsigned long long)e);
#pragma unroll
            for (int t = 0; t < 9; ++t) U[t] = 0.0;
#pragma unroll
            for (int a = 0; a < NPE; ++a) lx[a] = ly[a] = lz[a] = dx[a] = dy[a] = 0.0;
            J[0] = J[1] = J[2] = J[3] = 0.0;
        }
        if (unit) {
#pragma unroll
            for (int t = 0; t < 9; ++t) unit[9 * e + t] = U[t];
        }
        if (local) {
#pragma unroll
            for (int a = 0; a < NPE; ++a) {
                local[(e * NPE + a) * 3] = lx[a];
                local[(e * NPE + a) * 3 + 1] = ly[a];
                local[(e * NPE + a) * 3 + 2] = lz[a];
            }
        }
        if (Jo) {
#pragma unroll
            for (int t = 0; t < 4; ++t) Jo[4 * e + t] = J[t];
        }
        if (grads) {
#pragma unroll
            for (int a = 0; a < NPE; ++a) {
                grads[(e * NPE + a) * 2] = dx[a];
                grads[(e * NPE + a) * 2 + 1] = dy[a];
            }
        }
        if (B) {
            double* Be = B + e * 6 * DIM;
            for (int t = 0; t < 6 * DIM; ++t) Be[t] = 0.0;
#pragma unroll
            for (int a = 0; a < NPE; ++a) {
                Be[0 * DIM + 6 * a] = dx[a];
                Be[1 * DIM + 6 * a + 1] = dy[a];
                Be[2 * DIM + 6 * a] = dy[a];
                Be[2 * DIM + 6 * a + 1] = dx[a];
                Be[3 * DIM + 6 * a + 4] = -dx[a];
                Be[4 * DIM + 6 * a + 3] = dy[a];
                Be[5 * DIM + 6 * a + 3] = dy[a];
                Be[5 * DIM + 6 * a + 4] = dx[a];
            }
        }
    }
}

// ------------------------------------------------------------------ element-by-element operator
// y [N,6] = sum_e R_e^T K_e R_e u: one thread per node walks the node's incidence list in ascending (element, local)
// order (k_ebe_apply's order), so y is the same bits on every run and no atomics are used. K_e is the local-frame
// matrix as given (all 6 rows of the node, all 6 NPE columns), R_e rotates translations and rotations with unit_e.
template <int NPE>
__global__ void __launch_bounds__(256) k_shell_apply(const double* __restrict__ Ke, const double* __restrict__ unit,
                                                     const int64_t* __restrict__ conn,
                                                     const int32_t* __restrict__ inc_ptr,
                                                     const int32_t* __restrict__ inc, int64_t N,
                                                     const double* __restrict__ u, double* __restrict__ y) {
    constexpr int DIM = 6 * NPE;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int t = inc_ptr[i]; t < inc_ptr[i + 1]; ++t) {
            const int ea = inc[t];
            const int64_t e = ea / NPE;
            const int a = ea - (int)e * NPE;
            const double* Krow = Ke + e * DIM * DIM + (int64_t)(6 * a) * DIM;
            double U[9];
#pragma unroll
            for (int s = 0; s < 9; ++s) U[s] = unit[9 * e + s];
            double f[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int b = 0; b < NPE; ++b) {
                const int64_t j = conn[e * NPE + b];
                double ul[6];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const double g0 = u[6 * j + 3 * h], g1 = u[6 * j + 3 * h + 1], g2 = u[6 * j + 3 * h + 2];
#pragma unroll
                    for (int c = 0; c < 3; ++c) ul[3 * h + c] = (g0 * U[3 * c] + g1 * U[3 * c + 1]) + g2 * U[3 * c + 2];
                }
#pragma unroll
                for (int c = 0; c < 6; ++c)
#pragma unroll
                    for (int r = 0; r < 6; ++r) f[r] += Krow[r * DIM + 6 * b + c] * ul[c];
            }
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    acc[3 * h + k] += (U[k] * f[3 * h] + U[3 + k] * f[3 * h + 1]) + U[6 + k] * f[3 * h + 2];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) y[6 * i + r] = acc[r];
    }
}

// ------------------------------------------------------------------ stress resultants
// NMQ [M,6] = D B u_e with B summed over the integration points (s4) and u_e the element's rows of u [N,6] as they
// are -- the reference applies its local-frame B to the global displacement rows (`solver/shell.py:455-468,863-876`)
template <int NPE>
__global__ void __launch_bounds__(256) k_shell_stress(const double* __restrict__ X, const int64_t* __restrict__ conn,
                                                      int64_t M, ShellD D, ShellPts P, const double* __restrict__ u,
                                                      double* __restrict__ nmq, int64_t* __restrict__ bad) {
    constexpr int NP = NPE == 3 ? 1 : 4;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < M; e += (int64_t)gridDim.x * blockDim.x) {
        int64_t n[NPE];
#pragma unroll
        for (int a = 0; a < NPE; ++a) n[a] = conn[NPE * e + a];
        double U[9], lx[NPE], ly[NPE], sx[NPE], sy[NPE];
        bool ok = shell_frame<NPE>(X, n, U, lx, ly, nullptr);
#pragma unroll
        for (int a = 0; a < NPE; ++a) sx[a] = sy[a] = 0.0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            double J[4], dx[NPE], dy[NPE];
            ok = ok && shell_det_ok(shell_grads<NPE>(lx, ly, P.f[p], J, dx, dy));
#pragma unroll
            for (int a = 0; a < NPE; ++a) {
                sx[a] += dx[a];
                sy[a] += dy[a];
            }
        }
        double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (ok) {
            double eps[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int a = 0; a < NPE; ++a) {
                const double* ua = u + 6 * n[a];
                eps[0] += sx[a] * ua[0];
                eps[1] += sy[a] * ua[1];
                eps[2] += sy[a] * ua[0] + sx[a] * ua[1];
                eps[3] += -sx[a] * ua[4];
                eps[4] += sy[a] * ua[3];
                eps[5] += sy[a] * ua[3] + sx[a] * ua[4];
            }
            s[0] = D.m[0] * eps[0] + D.m[1] * eps[1];
            s[1] = D.m[1] * eps[0] + D.m[0] * eps[1];
            s[2] = D.m[2] * eps[2];
            s[3] = D.b[0] * eps[3] + D.b[1] * eps[4];
            s[4] = D.b[1] * eps[3] + D.b[0] * eps[4];
            s[5] = D.b[2] * eps[5];
        } else {
            atomicMin((unsigned long long*)bad, (unsigned long long)e);
        }
#pragma unroll
        for (int t = 0; t < 6; ++t) nmq[6 * e + t] = s[t];
    }
}

static bool shell_args(const char* what, int npe, const double* D6, const double* pts, ShellD* D, ShellPts* P) {
    if (npe != 3 && npe != 4) {
        set_error("%s: %d nodes per element (3: s3, 4: s4)", what, npe);
        return false;
    }
    if (D) {
        if (!D6) {
            set_error("%s: D6 is required", what);
            return false;
        }
        for (int t = 0; t < 3; ++t) D->m[t] = D6[t], D->b[t] = D6[3 + t];
    }
    memset(P, 0, sizeof(*P));
    if (npe == 4) {
        if (!pts) {
            set_error("%s: the s4 integration point factors are required", what);
            return false;
        }
        memcpy(P->f, pts, sizeof(P->f));
    }
    return true;
}

}  // namespace fem

using namespace fem;

extern "C" {

int fem_shell_ke(const double* coords, const int64_t* conn, int64_t M, int npe, const double* D6, const double* pts,
                 int frame, double* Ke, double* unit, int64_t* bad_idx, fem_stream_t stream) {
    ShellD D;
    ShellPts P;
    if (!shell_args("fem_shell_ke", npe, D6, pts, &D, &P)) return FEM_EARG;
    if (frame != FEM_SHELL_LOCAL && frame != FEM_SHELL_POINTS && frame != FEM_SHELL_GLOBAL) {
        set_error("fem_shell_ke: unknown frame %d", frame);
        return FEM_EARG;
    }
    if (frame == FEM_SHELL_POINTS && npe != 4) {
        set_error("fem_shell_ke: per-point matrices are an s4 output");
        return FEM_EARG;
    }
    if (M <= 0) return FEM_OK;
    if (!bad_idx) {
        set_error("fem_shell_ke: bad_idx is required");
        return FEM_EARG;
    }
    const dim3 g((unsigned)cdiv(M, 64));
#define FEM_SK(NPE_, MODE_)                                                                                          \
    hipLaunchKernelGGL((k_shell_ke<NPE_, MODE_>), g, dim3(256), 0, S(stream), coords, conn, M, D, P, Ke, unit, bad_idx)
    if (npe == 3) {
        if (frame == FEM_SHELL_GLOBAL) FEM_SK(3, SHELL_GLOBAL);
        else FEM_SK(3, SHELL_LOCAL);
    } else {
        if (frame == FEM_SHELL_GLOBAL) FEM_SK(4, SHELL_GLOBAL);
        else if (frame == FEM_SHELL_POINTS) FEM_SK(4, SHELL_POINTS);
        else FEM_SK(4, SHELL_LOCAL);
    }
#undef FEM_SK
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_shell_geom(const double* coords, const int64_t* conn, int64_t M, int npe, const double* pt, double* unit,
                   double* local, double* J, double* grads, double* B, int64_t* bad_idx, fem_stream_t stream) {
    ShellPts P;
    memset(&P, 0, sizeof(P));
    if (npe != 3 && npe != 4) {
        set_error("fem_shell_geom: %d nodes per element (3: s3, 4: s4)", npe);
        return FEM_EARG;
    }
    if (npe == 4 && (J || grads || B)) {
        if (!pt) {
            set_error("fem_shell_geom: the s4 point factors are required");
            return FEM_EARG;
        }
        memcpy(P.f[0], pt, sizeof(P.f[0]));
    }
    if (M <= 0) return FEM_OK;
    const dim3 g(stream_grid(M, 256));
    if (npe == 3)
        hipLaunchKernelGGL(k_shell_geom<3>, g, dim3(256), 0, S(stream), coords, conn, M, P, unit, local, J, grads, B,
                           bad_idx);
    else
        hipLaunchKernelGGL(k_shell_geom<4>, g, dim3(256), 0, S(stream), coords, conn, M, P, unit, local, J, grads, B,
                           bad_idx);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_shell_apply(const double* Ke, const double* unit, const int64_t* conn, int npe, const int32_t* inc_ptr,
                    const int32_t* inc, int64_t N, const double* u, double* y, fem_stream_t stream) {
    if (npe != 3 && npe != 4) {
        set_error("fem_shell_apply: %d nodes per element (3: s3, 4: s4)", npe);
        return FEM_EARG;
    }
    if (N <= 0) return FEM_OK;
    const dim3 g(stream_grid(N, 256));
    if (npe == 3)
        hipLaunchKernelGGL(k_shell_apply<3>, g, dim3(256), 0, S(stream), Ke, unit, conn, inc_ptr, inc, N, u, y);
    else
        hipLaunchKernelGGL(k_shell_apply<4>, g, dim3(256), 0, S(stream), Ke, unit, conn, inc_ptr, inc, N, u, y);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_shell_stress(const double* coords, const int64_t* conn, int64_t M, int npe, const double* D6, const double* pts,
                     const double* u, double* nmq, int64_t* bad_idx, fem_stream_t stream) {
    ShellD D;
    ShellPts P;
    if (!shell_args("fem_shell_stress", npe, D6, pts, &D, &P)) return FEM_EARG;
    if (M <= 0) return FEM_OK;
    if (!bad_idx) {
        set_error("fem_shell_stress: bad_idx is required");
        return FEM_EARG;
    }
    const dim3 g(stream_grid(M, 256));
    if (npe == 3)
        hipLaunchKernelGGL(k_shell_stress<3>, g, dim3(256), 0, S(stream), coords, conn, M, D, P, u, nmq, bad_idx);
    else
        hipLaunchKernelGGL(k_shell_stress<4>, g, dim3(256), 0, S(stream), coords, conn, M, D, P, u, nmq, bad_idx);
    FEM_LAUNCHED();
    return FEM_OK;
}

}  // extern "C"
