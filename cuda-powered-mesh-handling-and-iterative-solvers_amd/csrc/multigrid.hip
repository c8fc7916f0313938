// Geometric multigrid PCG on a nested hierarchy of c3d4 meshes (topology.refine_c3d4): z = V(degree, degree)-cycle(r)
// as the preconditioner of MODE_PCG's iteration. Level 0 is the coarsest mesh, level L - 1 the matrix being solved.
// Every level l carries its own assembled matrix A_l (plain SELL-64 of include/fem355.h, int32 `cols` or 16-bit
// `dcols`, bs = 1 or 3), the masked Jacobi weights w_l (zero on the fixed dofs: the project's convention, the matrix is
// untouched) and, above level 0, parents_l [N_l, 2] int32: node i of level l is 0.5 (a + b) of level l - 1, a == b for
// a node carried over. That is the whole prolongation P_l; child_ptr_l [N_{l-1} + 1] / child_l list for every node c
// of level l - 1 the nodes of level l that name it, ascending, once per occurrence (a carried node twice), so that the
// restriction P_l^T is a gather in list order.
//
// Rules of the file (those of pcg_coarse.hip): plain launches on the caller's stream, no workgroup waits on another,
// no floating-point atomics, every reduction finished in a fixed order that depends on the sizes only (bit-identical
// run to run), rows >= nrows never read or stored, matrix values read with nontemporal loads, a device `halt` word that
// turns the remaining kernels of a chunk into no-ops, the host reads the state once per chunk.
//
// The smoother is Chebyshev on diag(w) A over [lmax boost / ratio, lmax boost], in the residual-update form: with
// theta, delta the interval's centre and half width, sigma = theta / delta, rho_0 = 1 / sigma,
//   d_0 = (1 / theta) w o r,   rho_k = 1 / (2 sigma - rho_{k-1}),
//   r -= A d_{k-1},   d_k = rho_k rho_{k-1} d_{k-1} + (2 rho_k / delta) w o r,   x += d_k.
// The host passes c1[l][k] = rho_k rho_{k-1} (0 for k = 0) and c2[l][k] = 2 rho_k / delta (1 / theta for k = 0).
//   k_mg_first   : the first sweep of a pre-smoother, from x = 0: d = c2 w o r, x = d (no matrix)
//   k_mg_cheb    : one sweep fused with the matrix pass: row i reads d_old through its columns,
//                  r_i -= (A d_old)_i, d_new_i = c1 d_old_i + c2 w_i r_i, x_i += d_new_i (+ per-block partials of rdot.x
//                  for the outer iteration's r.z). residual-only form: r_i -= (A d_old)_i and nothing else
//   k_mg_restrict: r_c = P^T (mask_f o r_f), a thread per coarse node summing 0.5 r_f over its child list in list order
//   k_mg_dense   : x_0 = Einv r_0, one wave per row (pcg_coarse.hip's k_c2_dense)
//   k_mg_prolong : e = mask_f o 0.5 (x_c[a] + x_c[b]): x_f += e, d = e (the post-smoother's first sweep then subtracts
//                  A e from the residual like any other sweep)
// Per cycle and level above 0: degree - 1 pre sweeps with the matrix, one residual pass, degree post sweeps: 2 degree
// matrix passes, each reading the matrix once and d_old, r, w, x, writing r, d_new, x.
#include <limits.h>

#include "common.hpp"

namespace fem {

constexpr int MG_BLOCK = 256;
constexpr int MG_GRID_SPMV = 2048;   // cap of the grids that write partials (the one-block scalar kernel reads them)
constexpr int MG_GRID_VEC = 1024;
constexpr int MG_MAX_LEVELS = 16;
constexpr int MG_MAX_DEGREE = 8;

struct MgState {
    double rz, pq, alpha, beta, rz_new, tol;
    int iter;        // completed iterations
    int status;      // FEM_PCG_*
    int halt;        // 1: stopped; every iteration kernel is a no-op from then on
    int stop_iter;   // reported iteration of a guard stop
    int max_iter;
    int pad_;
};

template <typename CI>
__device__ __forceinline__ int64_t mg_col(const CI* c, int64_t row) {
    return sizeof(CI) == 2 ? row + (int64_t)*c : (int64_t)*c;
}

// ---------------------------------------------------------------- first pre-smoothing sweep (x = 0 before it)
__global__ void __launch_bounds__(MG_BLOCK) k_mg_first(int64_t n, const double* __restrict__ w,
                                                       const double* __restrict__ r, double* __restrict__ d,
                                                       double* __restrict__ x, double c2,
                                                       const MgState* __restrict__ st) {
    if (st && st->halt) return;
    for (int64_t e = (int64_t)blockIdx.x * MG_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * MG_BLOCK) {
        const double dv = c2 * (w[e] * r[e]);
        d[e] = dv;
        x[e] = dv;
    }
}

// ---------------------------------------------------------------- Chebyshev sweep fused with the matrix pass
// One wave per slice, one lane per block row (pcg_coarse.hip's walk). r_in / r_out may be the same array (a row reads
// and writes its own entries only); d_old is read through the columns and is never an array this launch writes.
// Lanes of the last slice past nrows gather row 0 and store nothing.
template <int BS, typename CI, bool RESID>
__global__ void __launch_bounds__(MG_BLOCK) k_mg_cheb(int64_t nslices, int64_t nrows,
                                                      const int64_t* __restrict__ slice_ptr,
                                                      const CI* __restrict__ cols, const double* __restrict__ vals,
                                                      const double* __restrict__ w, const double* r_in, double* r_out,
                                                      const double* __restrict__ d_old, double* __restrict__ d_new,
                                                      double* __restrict__ x, double c1, double c2,
                                                      const MgState* __restrict__ st, const double* __restrict__ rdot,
                                                      double* __restrict__ part) {
    constexpr int BB = BS * BS;
    constexpr int U = BS == 1 ? 4 : 1;   // entries in flight per lane
    __shared__ double lds[4];
    if (st && st->halt) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double dot = 0.0;
    const int xcd = blockIdx.x % NXCD;
    const int64_t lb = blockIdx.x / NXCD, nlb = gridDim.x / NXCD;
    const int64_t spx = (nslices + NXCD - 1) / NXCD;
    const int64_t s_begin = (int64_t)xcd * spx;
    const int64_t s_end = s_begin + spx < nslices ? s_begin + spx : nslices;
    for (int64_t s = s_begin + lb * 4 + wave; s < s_end; s += nlb * 4) {
        const int64_t p0 = slice_ptr[s];
        const int wd = (int)((slice_ptr[s + 1] - p0) >> 6);
        const int64_t row = s * 64 + lane;
        const bool live = row < nrows;
        const CI* c = cols + p0 + lane;
        const double* v = vals + p0 * BB + lane;
        double acc[BS];
#pragma unroll
        for (int a = 0; a < BS; ++a) acc[a] = 0.0;
        for (int k0 = 0; k0 < wd; k0 += U) {
            int64_t cc[U];
            double vv[U][BB];
            double xv[U][BS];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                cc[u] = (live && k0 + u < wd) ? mg_col(c + (int64_t)64 * (k0 + u), row) : 0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double* vk = v + (int64_t)64 * BB * (k0 + u);
#pragma unroll
                for (int e = 0; e < BB; ++e) vv[u][e] = (k0 + u < wd) ? __builtin_nontemporal_load(vk + 64 * e) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < BS; ++j) xv[u][j] = d_old[cc[u] * BS + j];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k0 + u < wd) {
#pragma unroll
                    for (int a = 0; a < BS; ++a)
#pragma unroll
                        for (int j = 0; j < BS; ++j) acc[a] += vv[u][a * BS + j] * xv[u][j];
                }
        }
        if (live) {
#pragma unroll
            for (int a = 0; a < BS; ++a) {
                const int64_t i = row * BS + a;
                const double rv = r_in[i] - acc[a];
                r_out[i] = rv;
                if (!RESID) {
                    const double dv = c1 * d_old[i] + c2 * (w[i] * rv);
                    d_new[i] = dv;
                    const double xn = x[i] + dv;
                    x[i] = xn;
                    if (part) dot += rdot[i] * xn;
                }
            }
        }
    }
    if (RESID || !part) return;   // uniform over the grid
    dot = block_sum256(dot, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = dot;
}

// ---------------------------------------------------------------- restriction r_c = P^T (mask_f o r_f)
// A thread per coarse node: the child lists hold about 15 entries (the node itself twice and one mid node per edge at
// it), a wave per node would idle most lanes, and the whole pass reads one fine vector once.
template <int BS>
__global__ void __launch_bounds__(MG_BLOCK) k_mg_restrict(int64_t nc, int64_t nf, const int32_t* __restrict__ child_ptr,
                                                          const int32_t* __restrict__ child,
                                                          const double* __restrict__ wf, const double* __restrict__ rf,
                                                          double* __restrict__ rc, const MgState* __restrict__ st) {
    if (st && st->halt) return;
    for (int64_t cn = (int64_t)blockIdx.x * MG_BLOCK + threadIdx.x; cn < nc; cn += (int64_t)gridDim.x * MG_BLOCK) {
        double s[BS];
#pragma unroll
        for (int a = 0; a < BS; ++a) s[a] = 0.0;
        const int p1 = child_ptr[cn + 1];
        for (int p = child_ptr[cn]; p < p1; ++p) {
            const int64_t i = child[p];
            if (i < 0 || i >= nf) continue;
#pragma unroll
            for (int a = 0; a < BS; ++a) s[a] += wf[i * BS + a] != 0.0 ? 0.5 * rf[i * BS + a] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < BS; ++a) rc[cn * BS + a] = s[a];
    }
}

// ---------------------------------------------------------------- prolongation x_f += mask_f o P x_c (d = the same)
template <int BS>
__global__ void __launch_bounds__(MG_BLOCK) k_mg_prolong(int64_t nf, int64_t nc, const int32_t* __restrict__ parents,
                                                         const double* __restrict__ wf, const double* __restrict__ xc,
                                                         double* __restrict__ xf, double* __restrict__ d,
                                                         const MgState* __restrict__ st) {
    if (st && st->halt) return;
    for (int64_t i = (int64_t)blockIdx.x * MG_BLOCK + threadIdx.x; i < nf; i += (int64_t)gridDim.x * MG_BLOCK) {
        const int64_t a = parents[2 * i], b = parents[2 * i + 1];
        const bool ok = a >= 0 && a < nc && b >= 0 && b < nc;
#pragma unroll
        for (int e = 0; e < BS; ++e) {
            double v = 0.0;
            if (ok && wf[i * BS + e] != 0.0) v = 0.5 * (xc[a * BS + e] + xc[b * BS + e]);
            xf[i * BS + e] += v;
            if (d) d[i * BS + e] = v;
        }
    }
}

// ---------------------------------------------------------------- dense symmetric product y = Einv c (coarsest level)
__global__ void __launch_bounds__(MG_BLOCK) k_mg_dense(int m, const double* __restrict__ Einv,
                                                       const double* __restrict__ c, double* __restrict__ y,
                                                       const MgState* __restrict__ st) {
    if (st && st->halt) return;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;   // whole waves leave: no shuffle is split
    const double* e = Einv + (int64_t)row * m;
    double s = 0.0;
    for (int j = lane; j < m; j += 64) s += e[j] * c[j];
    s = wave_sum(s);
    if (lane == 0) y[row] = s;
}

// ---------------------------------------------------------------- the outer iteration's vector kernels
__global__ void __launch_bounds__(MG_BLOCK) k_mg_init(int64_t n, const double* __restrict__ b,
                                                      const double* __restrict__ q, double* __restrict__ r) {
    for (int64_t e = (int64_t)blockIdx.x * MG_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * MG_BLOCK)
        r[e] = b[e] - q[e];
}

__global__ void __launch_bounds__(MG_BLOCK) k_mg_update(int64_t n, double* __restrict__ x, const double* __restrict__ p,
                                                        double* __restrict__ r, const double* __restrict__ q,
                                                        const MgState* __restrict__ st) {
    if (st->halt) return;
    const double al = st->alpha;
    for (int64_t e = (int64_t)blockIdx.x * MG_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * MG_BLOCK) {
        x[e] += al * p[e];
        r[e] = r[e] - al * q[e];
    }
}

__global__ void __launch_bounds__(MG_BLOCK) k_mg_pupdate(int64_t n, double* __restrict__ p, const double* __restrict__ z,
                                                         const MgState* __restrict__ st, int first) {
    if (st->halt) return;
    const double be = st->beta;
    for (int64_t e = (int64_t)blockIdx.x * MG_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * MG_BLOCK)
        p[e] = first ? z[e] : z[e] + be * p[e];
}

// q = A p with per-block partials of p.q (pcg_coarse.hip's k_c2_spmv for both block sizes)
template <int BS, typename CI>
__global__ void __launch_bounds__(MG_BLOCK) k_mg_spmv(int64_t nslices, int64_t nrows,
                                                      const int64_t* __restrict__ slice_ptr,
                                                      const CI* __restrict__ cols, const double* __restrict__ vals,
                                                      const double* __restrict__ x, double* __restrict__ y,
                                                      const MgState* __restrict__ st, double* __restrict__ part) {
    constexpr int BB = BS * BS;
    __shared__ double lds[4];
    if (st && st->halt) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double dot = 0.0;
    const int xcd = blockIdx.x % NXCD;
    const int64_t lb = blockIdx.x / NXCD, nlb = gridDim.x / NXCD;
    const int64_t spx = (nslices + NXCD - 1) / NXCD;
    const int64_t s_begin = (int64_t)xcd * spx;
    const int64_t s_end = s_begin + spx < nslices ? s_begin + spx : nslices;
    for (int64_t s = s_begin + lb * 4 + wave; s < s_end; s += nlb * 4) {
        const int64_t p0 = slice_ptr[s];
        const int wd = (int)((slice_ptr[s + 1] - p0) >> 6);
        const int64_t row = s * 64 + lane;
        const bool live = row < nrows;
        const CI* c = cols + p0 + lane;
        const double* v = vals + p0 * BB + lane;
        double acc[BS];
#pragma unroll
        for (int a = 0; a < BS; ++a) acc[a] = 0.0;
        for (int k = 0; k < wd; ++k) {
            const int64_t col = live ? mg_col(c + (int64_t)64 * k, row) : 0;
            const double* vk = v + (int64_t)64 * BB * k;
            double vv[BB];
#pragma unroll
            for (int e = 0; e < BB; ++e) vv[e] = __builtin_nontemporal_load(vk + 64 * e);
            double xv[BS];
#pragma unroll
            for (int j = 0; j < BS; ++j) xv[j] = x[col * BS + j];
#pragma unroll
            for (int a = 0; a < BS; ++a)
#pragma unroll
                for (int j = 0; j < BS; ++j) acc[a] += vv[a * BS + j] * xv[j];
        }
        if (live) {
#pragma unroll
            for (int a = 0; a < BS; ++a) {
                y[row * BS + a] = acc[a];
                if (part) dot += x[row * BS + a] * acc[a];
            }
        }
    }
    if (!part) return;
    dot = block_sum256(dot, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = dot;
}

// One block: the partials summed in a fixed order and the state stepped. phase 0: r0.z0; 1: p.q -> alpha and the
// guard; 2: r.z -> stop test, the guard on r.z (an underestimated lmax can make the cycle indefinite), beta, count,
// history.
__global__ void __launch_bounds__(MG_BLOCK) k_mg_scalars(MgState* __restrict__ st, const double* __restrict__ part,
                                                         int nblocks, int phase, double* __restrict__ hist,
                                                         int64_t hist_len) {
    __shared__ double lds[4];
    if (st->halt) return;   // uniform: written by thread 0 only after the sum below
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += MG_BLOCK) s += part[i];
    s = block_sum256(s, lds);
    if (threadIdx.x != 0) return;
    if (phase == 0) {
        st->rz = s;
        if (!(s >= 0.0) || isinf(s)) {
            st->status = FEM_PCG_BREAKDOWN;   // r0.z0 < 0 or non-finite: the first iteration cannot start
            st->stop_iter = 1;
            st->halt = 1;
        } else if (s == 0.0) {   // the start vector already solves the free rows (b = 0, x = 0): nothing to iterate on,
            st->status = FEM_PCG_CONVERGED;   // and p = z = 0 would only make p.Ap = 0 look like a breakdown
            st->stop_iter = 0;
            st->halt = 1;
        } else if (st->max_iter <= 0) {
            st->status = FEM_PCG_MAXITER;
            st->halt = 1;
        }
    } else if (phase == 1) {
        st->pq = s;
        if (!(s > 0.0) || isinf(s)) {
            st->status = FEM_PCG_BREAKDOWN;
            st->stop_iter = st->iter + 1;
            st->halt = 1;
        } else {
            st->alpha = st->rz / s;
        }
    } else {
        const int it = st->iter;
        st->rz_new = s;
        st->iter = it + 1;
        const double nrm = sqrt(s);
        if (hist && it < hist_len) hist[it] = nrm;
        if (nrm < st->tol) {
            st->status = FEM_PCG_CONVERGED;
            st->stop_iter = it + 1;
            st->halt = 1;
        } else if (!(s > 0.0) || isinf(s)) {
            st->status = FEM_PCG_BREAKDOWN;
            st->stop_iter = it + 1;
            st->halt = 1;
        } else {
            st->beta = s / st->rz;
            st->rz = s;
            if (it + 1 >= st->max_iter) {
                st->status = FEM_PCG_MAXITER;
                st->halt = 1;
            }
        }
    }
}

}  // namespace fem

using namespace fem;

// ---------------------------------------------------------------- host side
struct MgLevel {
    int64_t nrows, n;
    const int64_t* slice_ptr;
    const int32_t* cols;
    const int16_t* dcols;
    const double* vals;
    const double* w;
    const int32_t *parents, *child_ptr, *child;
    double *x, *d0, *d1, *r;   // d0 / d1 / r unused on level 0
    int grid_spmv, grid_vec;
};

struct fem_mg {
    int nlev, bs, degree, m0;
    MgLevel lev[MG_MAX_LEVELS];
    double c1[MG_MAX_LEVELS][MG_MAX_DEGREE], c2[MG_MAX_LEVELS][MG_MAX_DEGREE];
    const double* Einv;
    hipStream_t stream;
    void* block;
    double *r, *p, *q, *part_pq, *part_rz;
    MgState* st;
    MgState host;
    double* hist;
    int64_t hist_len;
};

static int mg_grid_spmv(int64_t nslices) { return grid_multiple_of_xcd(cdiv(nslices, 4), MG_GRID_SPMV); }
static int mg_grid_vec(int64_t n) {
    const int64_t g = cdiv(n, MG_BLOCK);
    return (int)(g > MG_GRID_VEC ? MG_GRID_VEC : (g < 1 ? 1 : g));
}

template <bool RESID>
static void mg_cheb(const fem_mg* s, const MgLevel& L, const double* r_in, const double* d_old, double* d_new, double c1,
                    double c2, const MgState* st, const double* rdot, double* part) {
    const int64_t nslices = cdiv(L.nrows, 64);
    const dim3 grid(L.grid_spmv), block(MG_BLOCK);
#define MG_LAUNCH(BS, CI, COLS)                                                                                      \
    hipLaunchKernelGGL((k_mg_cheb<BS, CI, RESID>), grid, block, 0, s->stream, nslices, L.nrows, L.slice_ptr, COLS,   \
                       L.vals, L.w, r_in, L.r, d_old, d_new, L.x, c1, c2, st, rdot, part)
    if (s->bs == 1) {
        if (L.dcols)
            MG_LAUNCH(1, int16_t, L.dcols);
        else
            MG_LAUNCH(1, int32_t, L.cols);
    } else {
        if (L.dcols)
            MG_LAUNCH(3, int16_t, L.dcols);
        else
            MG_LAUNCH(3, int32_t, L.cols);
    }
#undef MG_LAUNCH
}

static void mg_spmv(const fem_mg* s, const MgLevel& L, const double* x, double* y, const MgState* st, double* part) {
    const int64_t nslices = cdiv(L.nrows, 64);
    const dim3 grid(L.grid_spmv), block(MG_BLOCK);
#define MG_LAUNCH(BS, CI, COLS)                                                                                     \
    hipLaunchKernelGGL((k_mg_spmv<BS, CI>), grid, block, 0, s->stream, nslices, L.nrows, L.slice_ptr, COLS, L.vals, \
                       x, y, st, part)
    if (s->bs == 1) {
        if (L.dcols)
            MG_LAUNCH(1, int16_t, L.dcols);
        else
            MG_LAUNCH(1, int32_t, L.cols);
    } else {
        if (L.dcols)
            MG_LAUNCH(3, int16_t, L.dcols);
        else
            MG_LAUNCH(3, int32_t, L.cols);
    }
#undef MG_LAUNCH
}

static void mg_restrict(const fem_mg* s, int l, const MgState* st) {   // level l -> l - 1
    const MgLevel &F = s->lev[l], &Cc = s->lev[l - 1];
    const dim3 grid(mg_grid_vec(Cc.nrows)), block(MG_BLOCK);
    if (s->bs == 1)
        hipLaunchKernelGGL(k_mg_restrict<1>, grid, block, 0, s->stream, Cc.nrows, F.nrows, F.child_ptr, F.child, F.w,
                           (const double*)F.r, Cc.r, st);
    else
        hipLaunchKernelGGL(k_mg_restrict<3>, grid, block, 0, s->stream, Cc.nrows, F.nrows, F.child_ptr, F.child, F.w,
                           (const double*)F.r, Cc.r, st);
}

static void mg_prolong(const fem_mg* s, int l, double* d, const MgState* st) {   // level l - 1 -> l
    const MgLevel &F = s->lev[l], &Cc = s->lev[l - 1];
    const dim3 grid(mg_grid_vec(F.nrows)), block(MG_BLOCK);
    if (s->bs == 1)
        hipLaunchKernelGGL(k_mg_prolong<1>, grid, block, 0, s->stream, F.nrows, Cc.nrows, F.parents, F.w,
                           (const double*)Cc.x, F.x, d, st);
    else
        hipLaunchKernelGGL(k_mg_prolong<3>, grid, block, 0, s->stream, F.nrows, Cc.nrows, F.parents, F.w,
                           (const double*)Cc.x, F.x, d, st);
}

// z = cycle(rfine), left in lev[nlev - 1].x; rfine is not written. rdot / part: partials of rdot.z from the last sweep.
static void mg_cycle(const fem_mg* s, const double* rfine, const MgState* st, const double* rdot, double* part) {
    const int top = s->nlev - 1, deg = s->degree;
    for (int l = top; l >= 1; --l) {
        const MgLevel& L = s->lev[l];
        const double* rin = l == top ? rfine : L.r;
        hipLaunchKernelGGL(k_mg_first, dim3(L.grid_vec), dim3(MG_BLOCK), 0, s->stream, L.n, L.w, rin, L.d0, L.x,
                           s->c2[l][0], st);
        double *cur = L.d0, *nxt = L.d1;
        for (int k = 1; k < deg; ++k) {
            mg_cheb<false>(s, L, rin, cur, nxt, s->c1[l][k], s->c2[l][k], st, nullptr, nullptr);
            rin = L.r;
            double* t = cur;
            cur = nxt;
            nxt = t;
        }
        mg_cheb<true>(s, L, rin, cur, nullptr, 0.0, 0.0, st, nullptr, nullptr);
        mg_restrict(s, l, st);
    }
    const MgLevel& L0 = s->lev[0];
    hipLaunchKernelGGL(k_mg_dense, dim3((unsigned)cdiv(s->m0, 4)), dim3(MG_BLOCK), 0, s->stream, s->m0, s->Einv,
                       (const double*)L0.r, L0.x, st);
    for (int l = 1; l <= top; ++l) {
        const MgLevel& L = s->lev[l];
        double *cur = L.d0, *nxt = L.d1;
        mg_prolong(s, l, cur, st);
        for (int k = 0; k < deg; ++k) {
            const bool last = l == top && k == deg - 1;
            mg_cheb<false>(s, L, L.r, cur, nxt, s->c1[l][k], s->c2[l][k], st, last ? rdot : nullptr,
                           last ? part : nullptr);
            double* t = cur;
            cur = nxt;
            nxt = t;
        }
    }
}

static void mg_scalars(fem_mg* s, const double* part, int nblocks, int phase) {
    hipLaunchKernelGGL(k_mg_scalars, dim3(1), dim3(MG_BLOCK), 0, s->stream, s->st, part, nblocks, phase, s->hist,
                       s->hist_len);
}

static int mg_poll(fem_mg* s) {
    FEM_HIP(hipMemcpyAsync(&s->host, s->st, sizeof(MgState), hipMemcpyDeviceToHost, s->stream));
    FEM_HIP(hipStreamSynchronize(s->stream));
    return FEM_OK;
}

extern "C" {

int fem_mg_restrict(int64_t nc, int64_t nf, int bs, const int32_t* child_ptr, const int32_t* child, const double* wf,
                    const double* rf, double* rc, fem_stream_t stream) {
    if ((bs != 1 && bs != 3) || nc <= 0 || nf <= 0 || !child_ptr || !child || !wf || !rf || !rc) {
        set_error("fem_mg_restrict: bs 1 or 3, rows and every array are needed (bs %d, %lld coarse, %lld fine nodes)",
                  bs, (long long)nc, (long long)nf);
        return FEM_EARG;
    }
    const dim3 grid(mg_grid_vec(nc)), block(MG_BLOCK);
    if (bs == 1)
        hipLaunchKernelGGL(k_mg_restrict<1>, grid, block, 0, S(stream), nc, nf, child_ptr, child, wf, rf, rc,
                           (const MgState*)nullptr);
    else
        hipLaunchKernelGGL(k_mg_restrict<3>, grid, block, 0, S(stream), nc, nf, child_ptr, child, wf, rf, rc,
                           (const MgState*)nullptr);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_mg_prolong(int64_t nf, int64_t nc, int bs, const int32_t* parents, const double* wf, const double* xc,
                   double* xf, fem_stream_t stream) {
    if ((bs != 1 && bs != 3) || nc <= 0 || nf <= 0 || !parents || !wf || !xc || !xf) {
        set_error("fem_mg_prolong: bs 1 or 3, rows and every array are needed (bs %d, %lld coarse, %lld fine nodes)",
                  bs, (long long)nc, (long long)nf);
        return FEM_EARG;
    }
    const dim3 grid(mg_grid_vec(nf)), block(MG_BLOCK);
    if (bs == 1)
        hipLaunchKernelGGL(k_mg_prolong<1>, grid, block, 0, S(stream), nf, nc, parents, wf, xc, xf, (double*)nullptr,
                           (const MgState*)nullptr);
    else
        hipLaunchKernelGGL(k_mg_prolong<3>, grid, block, 0, S(stream), nf, nc, parents, wf, xc, xf, (double*)nullptr,
                           (const MgState*)nullptr);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_mg_create(int nlev, int bs, const int64_t* nrows, const void* const* slice_ptr, const void* const* cols,
                  const void* const* dcols, const void* const* vals, const void* const* w, const void* const* parents,
                  const void* const* child_ptr, const void* const* child, int degree, const double* c1,
                  const double* c2, int64_t m0, const double* Einv, fem_stream_t stream, fem_mg** out) {
    if (bs != 1 && bs != 3) {
        set_error("fem_mg_create: block size %d unsupported (1 or 3)", bs);
        return FEM_EARG;
    }
    if (nlev < 2 || nlev > MG_MAX_LEVELS || degree < 1 || degree > MG_MAX_DEGREE) {
        set_error("fem_mg_create: 2 to %d levels and degree 1 to %d, got %d levels, degree %d", MG_MAX_LEVELS,
                  MG_MAX_DEGREE, nlev, degree);
        return FEM_EARG;
    }
    if (!nrows || !slice_ptr || !cols || !dcols || !vals || !w || !parents || !child_ptr || !child || !c1 || !c2 ||
        !Einv || !out) {
        set_error("fem_mg_create: null argument");
        return FEM_EARG;
    }
    if (m0 != nrows[0] * bs || m0 > INT_MAX) {
        set_error("fem_mg_create: the coarse inverse must be [%lld, %lld], got m = %lld", (long long)(nrows[0] * bs),
                  (long long)(nrows[0] * bs), (long long)m0);
        return FEM_EARG;
    }
    for (int l = 0; l < nlev; ++l) {
        const bool mat = l > 0;
        if (nrows[l] <= 0 || nrows[l] * bs > (int64_t)INT_MAX || !w[l] ||
            (mat && (!slice_ptr[l] || (!cols[l] && !dcols[l]) || !vals[l] || !parents[l] || !child_ptr[l] || !child[l]))) {
            set_error("fem_mg_create: level %d needs rows, w and (above level 0) a matrix, parents and the child lists",
                      l);
            return FEM_EARG;
        }
    }
    fem_mg* s = new fem_mg();
    s->nlev = nlev;
    s->bs = bs;
    s->degree = degree;
    s->m0 = (int)m0;
    s->Einv = Einv;
    s->stream = S(stream);
    s->hist = nullptr;
    s->hist_len = 0;
    size_t total = 0;
    for (int l = 0; l < nlev; ++l) {
        MgLevel& L = s->lev[l];
        L.nrows = nrows[l];
        L.n = nrows[l] * bs;
        L.slice_ptr = (const int64_t*)slice_ptr[l];
        L.cols = (const int32_t*)cols[l];
        L.dcols = (const int16_t*)dcols[l];
        L.vals = (const double*)vals[l];
        L.w = (const double*)w[l];
        L.parents = (const int32_t*)parents[l];
        L.child_ptr = (const int32_t*)child_ptr[l];
        L.child = (const int32_t*)child[l];
        L.grid_spmv = mg_grid_spmv(cdiv(L.nrows, 64));
        L.grid_vec = mg_grid_vec(L.n);
        total += (size_t)L.n * (l == 0 ? 2 : 4);
        for (int k = 0; k < degree; ++k) {
            s->c1[l][k] = c1[l * degree + k];
            s->c2[l][k] = c2[l * degree + k];
        }
    }
    const MgLevel& T = s->lev[nlev - 1];
    total += 3 * (size_t)T.n + 2 * (size_t)T.grid_spmv;
    s->block = nullptr;
    const hipError_t e = hipMalloc(&s->block, sizeof(double) * total + sizeof(MgState));
    if (e != hipSuccess) {
        set_error("fem_mg_create: allocation failed: %s", hipGetErrorString(e));
        delete s;
        return FEM_EHIP;
    }
    double* p = (double*)s->block;
    for (int l = 0; l < nlev; ++l) {
        MgLevel& L = s->lev[l];
        L.x = p;
        p += L.n;
        L.r = p;
        p += L.n;
        L.d0 = L.d1 = nullptr;
        if (l > 0) {
            L.d0 = p;
            p += L.n;
            L.d1 = p;
            p += L.n;
        }
    }
    s->r = p;
    p += T.n;
    s->p = p;
    p += T.n;
    s->q = p;
    p += T.n;
    s->part_pq = p;
    p += T.grid_spmv;
    s->part_rz = p;
    p += T.grid_spmv;
    s->st = (MgState*)p;
    *out = s;
    return FEM_OK;
}

/* z = one V-cycle on r (both [n] of the finest level); r is not written */
int fem_mg_apply(fem_mg* s, const double* r, double* z) {
    if (!s || !r || !z) {
        set_error("fem_mg_apply: null argument");
        return FEM_EARG;
    }
    const MgLevel& T = s->lev[s->nlev - 1];
    mg_cycle(s, r, nullptr, nullptr, nullptr);
    FEM_LAUNCHED();
    FEM_HIP(hipMemcpyAsync(z, T.x, sizeof(double) * (size_t)T.n, hipMemcpyDeviceToDevice, s->stream));
    return FEM_OK;
}

/* one fused sweep on the work vectors of `level` (>= 1), for timing: what they hold afterwards is meaningless, and every
 * cycle writes them before it reads them */
int fem_mg_sweep(fem_mg* s, int level) {
    if (!s || level < 1 || level >= s->nlev) {
        set_error("fem_mg_sweep: level 1 to %d", s ? s->nlev - 1 : 0);
        return FEM_EARG;
    }
    const MgLevel& L = s->lev[level];
    mg_cheb<false>(s, L, L.r, L.d0, L.d1, s->c1[level][s->degree - 1], s->c2[level][s->degree - 1], nullptr, nullptr,
                   nullptr);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_mg_solve(fem_mg* s, const double* b, double* x, double tol, int max_iter, int chunk, double* hist,
                 int64_t hist_len, int* iters, int* status, double* rz) {
    if (!s || !b || !x) {
        set_error("fem_mg_solve: null argument");
        return FEM_EARG;
    }
    const MgLevel& T = s->lev[s->nlev - 1];
    s->hist = hist;
    s->hist_len = hist ? hist_len : 0;
    MgState h{};
    h.tol = tol;
    h.max_iter = max_iter;
    s->host = h;
    FEM_HIP(hipMemcpyAsync(s->st, &s->host, sizeof(MgState), hipMemcpyHostToDevice, s->stream));
    mg_spmv(s, T, x, s->q, nullptr, nullptr);
    hipLaunchKernelGGL(k_mg_init, dim3(T.grid_vec), dim3(MG_BLOCK), 0, s->stream, T.n, b, (const double*)s->q, s->r);
    mg_cycle(s, s->r, s->st, s->r, s->part_rz);
    mg_scalars(s, s->part_rz, T.grid_spmv, 0);
    hipLaunchKernelGGL(k_mg_pupdate, dim3(T.grid_vec), dim3(MG_BLOCK), 0, s->stream, T.n, s->p, (const double*)T.x,
                       (const MgState*)s->st, 1);
    FEM_LAUNCHED();
    if (chunk <= 0) chunk = 8;
    int done = 0, rc;
    while (done < max_iter) {
        const int k = chunk < max_iter - done ? chunk : max_iter - done;
        for (int i = 0; i < k; ++i) {
            mg_spmv(s, T, s->p, s->q, s->st, s->part_pq);
            mg_scalars(s, s->part_pq, T.grid_spmv, 1);
            hipLaunchKernelGGL(k_mg_update, dim3(T.grid_vec), dim3(MG_BLOCK), 0, s->stream, T.n, x,
                               (const double*)s->p, s->r, (const double*)s->q, (const MgState*)s->st);
            mg_cycle(s, s->r, s->st, s->r, s->part_rz);
            mg_scalars(s, s->part_rz, T.grid_spmv, 2);
            hipLaunchKernelGGL(k_mg_pupdate, dim3(T.grid_vec), dim3(MG_BLOCK), 0, s->stream, T.n, s->p,
                               (const double*)T.x, (const MgState*)s->st, 0);
            FEM_LAUNCHED();
        }
        done += k;
        if ((rc = mg_poll(s))) return rc;
        if (s->host.halt) break;
    }
    if ((rc = mg_poll(s))) return rc;
    const MgState& c = s->host;
    if (iters) *iters = c.status == FEM_PCG_BREAKDOWN ? c.stop_iter : c.iter;
    if (status) *status = c.status;
    if (rz) *rz = c.iter > 0 ? c.rz_new : c.rz;
    return FEM_OK;
}

int fem_mg_scalars(fem_mg* s, double* out6) {
    if (!s || !out6) {
        set_error("fem_mg_scalars: null argument");
        return FEM_EARG;
    }
    const int rc = mg_poll(s);
    if (rc) return rc;
    const MgState& c = s->host;
    out6[0] = c.rz;
    out6[1] = c.pq;
    out6[2] = c.alpha;
    out6[3] = c.beta;
    out6[4] = c.rz_new;
    out6[5] = (double)c.iter;
    return FEM_OK;
}

void fem_mg_destroy(fem_mg* s) {
    if (!s) return;
    (void)hipStreamSynchronize(s->stream);
    if (s->block) (void)hipFree(s->block);
    delete s;
}

}  // extern "C"
