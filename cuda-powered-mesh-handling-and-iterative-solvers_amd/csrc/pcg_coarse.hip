// Two-level PCG: the Jacobi preconditioner plus an additive rigid-body coarse correction,
//   M^-1 = diag(w) + Z (Z^T A Z)^-1 Z^T,
// on bs = 3 matrices with three translational dofs per node. Z is never stored: the row block of node i is
//   R_i = [I_3 | -[rel_i]x]   (u = t + theta x rel_i),   rel_i = (x_i - c_a) / rho_a,   a = agg[i],
// with the rows of the fixed dofs (w == 0) zero. agg [nrows] int32 holds -1 for a node in no aggregate; agg_ptr [k+1]
// / agg_nodes list every aggregate's nodes (ascending). The matrix is the plain SELL-64 layout of include/fem355.h
// with int32 `cols` or 16-bit `dcols`, as for pcg_multi.hip.
//
// Rules of the file (those of modal.hip / transient.hip / pcg_multi.hip): plain launches on the caller's stream, no
// workgroup waits on another, no floating-point atomics, every reduction finished in a fixed order that depends on
// the problem sizes only (bit-identical run to run), rows >= nrows never read or stored, matrix values read with
// nontemporal loads.
//
// Per iteration of the lock-step context (fem_pcg2_*):
//   k_c2_spmv      : q = A p, per-block partials of p.q
//   k_c2_scalars(1): partials summed by ONE block -> alpha; p.q <= 0 or non-finite -> FEM_PCG_BREAKDOWN
//   k_c2_update    : x += alpha p, r -= alpha q
//   k_c2_restrict  : c = Z^T r, one workgroup per aggregate (list order per thread, block_sum256 tree)
//   k_c2_dense     : y = Einv c, one wave per row (lane l adds columns l, l + 64, ... in order, wave_sum)
//   k_c2_prolong   : z = w o r + Z y, per-block partials of r.z
//   k_c2_scalars(2): -> stop test on sqrt(r.z), beta, iteration count, history
//   k_c2_pupdate   : p = z + beta p
#include <limits.h>

#include "common.hpp"

namespace fem {

constexpr int C2_BLOCK = 256;
constexpr int C2_GRID_SPMV = 2048;   // cap of the grids that write partials (the one-block scalar kernel reads them)
constexpr int C2_GRID_VEC = 1024;

struct C2State {
    double rz, pq, alpha, beta, rz_new, tol;
    int iter;        // completed iterations
    int status;      // FEM_PCG_*
    int halt;        // 1: stopped; every iteration kernel is a no-op from then on
    int stop_iter;   // reported iteration of a guard stop
    int max_iter;
    int pad_;
};

template <typename CI>
__device__ __forceinline__ int64_t c2_col(const CI* c, int64_t row) {
    return sizeof(CI) == 2 ? row + (int64_t)*c : (int64_t)*c;
}

// ---------------------------------------------------------------- restriction c = Z^T r
// Workgroup a walks agg_nodes[agg_ptr[a] .. agg_ptr[a + 1]): thread t takes positions t, t + 256, ... in list order.
__global__ void __launch_bounds__(C2_BLOCK) k_c2_restrict(const int32_t* __restrict__ agg_ptr,
                                                          const int32_t* __restrict__ agg_nodes,
                                                          const double* __restrict__ rel, const double* __restrict__ w,
                                                          const double* __restrict__ r, double* __restrict__ c,
                                                          const C2State* __restrict__ st) {
    __shared__ double lds[4];
    if (st && st->halt) return;
    const int a = blockIdx.x;
    const int p0 = agg_ptr[a], p1 = agg_ptr[a + 1];
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int p = p0 + (int)threadIdx.x; p < p1; p += C2_BLOCK) {
        const int64_t i = agg_nodes[p];
        const double r0 = w[3 * i] != 0.0 ? r[3 * i] : 0.0;
        const double r1 = w[3 * i + 1] != 0.0 ? r[3 * i + 1] : 0.0;
        const double r2 = w[3 * i + 2] != 0.0 ? r[3 * i + 2] : 0.0;
        const double x = rel[3 * i], y = rel[3 * i + 1], z = rel[3 * i + 2];
        s[0] += r0;
        s[1] += r1;
        s[2] += r2;
        s[3] += y * r2 - z * r1;   // rel x r
        s[4] += z * r0 - x * r2;
        s[5] += x * r1 - y * r0;
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        const double t = block_sum256(s[e], lds);
        if (threadIdx.x == 0) c[6 * (int64_t)a + e] = t;
    }
}

// ---------------------------------------------------------------- dense symmetric product y = Einv c
__global__ void __launch_bounds__(C2_BLOCK) k_c2_dense(int m, const double* __restrict__ Einv,
                                                       const double* __restrict__ c, double* __restrict__ y,
                                                       const C2State* __restrict__ st) {
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

// ---------------------------------------------------------------- prolongation z = w o r + Z y (+ r.z partials)
__global__ void __launch_bounds__(C2_BLOCK) k_c2_prolong(int64_t nrows, const int32_t* __restrict__ agg,
                                                         const double* __restrict__ rel, const double* __restrict__ w,
                                                         const double* __restrict__ y, const double* __restrict__ r,
                                                         double* __restrict__ z, const C2State* __restrict__ st,
                                                         double* __restrict__ part) {
    __shared__ double lds[4];
    if (st && st->halt) return;
    double dot = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * C2_BLOCK + threadIdx.x; i < nrows; i += (int64_t)gridDim.x * C2_BLOCK) {
        const int a = agg[i];
        double u[3] = {0.0, 0.0, 0.0};
        if (a >= 0) {
            const double* ya = y + 6 * (int64_t)a;
            const double rx = rel[3 * i], ry = rel[3 * i + 1], rz = rel[3 * i + 2];
            const double t3 = ya[3], t4 = ya[4], t5 = ya[5];
            u[0] = ya[0] + (t4 * rz - t5 * ry);   // t + theta x rel
            u[1] = ya[1] + (t5 * rx - t3 * rz);
            u[2] = ya[2] + (t3 * ry - t4 * rx);
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const double wv = w[3 * i + e], rv = r[3 * i + e];
            const double zv = wv * rv + (wv != 0.0 ? u[e] : 0.0);
            z[3 * i + e] = zv;
            dot += rv * zv;
        }
    }
    if (!part) return;   // uniform over the grid
    dot = block_sum256(dot, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = dot;
}

// ---------------------------------------------------------------- Galerkin product E = Z^T A Z
// A lane per block row. Count pass: the number of distinct aggregates among the row's neighbours. Emit pass: the row
// walks its entries once per distinct neighbour aggregate b in ascending id, summing S = sum_{j in b} A_ij R_j
// (18 accumulators) in entry order, and stores the record (key = a k + b, R_i^T S) at its offset from the scanned
// counts. Padding entries name the row itself (or the last row) with zero values: they add no aggregate that the
// diagonal entry has not, and no value.
template <typename CI>
__global__ void __launch_bounds__(C2_BLOCK) k_c2_gal_count(int64_t nslices, int64_t nrows,
                                                           const int64_t* __restrict__ slice_ptr,
                                                           const CI* __restrict__ cols, const int32_t* __restrict__ agg,
                                                           int64_t* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= nslices) return;
    const int64_t row = s * 64 + lane;
    if (row >= nrows) return;   // no shuffles below
    int64_t n = 0;
    if (agg[row] >= 0) {
        const int64_t p0 = slice_ptr[s];
        const int wd = (int)((slice_ptr[s + 1] - p0) >> 6);
        const CI* c = cols + p0 + lane;
        int cur = -1;
        for (;;) {
            int nxt = INT_MAX;
            for (int k = 0; k < wd; ++k) {
                const int g = agg[c2_col(c + (int64_t)64 * k, row)];
                if (g > cur && g < nxt) nxt = g;
            }
            if (nxt == INT_MAX) break;
            ++n;
            cur = nxt;
        }
    }
    count[row] = n;
}

template <typename CI>
__global__ void __launch_bounds__(C2_BLOCK) k_c2_gal_emit(int64_t nslices, int64_t nrows, int kagg,
                                                          const int64_t* __restrict__ slice_ptr,
                                                          const CI* __restrict__ cols, const double* __restrict__ vals,
                                                          const int32_t* __restrict__ agg, const double* __restrict__ rel,
                                                          const double* __restrict__ w, const int64_t* __restrict__ offset,
                                                          int64_t* __restrict__ keys, double* __restrict__ rec) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= nslices) return;
    const int64_t row = s * 64 + lane;
    if (row >= nrows) return;
    const int a = agg[row];
    if (a < 0) return;
    const int64_t p0 = slice_ptr[s];
    const int wd = (int)((slice_ptr[s + 1] - p0) >> 6);
    const CI* c = cols + p0 + lane;
    const double* v = vals + p0 * 9 + lane;
    const double ix = rel[3 * row], iy = rel[3 * row + 1], iz = rel[3 * row + 2];
    const double mi0 = w[3 * row] != 0.0 ? 1.0 : 0.0, mi1 = w[3 * row + 1] != 0.0 ? 1.0 : 0.0,
                 mi2 = w[3 * row + 2] != 0.0 ? 1.0 : 0.0;
    int64_t o = offset[row];
    int nxt = INT_MAX;
    for (int k = 0; k < wd; ++k) {
        const int g = agg[c2_col(c + (int64_t)64 * k, row)];
        if (g >= 0 && g < nxt) nxt = g;
    }
    while (nxt != INT_MAX) {
        double S[3][6];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int q = 0; q < 6; ++q) S[r][q] = 0.0;
        int nn = INT_MAX;
        for (int k = 0; k < wd; ++k) {
            const int64_t col = c2_col(c + (int64_t)64 * k, row);
            const int g = agg[col];
            if (g == nxt) {
                const double* vk = v + (int64_t)64 * 9 * k;
                const double jx = rel[3 * col], jy = rel[3 * col + 1], jz = rel[3 * col + 2];
                const double m0 = w[3 * col] != 0.0 ? 1.0 : 0.0, m1 = w[3 * col + 1] != 0.0 ? 1.0 : 0.0,
                             m2 = w[3 * col + 2] != 0.0 ? 1.0 : 0.0;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double a0 = __builtin_nontemporal_load(vk + 64 * (3 * r)) * m0;
                    const double a1 = __builtin_nontemporal_load(vk + 64 * (3 * r + 1)) * m1;
                    const double a2 = __builtin_nontemporal_load(vk + 64 * (3 * r + 2)) * m2;
                    S[r][0] += a0;
                    S[r][1] += a1;
                    S[r][2] += a2;
                    // rotation columns of R_j: rows of -[rel]x are (0, z, -y), (-z, 0, x), (y, -x, 0)
                    S[r][3] += a2 * jy - a1 * jz;
                    S[r][4] += a0 * jz - a2 * jx;
                    S[r][5] += a1 * jx - a0 * jy;
                }
            } else if (g > nxt && g < nn) {
                nn = g;
            }
        }
        keys[o] = (int64_t)a * kagg + nxt;
        double* out = rec + o * 36;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double s0 = mi0 * S[0][q], s1 = mi1 * S[1][q], s2 = mi2 * S[2][q];
            out[q] = s0;
            out[6 + q] = s1;
            out[12 + q] = s2;
            out[18 + q] = iy * s2 - iz * s1;   // rel_i x S[:, q]
            out[24 + q] = iz * s0 - ix * s2;
            out[30 + q] = ix * s1 - iy * s0;
        }
        ++o;
        nxt = nn;
    }
}

// one wave per key: lane e < 36 adds entry e of the key's records in sorted (record) order
__global__ void __launch_bounds__(C2_BLOCK) k_c2_gal_sum(int64_t nkeys, int kagg, const int64_t* __restrict__ ukeys,
                                                         const int64_t* __restrict__ key_ptr,
                                                         const int64_t* __restrict__ order,
                                                         const double* __restrict__ rec, double* __restrict__ E) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= nkeys || lane >= 36) return;
    double s = 0.0;
    for (int64_t p = key_ptr[u]; p < key_ptr[u + 1]; ++p) s += rec[order[p] * 36 + lane];
    const int64_t key = ukeys[u];
    const int64_t a = key / kagg, b = key % kagg;
    const int64_t m = 6 * (int64_t)kagg;
    E[(6 * a + lane / 6) * m + 6 * b + lane % 6] = s;
}

// ---------------------------------------------------------------- the iteration's matrix pass and vector kernels
// q = A p with per-block partials of p.q: one wave per slice, one lane per block row (pcg_multi.hip's walk at one
// column). Lanes of the last slice past nrows gather row 0 and store nothing.
template <typename CI>
__global__ void __launch_bounds__(C2_BLOCK) k_c2_spmv(int64_t nslices, int64_t nrows,
                                                      const int64_t* __restrict__ slice_ptr,
                                                      const CI* __restrict__ cols, const double* __restrict__ vals,
                                                      const double* __restrict__ x, double* __restrict__ y,
                                                      const C2State* __restrict__ st, double* __restrict__ part) {
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
        const double* v = vals + p0 * 9 + lane;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int k = 0; k < wd; ++k) {
            const int64_t col = live ? c2_col(c + (int64_t)64 * k, row) : 0;
            const double* vk = v + (int64_t)64 * 9 * k;
            double vv[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) vv[e] = __builtin_nontemporal_load(vk + 64 * e);
            const double x0 = x[3 * col], x1 = x[3 * col + 1], x2 = x[3 * col + 2];
            a0 += vv[0] * x0;
            a0 += vv[1] * x1;
            a0 += vv[2] * x2;
            a1 += vv[3] * x0;
            a1 += vv[4] * x1;
            a1 += vv[5] * x2;
            a2 += vv[6] * x0;
            a2 += vv[7] * x1;
            a2 += vv[8] * x2;
        }
        if (live) {
            y[3 * row] = a0;
            y[3 * row + 1] = a1;
            y[3 * row + 2] = a2;
            if (part) dot += x[3 * row] * a0 + x[3 * row + 1] * a1 + x[3 * row + 2] * a2;
        }
    }
    if (!part) return;
    dot = block_sum256(dot, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = dot;
}

// r = b - q
__global__ void __launch_bounds__(C2_BLOCK) k_c2_init(int64_t n, const double* __restrict__ b,
                                                      const double* __restrict__ q, double* __restrict__ r) {
    for (int64_t e = (int64_t)blockIdx.x * C2_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * C2_BLOCK)
        r[e] = b[e] - q[e];
}

// x += alpha p, r -= alpha q
__global__ void __launch_bounds__(C2_BLOCK) k_c2_update(int64_t n, double* __restrict__ x, const double* __restrict__ p,
                                                        double* __restrict__ r, const double* __restrict__ q,
                                                        const C2State* __restrict__ st) {
    if (st->halt) return;
    const double al = st->alpha;
    for (int64_t e = (int64_t)blockIdx.x * C2_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * C2_BLOCK) {
        x[e] += al * p[e];
        r[e] = r[e] - al * q[e];
    }
}

// p = z + beta p (first: p = z)
__global__ void __launch_bounds__(C2_BLOCK) k_c2_pupdate(int64_t n, double* __restrict__ p, const double* __restrict__ z,
                                                         const C2State* __restrict__ st, int first) {
    if (st->halt) return;
    const double be = st->beta;
    for (int64_t e = (int64_t)blockIdx.x * C2_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * C2_BLOCK)
        p[e] = first ? z[e] : z[e] + be * p[e];
}

// One block: the partials summed in a fixed order (thread t adds blocks t, t + 256, ..., then the block tree) and the
// state stepped. phase 0: r0.z0; 1: p.q -> alpha and the guard; 2: r.z -> stop test, beta, count, history.
__global__ void __launch_bounds__(C2_BLOCK) k_c2_scalars(C2State* __restrict__ st, const double* __restrict__ part,
                                                         int nblocks, int phase, double* __restrict__ hist,
                                                         int64_t hist_len) {
    __shared__ double lds[4];
    if (st->halt) return;   // uniform: written by thread 0 only after the sum below
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += C2_BLOCK) s += part[i];
    s = block_sum256(s, lds);
    if (threadIdx.x != 0) return;
    if (phase == 0) {
        st->rz = s;
        if (st->max_iter <= 0) {
            st->status = FEM_PCG_MAXITER;
            st->halt = 1;
        }
    } else if (phase == 1) {
        st->pq = s;
        if (!(s > 0.0) || isinf(s)) {   // E^-1 is only numerically SPD: p.q <= 0 or non-finite
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
static int c2_grid_spmv(int64_t nslices) { return grid_multiple_of_xcd(cdiv(nslices, 4), C2_GRID_SPMV); }
static int c2_grid_vec(int64_t n) {
    const int64_t g = cdiv(n, C2_BLOCK);
    return (int)(g > C2_GRID_VEC ? C2_GRID_VEC : (g < 1 ? 1 : g));
}

static void c2_spmv(hipStream_t st, int64_t nrows, const int64_t* slice_ptr, const int32_t* cols, const int16_t* dcols,
                    const double* vals, const double* x, double* y, const C2State* state, double* part) {
    const int64_t nslices = cdiv(nrows, 64);
    const int grid = c2_grid_spmv(nslices);
    if (dcols)
        hipLaunchKernelGGL(k_c2_spmv<int16_t>, dim3(grid), dim3(C2_BLOCK), 0, st, nslices, nrows, slice_ptr, dcols,
                           vals, x, y, state, part);
    else
        hipLaunchKernelGGL(k_c2_spmv<int32_t>, dim3(grid), dim3(C2_BLOCK), 0, st, nslices, nrows, slice_ptr, cols, vals,
                           x, y, state, part);
}

static void c2_restrict(hipStream_t st, int k, const int32_t* agg_ptr, const int32_t* agg_nodes, const double* rel,
                        const double* w, const double* r, double* c, const C2State* state) {
    hipLaunchKernelGGL(k_c2_restrict, dim3(k), dim3(C2_BLOCK), 0, st, agg_ptr, agg_nodes, rel, w, r, c, state);
}

static void c2_apply(hipStream_t st, int64_t nrows, int k, const int32_t* agg, const double* rel, const double* w,
                     const double* Einv, const double* c, const double* r, double* y, double* z, const C2State* state,
                     double* part) {
    const int m = 6 * k;
    hipLaunchKernelGGL(k_c2_dense, dim3((unsigned)cdiv(m, 4)), dim3(C2_BLOCK), 0, st, m, Einv, c, y, state);
    hipLaunchKernelGGL(k_c2_prolong, dim3(c2_grid_vec(nrows)), dim3(C2_BLOCK), 0, st, nrows, agg, rel, w, y, r, z,
                       state, part);
}

static bool c2_dims_ok(const char* fn, int64_t nrows, int bs, int k) {
    if (bs != 3) {
        set_error("%s: block size %d unsupported (the rigid-body coarse space needs 3 translational dofs per node)", fn,
                  bs);
        return false;
    }
    if (nrows <= 0 || k < 1 || k > FEM_COARSE_MAX_AGG) {
        set_error("%s: needs rows and 1 to %d aggregates, got %lld rows, %d aggregates", fn, FEM_COARSE_MAX_AGG,
                  (long long)nrows, k);
        return false;
    }
    return true;
}

struct fem_pcg2 {
    int64_t nrows, n;
    int k;
    const int64_t* slice_ptr;
    const int32_t* cols;
    const int16_t* dcols;
    const double* vals;
    const double* b;
    double* x;
    const double* w;
    const int32_t *agg, *agg_ptr, *agg_nodes;
    const double *rel, *Einv;
    double tol;
    double* hist;
    int64_t hist_len;
    hipStream_t stream;
    int grid_spmv, grid_vec;
    void* block;   // one allocation: r, p, q, z, c, y, the two partial arrays, the state
    double *r, *p, *q, *z, *c, *y, *part_pq, *part_rz;
    C2State* st;
    C2State host;
};

static void c2_scalars(fem_pcg2* s, const double* part, int nblocks, int phase) {
    hipLaunchKernelGGL(k_c2_scalars, dim3(1), dim3(C2_BLOCK), 0, s->stream, s->st, part, nblocks, phase, s->hist,
                       s->hist_len);
}

static void c2_precondition(fem_pcg2* s) {
    c2_restrict(s->stream, s->k, s->agg_ptr, s->agg_nodes, s->rel, s->w, s->r, s->c, s->st);
    c2_apply(s->stream, s->nrows, s->k, s->agg, s->rel, s->w, s->Einv, s->c, s->r, s->y, s->z, s->st, s->part_rz);
}

static int c2_start(fem_pcg2* s, int max_iter) {
    C2State h{};
    h.tol = s->tol;
    h.max_iter = max_iter;
    s->host = h;
    FEM_HIP(hipMemcpyAsync(s->st, &s->host, sizeof(C2State), hipMemcpyHostToDevice, s->stream));
    c2_spmv(s->stream, s->nrows, s->slice_ptr, s->cols, s->dcols, s->vals, s->x, s->q, nullptr, nullptr);
    hipLaunchKernelGGL(k_c2_init, dim3(s->grid_vec), dim3(C2_BLOCK), 0, s->stream, s->n, s->b, s->q, s->r);
    c2_precondition(s);
    c2_scalars(s, s->part_rz, c2_grid_vec(s->nrows), 0);
    hipLaunchKernelGGL(k_c2_pupdate, dim3(s->grid_vec), dim3(C2_BLOCK), 0, s->stream, s->n, s->p, s->z,
                       (const C2State*)s->st, 1);
    FEM_LAUNCHED();
    return FEM_OK;
}

static int c2_iterate(fem_pcg2* s, int k) {
    for (int i = 0; i < k; ++i) {
        c2_spmv(s->stream, s->nrows, s->slice_ptr, s->cols, s->dcols, s->vals, s->p, s->q, s->st, s->part_pq);
        c2_scalars(s, s->part_pq, s->grid_spmv, 1);
        hipLaunchKernelGGL(k_c2_update, dim3(s->grid_vec), dim3(C2_BLOCK), 0, s->stream, s->n, s->x, s->p, s->r, s->q,
                           (const C2State*)s->st);
        c2_precondition(s);
        c2_scalars(s, s->part_rz, c2_grid_vec(s->nrows), 2);
        hipLaunchKernelGGL(k_c2_pupdate, dim3(s->grid_vec), dim3(C2_BLOCK), 0, s->stream, s->n, s->p, s->z,
                           (const C2State*)s->st, 0);
        FEM_LAUNCHED();
    }
    return FEM_OK;
}

static int c2_poll(fem_pcg2* s) {
    FEM_HIP(hipMemcpyAsync(&s->host, s->st, sizeof(C2State), hipMemcpyDeviceToHost, s->stream));
    FEM_HIP(hipStreamSynchronize(s->stream));
    return FEM_OK;
}

extern "C" {

int fem_coarse_restrict(int64_t nrows, int bs, int k, const int32_t* agg_ptr, const int32_t* agg_nodes,
                        const double* rel, const double* w, const double* r, double* c, fem_stream_t stream) {
    if (!c2_dims_ok("fem_coarse_restrict", nrows, bs, k)) return FEM_EARG;
    c2_restrict(S(stream), k, agg_ptr, agg_nodes, rel, w, r, c, nullptr);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_coarse_apply(int64_t nrows, int bs, int k, const int32_t* agg, const double* rel, const double* w,
                     const double* Einv, const double* c, const double* r, double* y, double* z, fem_stream_t stream) {
    if (!c2_dims_ok("fem_coarse_apply", nrows, bs, k)) return FEM_EARG;
    c2_apply(S(stream), nrows, k, agg, rel, w, Einv, c, r, y, z, nullptr, nullptr);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_coarse_galerkin_count(int64_t nrows, int bs, const int64_t* slice_ptr, const int32_t* cols,
                              const int16_t* dcols, const int32_t* agg, int64_t* count, fem_stream_t stream) {
    if (!c2_dims_ok("fem_coarse_galerkin_count", nrows, bs, 1)) return FEM_EARG;
    if (!cols && !dcols) {
        set_error("fem_coarse_galerkin_count: needs a column array");
        return FEM_EARG;
    }
    const int64_t nslices = cdiv(nrows, 64);
    const dim3 grid((unsigned)cdiv(nslices, 4));
    if (dcols)
        hipLaunchKernelGGL(k_c2_gal_count<int16_t>, grid, dim3(C2_BLOCK), 0, S(stream), nslices, nrows, slice_ptr,
                           dcols, agg, count);
    else
        hipLaunchKernelGGL(k_c2_gal_count<int32_t>, grid, dim3(C2_BLOCK), 0, S(stream), nslices, nrows, slice_ptr, cols,
                           agg, count);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_coarse_galerkin(int64_t nrows, int bs, int k, const int64_t* slice_ptr, const int32_t* cols,
                        const int16_t* dcols, const double* vals, const int32_t* agg, const double* rel,
                        const double* w, const int64_t* offset, int64_t* keys, double* rec, fem_stream_t stream) {
    if (!c2_dims_ok("fem_coarse_galerkin", nrows, bs, k)) return FEM_EARG;
    if (!cols && !dcols) {
        set_error("fem_coarse_galerkin: needs a column array");
        return FEM_EARG;
    }
    const int64_t nslices = cdiv(nrows, 64);
    const dim3 grid((unsigned)cdiv(nslices, 4));
    if (dcols)
        hipLaunchKernelGGL(k_c2_gal_emit<int16_t>, grid, dim3(C2_BLOCK), 0, S(stream), nslices, nrows, k, slice_ptr,
                           dcols, vals, agg, rel, w, offset, keys, rec);
    else
        hipLaunchKernelGGL(k_c2_gal_emit<int32_t>, grid, dim3(C2_BLOCK), 0, S(stream), nslices, nrows, k, slice_ptr,
                           cols, vals, agg, rel, w, offset, keys, rec);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_coarse_galerkin_sum(int64_t nkeys, int k, const int64_t* ukeys, const int64_t* key_ptr, const int64_t* order,
                            const double* rec, double* E, fem_stream_t stream) {
    if (nkeys < 0 || k < 1 || k > FEM_COARSE_MAX_AGG) {
        set_error("fem_coarse_galerkin_sum: %lld keys, %d aggregates", (long long)nkeys, k);
        return FEM_EARG;
    }
    if (nkeys == 0) return FEM_OK;
    hipLaunchKernelGGL(k_c2_gal_sum, dim3((unsigned)cdiv(nkeys, 4)), dim3(C2_BLOCK), 0, S(stream), nkeys, k, ukeys,
                       key_ptr, order, rec, E);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_pcg2_create(int64_t nrows, int bs, const int64_t* slice_ptr, const int32_t* cols, const int16_t* dcols,
                    const double* vals, const double* b, double* x, const double* w, int k, const int32_t* agg,
                    const int32_t* agg_ptr, const int32_t* agg_nodes, const double* rel, const double* Einv, double tol,
                    double* hist, int64_t hist_len, fem_stream_t stream, fem_pcg2** out) {
    if (!c2_dims_ok("fem_pcg2_create", nrows, bs, k)) return FEM_EARG;
    if ((!cols && !dcols) || !vals || !b || !x || !w || !agg || !agg_ptr || !agg_nodes || !rel || !Einv || !out) {
        set_error("fem_pcg2_create: needs a column array, the values, b, x, w and the coarse space's arrays");
        return FEM_EARG;
    }
    fem_pcg2* s = new fem_pcg2();
    s->nrows = nrows;
    s->n = nrows * 3;
    s->k = k;
    s->slice_ptr = slice_ptr;
    s->cols = cols;
    s->dcols = dcols;
    s->vals = vals;
    s->b = b;
    s->x = x;
    s->w = w;
    s->agg = agg;
    s->agg_ptr = agg_ptr;
    s->agg_nodes = agg_nodes;
    s->rel = rel;
    s->Einv = Einv;
    s->tol = tol;
    s->hist = hist;
    s->hist_len = hist ? hist_len : 0;
    s->stream = S(stream);
    s->grid_spmv = c2_grid_spmv(cdiv(nrows, 64));
    s->grid_vec = c2_grid_vec(s->n);
    const size_t vec = sizeof(double) * (size_t)s->n;
    const size_t cm = sizeof(double) * 6 * (size_t)k;
    const size_t ppq = sizeof(double) * (size_t)s->grid_spmv;
    const size_t prz = sizeof(double) * (size_t)c2_grid_vec(nrows);
    s->block = nullptr;
    const hipError_t e = hipMalloc(&s->block, 4 * vec + 2 * cm + ppq + prz + sizeof(C2State));
    if (e != hipSuccess) {
        set_error("fem_pcg2_create: allocation failed: %s", hipGetErrorString(e));
        delete s;
        return FEM_EHIP;
    }
    char* p = (char*)s->block;
    s->r = (double*)p;
    s->p = (double*)(p + vec);
    s->q = (double*)(p + 2 * vec);
    s->z = (double*)(p + 3 * vec);
    s->c = (double*)(p + 4 * vec);
    s->y = (double*)(p + 4 * vec + cm);
    s->part_pq = (double*)(p + 4 * vec + 2 * cm);
    s->part_rz = (double*)(p + 4 * vec + 2 * cm + ppq);
    s->st = (C2State*)(p + 4 * vec + 2 * cm + ppq + prz);
    *out = s;
    return FEM_OK;
}

int fem_pcg2_solve(fem_pcg2* s, int max_iter, int chunk, int* iters, int* status, double* rz) {
    int rc = c2_start(s, max_iter);
    if (rc) return rc;
    if (chunk <= 0) chunk = 32;
    int done = 0;
    while (done < max_iter) {
        const int k = chunk < max_iter - done ? chunk : max_iter - done;
        if ((rc = c2_iterate(s, k))) return rc;
        done += k;
        if ((rc = c2_poll(s))) return rc;
        if (s->host.halt) break;
    }
    if ((rc = c2_poll(s))) return rc;
    const C2State& c = s->host;
    if (iters) *iters = c.status == FEM_PCG_BREAKDOWN ? c.stop_iter : c.iter;
    if (status) *status = c.status;
    if (rz) *rz = c.iter > 0 ? c.rz_new : c.rz;
    return FEM_OK;
}

int fem_pcg2_scalars(fem_pcg2* s, double* out6) {
    const int rc = c2_poll(s);
    if (rc) return rc;
    const C2State& c = s->host;
    out6[0] = c.rz;
    out6[1] = c.pq;
    out6[2] = c.alpha;
    out6[3] = c.beta;
    out6[4] = c.rz_new;
    out6[5] = (double)c.iter;
    return FEM_OK;
}

void fem_pcg2_destroy(fem_pcg2* s) {
    if (!s) return;
    (void)hipStreamSynchronize(s->stream);
    if (s->block) (void)hipFree(s->block);
    delete s;
}

}  // extern "C"
