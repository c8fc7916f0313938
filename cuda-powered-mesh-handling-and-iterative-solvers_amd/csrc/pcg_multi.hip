// Multi-load-case (P)CG: NV right-hand sides solved in lock-step, the matrix streamed once per iteration for all.
//
// Multi-vectors are [n, NV] row-major (n = nrows * bs, the NV columns of one dof adjacent), so one gathered block
// column of the SpMM delivers bs * NV contiguous doubles (16-byte loads). The matrix is the plain SELL-64 layout of
// include/fem355.h. Every column is an independent CG / Jacobi-PCG of the single-vector context (pcg.hip: finish_pq /
// finish_rz semantics, `solver/solver.py:144-229` / `:766-812`) with its own alpha, beta, iteration count and status in
// a device state array; a column that stopped is frozen: its x, r and p are skipped by predicate from then on.
//
// Per iteration, plain launches on the stream (no workgroup depends on another within a launch):
//   k_mpcg_spmm<DOT>  : q = A p, per-block partials of p.q per column
//   k_mpcg_scalars(1) : partials summed in block order by ONE block -> alpha per column, CG guards
//   k_mpcg_update     : x += alpha p, r -= alpha q (CG: masked), per-block partials of r.z per column
//   k_mpcg_scalars(2) : -> stop test, beta, iteration count, history
//   k_mpcg_pupdate    : p = w r + beta p
// Reductions are finished by the next launch in a fixed order: results are bit-reproducible, and a column's bits do
// not depend on what the other columns hold. Grid sizes depend on (nslices, bs, NV) only.
#include "common.hpp"

namespace fem {

constexpr int M_BLOCK = 256;
constexpr int M_MAXNV = 8;
constexpr int M_GRID_SPMM = 2048;   // cap of the grids that write partials: the one-block scalar kernel reads at
constexpr int M_GRID_VEC = 1024;    // most this many partials per column

struct MCol {
    double rz, pq, alpha, beta, rz_new, tol;
    int iter;        // completed iterations
    int status;      // FEM_PCG_*
    int halt;        // 1: the column is frozen
    int stop_iter;   // reported iteration of a guard stop
};
struct MState {
    MCol c[M_MAXNV];
    double eps;
    int mode, max_iter;
    int nrun;        // columns still running: 0 turns every iteration kernel into a no-op
    int pad_;
};

// ---------------------------------------------------------------- SpMM (+ p.q partials)
// One wave per slice, one lane per block row; per stored block: the column, the bs^2 value planes (coalesced,
// nontemporal as in the single-vector PCG kernels) and the bs * NV gathered doubles, then the FMAs in (k, r, j)
// order -- the per-row summation order of pcg.hip's sell_row for every column.
// Lanes of the last slice past nrows: the pattern stores column nrows - 1 and zero values there (pattern.hip); the
// kernel gathers row 0 for them whatever the pattern says and never stores their rows.
template <int BS, int NV, typename CI, bool DOT>
__global__ void __launch_bounds__(M_BLOCK) k_mpcg_spmm(int64_t nslices, int64_t nrows,
                                                       const int64_t* __restrict__ slice_ptr,
                                                       const CI* __restrict__ cols, const double* __restrict__ vals,
                                                       const double* __restrict__ X, double* __restrict__ Y,
                                                       const MState* __restrict__ st, double* __restrict__ part) {
    constexpr int U = BS == 1 ? 4 : 1;          // entries in flight per lane
    constexpr int NP = BS * NV / 2;             // 16-byte pieces of one gathered block column
    __shared__ double lds[4 * NV];
    if (DOT && st->nrun == 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double dot[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) dot[v] = 0.0;
    // XCD-aware walk (as pcg.hip's slice_walk): XCD blockIdx % 8 owns a contiguous slice range
    const int xcd = blockIdx.x % NXCD;
    const int64_t lb = blockIdx.x / NXCD, nlb = gridDim.x / NXCD;
    const int64_t spx = (nslices + NXCD - 1) / NXCD;
    const int64_t s_begin = (int64_t)xcd * spx;
    const int64_t s_end = s_begin + spx < nslices ? s_begin + spx : nslices;
    for (int64_t s = s_begin + lb * 4 + wave; s < s_end; s += nlb * 4) {
        const int64_t p0 = slice_ptr[s];
        const int w = (int)((slice_ptr[s + 1] - p0) >> 6);
        const int64_t row = s * 64 + lane;
        const bool live = row < nrows;
        const CI* c = cols + p0 + lane;
        const double* v = vals + p0 * (BS * BS) + lane;
        double acc[BS][NV];
#pragma unroll
        for (int r = 0; r < BS; ++r)
#pragma unroll
            for (int j = 0; j < NV; ++j) acc[r][j] = 0.0;
        for (int k0 = 0; k0 < w; k0 += U) {
            int64_t cc[U];
            double vv[U][BS * BS];
            double2 xv[U][NP];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int64_t col = 0;
                if (k0 + u < w) {
                    const int64_t ci = (int64_t)c[(int64_t)64 * (k0 + u)];
                    col = sizeof(CI) == 2 ? row + ci : ci;
                }
                cc[u] = live ? col : 0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double* vk = v + (int64_t)64 * BS * BS * (k0 + u);
#pragma unroll
                for (int e = 0; e < BS * BS; ++e)
                    vv[u][e] = (k0 + u < w) ? __builtin_nontemporal_load(vk + 64 * e) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double2* xp = reinterpret_cast<const double2*>(X + cc[u] * (BS * NV));
#pragma unroll
                for (int e = 0; e < NP; ++e) xv[u][e] = xp[e];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k0 + u < w) {
#pragma unroll
                    for (int r = 0; r < BS; ++r)
#pragma unroll
                        for (int j = 0; j < BS; ++j)
#pragma unroll
                            for (int e = 0; e < NV / 2; ++e) {
                                acc[r][2 * e] += vv[u][r * BS + j] * xv[u][j * (NV / 2) + e].x;
                                acc[r][2 * e + 1] += vv[u][r * BS + j] * xv[u][j * (NV / 2) + e].y;
                            }
                }
        }
        if (live) {
            double2* yp = reinterpret_cast<double2*>(Y + row * (BS * NV));
#pragma unroll
            for (int r = 0; r < BS; ++r)
#pragma unroll
                for (int e = 0; e < NV / 2; ++e) yp[r * (NV / 2) + e] = make_double2(acc[r][2 * e], acc[r][2 * e + 1]);
            if (DOT) {
                const double2* pp = reinterpret_cast<const double2*>(X + row * (BS * NV));
#pragma unroll
                for (int r = 0; r < BS; ++r)
#pragma unroll
                    for (int e = 0; e < NV / 2; ++e) {
                        const double2 pv = pp[r * (NV / 2) + e];
                        dot[2 * e] += pv.x * acc[r][2 * e];
                        dot[2 * e + 1] += pv.y * acc[r][2 * e + 1];
                    }
            }
        }
    }
    if (!DOT) return;
#pragma unroll
    for (int v = 0; v < NV; ++v) dot[v] = wave_sum(dot[v]);
    if (lane == 0) {
#pragma unroll
        for (int v = 0; v < NV; ++v) lds[wave * NV + v] = dot[v];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int t = threadIdx.x;
        part[(int64_t)blockIdx.x * NV + t] = (lds[t] + lds[NV + t]) + (lds[2 * NV + t] + lds[3 * NV + t]);
    }
}

// ---------------------------------------------------------------- vector kernels
// The multi-vectors are walked as flat arrays of 16-byte column pairs: thread e handles pair e % (NV / 2) of dof
// e / (NV / 2), so a thread sees the same two columns in every step of its grid-stride loop (block and grid sizes are
// multiples of NV / 2) and every load of a wave is contiguous.

// per-block partials of the two columns of every thread's pair: lanes of equal pair summed by a fixed shuffle tree,
// the four waves added in a fixed order, part[block][NV]
template <int NV>
__device__ __forceinline__ void pair_partials(double a0, double a1, double* lds, double* __restrict__ part) {
    constexpr int H = NV / 2;
#pragma unroll
    for (int o = 32; o >= H; o >>= 1) {
        a0 += __shfl_xor(a0, o, 64);
        a1 += __shfl_xor(a1, o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < H) {
        lds[wave * NV + 2 * lane] = a0;
        lds[wave * NV + 2 * lane + 1] = a1;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int t = threadIdx.x;
        part[(int64_t)blockIdx.x * NV + t] = (lds[t] + lds[NV + t]) + (lds[2 * NV + t] + lds[3 * NV + t]);
    }
}

// CG mode: x = 0 on the fixed dofs (w == 0), every column
template <int NV>
__global__ void __launch_bounds__(M_BLOCK) k_mpcg_zero_fixed(int64_t n, double2* __restrict__ x,
                                                             const double* __restrict__ w) {
    constexpr int H = NV / 2;
    const int64_t total = n * H;
    for (int64_t e = (int64_t)blockIdx.x * M_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * M_BLOCK)
        if (w[e / H] == 0.0) x[e] = make_double2(0.0, 0.0);
}

// start: r = b - q (q = A x0; CG: masked), p = z = w r, partials of r.z -- every column, padding columns included
// (their b and x are zero, so their r and p are written as zeros)
template <int NV>
__global__ void __launch_bounds__(M_BLOCK) k_mpcg_init(int64_t n, const double2* __restrict__ b,
                                                       const double2* __restrict__ q, const double* __restrict__ w,
                                                       double2* __restrict__ r, double2* __restrict__ p,
                                                       const MState* __restrict__ st, double* __restrict__ part) {
    constexpr int H = NV / 2;
    __shared__ double lds[4 * NV];
    const bool cg = st->mode != FEM_MODE_PCG;
    const int64_t total = n * H;
    double a0 = 0.0, a1 = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * M_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * M_BLOCK) {
        const double wv = w[e / H];
        const double2 bv = b[e], qv = q[e];
        double2 rv = make_double2(bv.x - qv.x, bv.y - qv.y);
        if (cg && wv == 0.0) rv = make_double2(0.0, 0.0);
        const double2 zv = make_double2(wv * rv.x, wv * rv.y);
        r[e] = rv;
        p[e] = zv;
        a0 += rv.x * zv.x;
        a1 += rv.y * zv.y;
    }
    pair_partials<NV>(a0, a1, lds, part);
}

// x += alpha p, r -= alpha q (CG: r = 0 on the fixed dofs), partials of r.z -- running columns only
template <int NV>
__global__ void __launch_bounds__(M_BLOCK) k_mpcg_update(int64_t n, double2* __restrict__ x,
                                                         const double2* __restrict__ p, double2* __restrict__ r,
                                                         const double2* __restrict__ q, const double* __restrict__ w,
                                                         const MState* __restrict__ st, double* __restrict__ part) {
    constexpr int H = NV / 2;
    __shared__ double lds[4 * NV];
    if (st->nrun == 0) return;
    const int c0 = 2 * (threadIdx.x % H);
    const bool run0 = !st->c[c0].halt, run1 = !st->c[c0 + 1].halt;
    const double al0 = st->c[c0].alpha, al1 = st->c[c0 + 1].alpha;
    const bool cg = st->mode != FEM_MODE_PCG;
    const int64_t total = n * H;
    double a0 = 0.0, a1 = 0.0;
    if (run0 || run1) {
        for (int64_t e = (int64_t)blockIdx.x * M_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * M_BLOCK) {
            const double wv = w[e / H];
            const double2 pv = p[e], qv = q[e];
            double2 xv = x[e], rv = r[e];
            if (run0) {
                xv.x += al0 * pv.x;
                rv.x = rv.x - al0 * qv.x;
                if (cg && wv == 0.0) rv.x = 0.0;
                a0 += rv.x * (wv * rv.x);
            }
            if (run1) {
                xv.y += al1 * pv.y;
                rv.y = rv.y - al1 * qv.y;
                if (cg && wv == 0.0) rv.y = 0.0;
                a1 += rv.y * (wv * rv.y);
            }
            x[e] = xv;   // a frozen column of the pair gets its own bits back
            r[e] = rv;
        }
    }
    pair_partials<NV>(a0, a1, lds, part);
}

// p = w r + beta p -- running columns only (a column that stopped in this iteration keeps its p)
template <int NV>
__global__ void __launch_bounds__(M_BLOCK) k_mpcg_pupdate(int64_t n, double2* __restrict__ p,
                                                          const double2* __restrict__ r, const double* __restrict__ w,
                                                          const MState* __restrict__ st) {
    constexpr int H = NV / 2;
    if (st->nrun == 0) return;
    const int c0 = 2 * (threadIdx.x % H);
    const bool run0 = !st->c[c0].halt, run1 = !st->c[c0 + 1].halt;
    if (!run0 && !run1) return;
    const double be0 = st->c[c0].beta, be1 = st->c[c0 + 1].beta;
    const int64_t total = n * H;
    for (int64_t e = (int64_t)blockIdx.x * M_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * M_BLOCK) {
        const double wv = w[e / H];
        const double2 rv = r[e];
        double2 pv = p[e];
        if (run0) pv.x = wv * rv.x + be0 * pv.x;
        if (run1) pv.y = wv * rv.y + be1 * pv.y;
        p[e] = pv;
    }
}

// ---------------------------------------------------------------- scalars (one block)
// Sums part[nblocks][nv] per column in a fixed order (a wave per column: lane l adds blocks l, l + 64, ... in order,
// then the wave tree) and steps the column's state. phase 0: r0.z0; 1: p.q -> alpha, CG guards (pcg.hip finish_pq);
// 2: r.z -> stop test, beta, iteration count, history (finish_rz), then FEM_PCG_MAXITER. Frozen columns are skipped.
__global__ void __launch_bounds__(M_BLOCK) k_mpcg_scalars(MState* __restrict__ st, const double* __restrict__ part,
                                                          int nblocks, int nv, int phase, double* __restrict__ hist,
                                                          int64_t hist_len) {
    __shared__ int running[M_MAXNV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (phase != 0 && st->nrun == 0) return;
    for (int v = wave; v < nv; v += 4) {
        MCol* c = &st->c[v];
        int halt = c->halt;
        if (!(phase != 0 && halt)) {
            double s = 0.0;
            for (int i = lane; i < nblocks; i += 64) s += part[(int64_t)i * nv + v];
            s = wave_sum(s);
            if (lane == 0) {
                const bool cg = st->mode != FEM_MODE_PCG;
                const double eps = st->eps;
                if (phase == 0) {
                    c->rz = s;
                    if (!halt && st->max_iter <= 0) {
                        c->status = FEM_PCG_MAXITER;
                        halt = 1;
                    }
                } else if (phase == 1) {
                    c->pq = s;
                    if (cg) {
                        if (fabs(s) < eps || s < 0.0) {               // `solver/solver.py:187`
                            c->status = FEM_PCG_BREAKDOWN;
                            c->stop_iter = c->iter + 1;
                            halt = 1;
                        } else {
                            const double a = c->rz / (s + eps);       // `:194`
                            c->alpha = a;
                            if (isnan(a) || isinf(a)) {               // `:196`
                                c->status = FEM_PCG_ALPHA_NAN;
                                c->stop_iter = c->iter + 1;
                                halt = 1;
                            }
                        }
                    } else {
                        c->alpha = c->rz / s;                         // `:800` (no guards)
                    }
                } else {
                    const int it = c->iter;
                    c->rz_new = s;
                    c->iter = it + 1;
                    const double nrm = sqrt(s);
                    if (hist && it < hist_len) hist[(int64_t)it * nv + v] = nrm;
                    if (nrm < c->tol) {                               // `:210` / `:805`
                        c->status = FEM_PCG_CONVERGED;
                        c->stop_iter = it + 1;
                        halt = 1;
                    } else {
                        const double b = cg ? s / (c->rz + eps) : s / c->rz;   // `:213` / `:808`
                        c->beta = b;
                        if (cg && (isnan(b) || isinf(b))) {           // `:214`
                            c->status = FEM_PCG_BETA_NAN;
                            c->stop_iter = it + 1;
                            halt = 1;
                        } else if (it + 1 >= st->max_iter) {
                            c->status = FEM_PCG_MAXITER;
                            halt = 1;
                        }
                        c->rz = s;
                    }
                }
                c->halt = halt;
            }
        }
        if (lane == 0) running[v] = !halt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int v = 0; v < nv; ++v) n += running[v];
        st->nrun = n;
    }
}

}  // namespace fem

using namespace fem;

// ---------------------------------------------------------------- host side
struct fem_mpcg {
    int64_t nrows, n, nslices;
    int bs, nv, nactive, mode;
    const int64_t* slice_ptr;
    const int32_t* cols;
    const int16_t* dcols;
    const double* vals;
    const double* B;
    double* X;
    const double* w;
    double eps;
    double tol[M_MAXNV];
    double* hist;
    int64_t hist_len;
    hipStream_t stream;
    int grid_spmm, grid_vec;
    void* block;          // one allocation: r, p, q, the two partial arrays, the state
    double *r, *p, *q, *part_pq, *part_rz;
    MState* st;
    MState host;
};

static bool mp_dims_ok(const char* fn, int bs, int nv) {
    if (bs != 1 && bs != 3) {
        set_error("%s: block size %d unsupported (1 or 3)", fn, bs);
        return false;
    }
    if (nv != 2 && nv != 4 && nv != 8) {
        set_error("%s: %d columns unsupported (the multi-vector kernels are built for 2, 4 and 8)", fn, nv);
        return false;
    }
    return true;
}

static int mp_grid_spmm(int64_t nslices) { return grid_multiple_of_xcd(cdiv(nslices, 4), M_GRID_SPMM); }
// from the padded row count, so that the grid depends on (nslices, bs, nv) only
static int mp_grid_vec(int64_t nslices, int bs, int nv) {
    return grid_multiple_of_xcd(cdiv(nslices * 64 * bs * (nv / 2), M_BLOCK), M_GRID_VEC);
}

template <int BS, int NV, bool DOT>
static void mp_spmm_ci(int grid, hipStream_t st, int64_t nslices, int64_t nrows, const int64_t* slice_ptr,
                       const int32_t* cols, const int16_t* dcols, const double* vals, const double* X, double* Y,
                       const MState* state, double* part) {
    if (dcols)
        hipLaunchKernelGGL((k_mpcg_spmm<BS, NV, int16_t, DOT>), dim3(grid), dim3(M_BLOCK), 0, st, nslices, nrows,
                           slice_ptr, dcols, vals, X, Y, state, part);
    else
        hipLaunchKernelGGL((k_mpcg_spmm<BS, NV, int32_t, DOT>), dim3(grid), dim3(M_BLOCK), 0, st, nslices, nrows,
                           slice_ptr, cols, vals, X, Y, state, part);
}

template <bool DOT>
static int mp_spmm(int bs, int nv, int grid, hipStream_t st, int64_t nslices, int64_t nrows, const int64_t* slice_ptr,
                   const int32_t* cols, const int16_t* dcols, const double* vals, const double* X, double* Y,
                   const MState* state, double* part) {
#define MP_CASE(B, V)                                                                                            \
    if (bs == B && nv == V)                                                                                      \
        mp_spmm_ci<B, V, DOT>(grid, st, nslices, nrows, slice_ptr, cols, dcols, vals, X, Y, state, part);
    MP_CASE(1, 2) MP_CASE(1, 4) MP_CASE(1, 8) MP_CASE(3, 2) MP_CASE(3, 4) MP_CASE(3, 8)
#undef MP_CASE
    FEM_LAUNCHED();
    return FEM_OK;
}

extern "C" {

int fem_spmm(int64_t nrows, int bs, int nv, const int64_t* slice_ptr, const int32_t* cols, const int16_t* dcols,
             const double* vals, const double* X, double* Y, fem_stream_t stream) {
    if (!mp_dims_ok("fem_spmm", bs, nv)) return FEM_EARG;
    if (nrows <= 0 || (!cols && !dcols) || (((uintptr_t)X | (uintptr_t)Y) & 15)) {
        set_error("fem_spmm: needs rows, a column array and 16-byte aligned multi-vectors");
        return FEM_EARG;
    }
    const int64_t nslices = cdiv(nrows, 64);
    return mp_spmm<false>(bs, nv, mp_grid_spmm(nslices), S(stream), nslices, nrows, slice_ptr, cols, dcols, vals, X, Y,
                          nullptr, nullptr);
}

int fem_mpcg_create(int64_t nrows, int bs, int nv, int nactive, const int64_t* slice_ptr, const int32_t* cols,
                    const int16_t* dcols, const double* vals, const double* B, double* X, const double* w, int mode,
                    const double* tol, double eps, double* hist, int64_t hist_len, fem_stream_t stream,
                    fem_mpcg** out) {
    if (!mp_dims_ok("fem_mpcg_create", bs, nv)) return FEM_EARG;
    if (mode != FEM_MODE_CG_STABLE && mode != FEM_MODE_PCG) {
        set_error("fem_mpcg_create: mode %d unsupported (FEM_MODE_CG_STABLE or FEM_MODE_PCG; constraints take one "
                  "right-hand side: fem_pcg_create)", mode);
        return FEM_EARG;
    }
    if (nactive < 1 || nactive > nv) {
        set_error("fem_mpcg_create: %d active columns of %d", nactive, nv);
        return FEM_EARG;
    }
    if (nrows <= 0 || (!cols && !dcols) || !tol || (((uintptr_t)B | (uintptr_t)X) & 15)) {
        set_error("fem_mpcg_create: needs rows, a column array, tolerances and 16-byte aligned multi-vectors");
        return FEM_EARG;
    }
    fem_mpcg* s = new fem_mpcg();
    s->nrows = nrows;
    s->bs = bs;
    s->nv = nv;
    s->nactive = nactive;
    s->mode = mode;
    s->n = nrows * bs;
    s->nslices = cdiv(nrows, 64);
    s->slice_ptr = slice_ptr;
    s->cols = cols;
    s->dcols = dcols;
    s->vals = vals;
    s->B = B;
    s->X = X;
    s->w = w;
    s->eps = eps;
    for (int v = 0; v < M_MAXNV; ++v) s->tol[v] = v < nactive ? tol[v] : 0.0;
    s->hist = hist;
    s->hist_len = hist ? hist_len : 0;
    s->stream = S(stream);
    s->grid_spmm = mp_grid_spmm(s->nslices);
    s->grid_vec = mp_grid_vec(s->nslices, bs, nv);
    const size_t vec = sizeof(double) * (size_t)s->n * (size_t)nv;   // a multiple of 16
    const size_t ppq = sizeof(double) * (size_t)s->grid_spmm * (size_t)nv;
    const size_t prz = sizeof(double) * (size_t)s->grid_vec * (size_t)nv;
    s->block = nullptr;
    const hipError_t e = hipMalloc(&s->block, 3 * vec + ppq + prz + sizeof(MState));
    if (e != hipSuccess) {
        set_error("fem_mpcg_create: allocation failed: %s", hipGetErrorString(e));
        delete s;
        return FEM_EHIP;
    }
    char* b = (char*)s->block;
    s->r = (double*)b;
    s->p = (double*)(b + vec);
    s->q = (double*)(b + 2 * vec);
    s->part_pq = (double*)(b + 3 * vec);
    s->part_rz = (double*)(b + 3 * vec + ppq);
    s->st = (MState*)(b + 3 * vec + ppq + prz);
    *out = s;
    return FEM_OK;
}

void fem_mpcg_destroy(fem_mpcg* s) {
    if (!s) return;
    (void)hipStreamSynchronize(s->stream);
    if (s->block) (void)hipFree(s->block);
    delete s;
}

}  // extern "C"

#define MP_NV(fn, ...)                         \
    do {                                       \
        if (s->nv == 2) fn<2> __VA_ARGS__;     \
        else if (s->nv == 4) fn<4> __VA_ARGS__; \
        else fn<8> __VA_ARGS__;                \
    } while (0)

template <int NV>
static void mp_zero_fixed(fem_mpcg* s) {
    hipLaunchKernelGGL(k_mpcg_zero_fixed<NV>, dim3(s->grid_vec), dim3(M_BLOCK), 0, s->stream, s->n, (double2*)s->X,
                       s->w);
}
template <int NV>
static void mp_init(fem_mpcg* s) {
    hipLaunchKernelGGL(k_mpcg_init<NV>, dim3(s->grid_vec), dim3(M_BLOCK), 0, s->stream, s->n, (const double2*)s->B,
                       (const double2*)s->q, s->w, (double2*)s->r, (double2*)s->p, (const MState*)s->st, s->part_rz);
}
template <int NV>
static void mp_update(fem_mpcg* s) {
    hipLaunchKernelGGL(k_mpcg_update<NV>, dim3(s->grid_vec), dim3(M_BLOCK), 0, s->stream, s->n, (double2*)s->X,
                       (const double2*)s->p, (double2*)s->r, (const double2*)s->q, s->w, (const MState*)s->st,
                       s->part_rz);
}
template <int NV>
static void mp_pupdate(fem_mpcg* s) {
    hipLaunchKernelGGL(k_mpcg_pupdate<NV>, dim3(s->grid_vec), dim3(M_BLOCK), 0, s->stream, s->n, (double2*)s->p,
                       (const double2*)s->r, s->w, (const MState*)s->st);
}

static void mp_scalars(fem_mpcg* s, const double* part, int nblocks, int phase) {
    hipLaunchKernelGGL(k_mpcg_scalars, dim3(1), dim3(M_BLOCK), 0, s->stream, s->st, part, nblocks, s->nv, phase,
                       s->hist, s->hist_len);
}

static int mp_start(fem_mpcg* s, int max_iter) {
    MState h{};
    h.eps = s->eps;
    h.mode = s->mode;
    h.max_iter = max_iter;
    h.nrun = s->nactive;
    for (int v = 0; v < M_MAXNV; ++v) {
        h.c[v].tol = s->tol[v];
        h.c[v].halt = v < s->nactive ? 0 : 1;   // padding columns are frozen from the start
    }
    s->host = h;
    FEM_HIP(hipMemcpyAsync(s->st, &s->host, sizeof(MState), hipMemcpyHostToDevice, s->stream));
    if (s->mode == FEM_MODE_CG_STABLE) {
        MP_NV(mp_zero_fixed, (s));
        FEM_LAUNCHED();
    }
    const int rc = mp_spmm<false>(s->bs, s->nv, s->grid_spmm, s->stream, s->nslices, s->nrows, s->slice_ptr, s->cols,
                                  s->dcols, s->vals, s->X, s->q, nullptr, nullptr);
    if (rc) return rc;
    MP_NV(mp_init, (s));
    FEM_LAUNCHED();
    mp_scalars(s, s->part_rz, s->grid_vec, 0);
    FEM_LAUNCHED();
    return FEM_OK;
}

static int mp_iterate(fem_mpcg* s, int k) {
    for (int i = 0; i < k; ++i) {
        const int rc = mp_spmm<true>(s->bs, s->nv, s->grid_spmm, s->stream, s->nslices, s->nrows, s->slice_ptr,
                                     s->cols, s->dcols, s->vals, s->p, s->q, s->st, s->part_pq);
        if (rc) return rc;
        mp_scalars(s, s->part_pq, s->grid_spmm, 1);
        MP_NV(mp_update, (s));
        mp_scalars(s, s->part_rz, s->grid_vec, 2);
        MP_NV(mp_pupdate, (s));
        FEM_LAUNCHED();
    }
    return FEM_OK;
}

static int mp_poll(fem_mpcg* s) {
    FEM_HIP(hipMemcpyAsync(&s->host, s->st, sizeof(MState), hipMemcpyDeviceToHost, s->stream));
    FEM_HIP(hipStreamSynchronize(s->stream));
    return FEM_OK;
}

extern "C" {

int fem_mpcg_solve(fem_mpcg* s, int max_iter, int chunk, int* iters, int* status, double* rz) {
    int rc = mp_start(s, max_iter);
    if (rc) return rc;
    if (chunk <= 0) chunk = 32;
    int done = 0;
    while (done < max_iter) {
        const int k = chunk < max_iter - done ? chunk : max_iter - done;
        if ((rc = mp_iterate(s, k))) return rc;
        done += k;
        if ((rc = mp_poll(s))) return rc;
        if (s->host.nrun == 0) break;
        if (chunk < 256) chunk *= 2;   // poll less often once the solve is clearly long
    }
    if ((rc = mp_poll(s))) return rc;
    for (int v = 0; v < s->nactive; ++v) {
        const MCol& c = s->host.c[v];
        // guard stops report the reference's printed iteration, every other status the completed iterations
        if (iters) iters[v] = (c.status == FEM_PCG_BREAKDOWN || c.status == FEM_PCG_ALPHA_NAN) ? c.stop_iter : c.iter;
        if (status) status[v] = c.status;
        if (rz) rz[v] = c.iter > 0 ? c.rz_new : c.rz;
    }
    return FEM_OK;
}

int fem_mpcg_scalars(fem_mpcg* s, double* out) {
    const int rc = mp_poll(s);
    if (rc) return rc;
    for (int v = 0; v < s->nactive; ++v) {
        const MCol& c = s->host.c[v];
        double* o = out + 6 * v;
        o[0] = c.rz;
        o[1] = c.pq;
        o[2] = c.alpha;
        o[3] = c.beta;
        o[4] = c.rz_new;
        o[5] = (double)c.iter;
    }
    return FEM_OK;
}

}  // extern "C"
