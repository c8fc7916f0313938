// Transient dynamics: the kernels of the implicit Newmark integrator for M a + C v + K u = f(t) with Rayleigh damping
// C = alpha M + beta_R K (system.py NewmarkIntegrator; the reference has no time integration).
//
//   k_axpby_mass (+ k_axpby_diag)      : K_eff = cK K + cM M in K's own layout, once per run
//   k_newmark_rhs                      : b = amp F + M yM + K yK in ONE sweep of the SELL-64 pattern, per step
//   k_newmark_update                   : a, v, u and the next step's (yK | yM) from the solve's x, one pass, per step
//   k_quadform_km (+ k_quadform_sum)   : (x^T K x, y^T M y) in one sweep, for the energy
// The rules of modal.hip hold: plain launches only; no workgroup waits on another; no floating-point atomics; every
// reduction is written as per-workgroup partials and summed in workgroup order by the following one-workgroup launch,
// so results are bit-reproducible. Rows >= n are never read nor stored. The matrix streams are read with nontemporal
// loads; K is read in the layout it is held in (the plain planes, or the bs = 3 layout A of include/fem355.h).
#include "common.hpp"

namespace fem {

constexpr int T_BLOCK = 256;
constexpr int T_GRID_SWEEP = 2048;   // as modal.hip's K/M product
constexpr int T_GRID_VEC = 1024;

typedef double dbl2 __attribute__((ext_vector_type(2)));   // a 16-byte value the nontemporal builtin takes

// ---------------------------------------------------------------- K_eff = cK K + cM M
// Flat walk in 16-byte pairs over the value array. Both layouts keep the bs^2 values of the 64 entries (slice base +
// 64 k + lane) in one chunk of 64 bs^2 doubles, so the entry of a value follows from its position alone:
//   plain : value rc of lane l at 64 rc + l                      -> a pair holds value rc of lanes l, l + 1
//   A     : values (2t, 2t + 1) of lane l at 128 t + 2 l, value 8 at 512 + l -> a pair below 512 holds two values of
//           one lane, above it value 8 of two lanes
// MASS_SELL: value rc = r bs + r gets cM ms[entry] (M = M_s (x) I_bs); padding entries hold 0 in both matrices and
// stay 0. MASS_DIAG: the sweep scales K alone and k_axpby_diag then writes the rows' diagonal entries.
template <int BS, int LA, int MASS>
__global__ void __launch_bounds__(T_BLOCK) k_axpby_mass(int64_t npairs, const dbl2* __restrict__ K,
                                                        const double* __restrict__ ms, double cK, double cM,
                                                        dbl2* __restrict__ out) {
    constexpr int CH = 32 * BS * BS;   // pairs per chunk
    for (int64_t i = (int64_t)blockIdx.x * T_BLOCK + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * T_BLOCK) {
        const dbl2 k = __builtin_nontemporal_load(K + i);
        dbl2 o;
        o.x = cK * k.x;
        o.y = cK * k.y;
        if (MASS == FEM_MASS_SELL) {
            const int64_t ch = i / CH;
            const int q = (int)(i - ch * CH) * 2;   // position of the pair's first double in the chunk
            const double* m = ms + ch * 64;
            if (BS == 1) {
                o.x = cK * k.x + cM * __builtin_nontemporal_load(m + q);
                o.y = cK * k.y + cM * __builtin_nontemporal_load(m + q + 1);
            } else if (LA) {
                if (q >= 512) {   // value 8 of lanes q - 512, q - 511
                    o.x = cK * k.x + cM * m[q - 512];
                    o.y = cK * k.y + cM * m[q - 511];
                } else if ((q >> 7) == 0 || (q >> 7) == 2) {   // values (0, 1) or (4, 5) of lane (q % 128) / 2
                    o.x = cK * k.x + cM * m[(q & 127) >> 1];
                }
            } else {
                const int rc = q >> 6;
                if (rc == 0 || rc == 4 || rc == 8) {   // a diagonal plane: lanes q % 64, q % 64 + 1
                    o.x = cK * k.x + cM * m[q & 63];
                    o.y = cK * k.y + cM * m[(q & 63) + 1];
                }
            }
        }
        out[i] = o;
    }
}

// the diagonal mass: value (r, r) of each row's own block (slot diagpos - rowptr of the row, as k_jacobi finds it)
template <int BS, int LA>
__global__ void __launch_bounds__(T_BLOCK) k_axpby_diag(int64_t nrows, const int64_t* __restrict__ slice_ptr,
                                                        const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ diagpos,
                                                        const double* __restrict__ K, const double* __restrict__ d,
                                                        double cK, double cM, double* __restrict__ out) {
    const int64_t n = nrows * BS;
    for (int64_t i = (int64_t)blockIdx.x * T_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * T_BLOCK) {
        const int64_t node = i / BS;
        const int r = (int)(i - node * BS);
        const int32_t dp = diagpos[node];
        if (dp < 0) continue;   // a node no element touches: no entry
        const int64_t E = slice_ptr[node >> 6] + (int64_t)(dp - rowptr[node]) * 64 + (node & 63);
        const int rc = r * BS + r;
        const int64_t pos = LA ? sell_val_a(E, rc) : (E - (E & 63)) * (BS * BS) + (int64_t)rc * 64 + (E & 63);
        out[pos] = cK * K[pos] + cM * d[i];
    }
}

// ---------------------------------------------------------------- the pattern walk shared by the two sweeps
// modal.hip's k_spmm_km at NV = 2 (one wave per slice, one lane per block row, entries in k order): X [n, 2] row-major,
// column 0 feeds the K block and column 1 the scalar mass, so the 16-byte gather of a dof serves both. HASK = false
// drops the K stream (8 + 2 bytes per entry instead of 8 bs^2 + 8 + 2). FUSE: both products go into ONE accumulator
// per row (the right-hand side), else into two (the quadratic forms). Returns with accK / accM of the lane's block row.
template <int BS, typename CI, int MASS, int LA, bool HASK, bool FUSE>
__device__ __forceinline__ void km_row_walk(int64_t p0, int w, int64_t row, bool live, int lane,
                                            const CI* __restrict__ cols, const double* __restrict__ vals,
                                            const double* __restrict__ mass, const double* __restrict__ X,
                                            double (&accK)[BS], double (&accM)[BS]) {
    constexpr int U = (BS == 1 || !HASK) ? 4 : 1;   // entries in flight per lane
    constexpr int B2 = BS * BS;
    const CI* c = cols + p0 + lane;
    const double* mp = mass + p0 + lane;
    for (int k0 = 0; k0 < w; k0 += U) {
        int64_t cc[U];
        double vv[U][B2], mv[U];
        double2 xv[U][BS];
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
            const bool in = k0 + u < w;
#pragma unroll
            for (int e = 0; e < B2; ++e) vv[u][e] = 0.0;
            if (HASK && in) {
                const double* vk = vals + (p0 + (int64_t)64 * (k0 + u)) * B2;
                if (LA) {   // layout A (BS = 3): four 16-byte pairs and value 8
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const dbl2 pr = __builtin_nontemporal_load(reinterpret_cast<const dbl2*>(vk + 128 * t) + lane);
                        vv[u][2 * t] = pr.x;
                        vv[u][2 * t + 1] = pr.y;
                    }
                    vv[u][B2 - 1] = __builtin_nontemporal_load(vk + 512 + lane);
                } else {
#pragma unroll
                    for (int e = 0; e < B2; ++e) vv[u][e] = __builtin_nontemporal_load(vk + 64 * e + lane);
                }
            }
            mv[u] = 0.0;
            if (MASS == FEM_MASS_SELL && in) mv[u] = __builtin_nontemporal_load(mp + (int64_t)64 * (k0 + u));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double2* xp = reinterpret_cast<const double2*>(X + cc[u] * (BS * 2));
#pragma unroll
            for (int j = 0; j < BS; ++j) xv[u][j] = xp[j];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (k0 + u < w) {
                if (HASK) {
#pragma unroll
                    for (int r = 0; r < BS; ++r)
#pragma unroll
                        for (int j = 0; j < BS; ++j) accK[r] += vv[u][r * BS + j] * xv[u][j].x;
                }
                if (MASS == FEM_MASS_SELL) {
#pragma unroll
                    for (int r = 0; r < BS; ++r) {
                        if (FUSE) accK[r] += mv[u] * xv[u][r].y;
                        else accM[r] += mv[u] * xv[u][r].y;
                    }
                }
            }
    }
}

// b = amp F + M Y[:, 1] + K Y[:, 0]; F may be NULL (no load). MASS_DIAG: the mass term is d o Y[:, 1] of the lane's row.
template <int BS, typename CI, int MASS, int LA, bool HASK>
__global__ void __launch_bounds__(T_BLOCK) k_newmark_rhs(int64_t nslices, int64_t nrows,
                                                         const int64_t* __restrict__ slice_ptr,
                                                         const CI* __restrict__ cols, const double* __restrict__ vals,
                                                         const double* __restrict__ mass, double amp,
                                                         const double* __restrict__ F, const double* __restrict__ Y,
                                                         double* __restrict__ b) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int xcd = blockIdx.x % NXCD;
    const int64_t lb = blockIdx.x / NXCD, nlb = gridDim.x / NXCD;
    const int64_t spx = (nslices + NXCD - 1) / NXCD;
    const int64_t s_begin = (int64_t)xcd * spx;
    const int64_t s_end = s_begin + spx < nslices ? s_begin + spx : nslices;
    for (int64_t s = s_begin + lb * 4 + wave; s < s_end; s += nlb * 4) {
        const int64_t p0 = slice_ptr[s];
        const int w = (HASK || MASS == FEM_MASS_SELL) ? (int)((slice_ptr[s + 1] - p0) >> 6) : 0;
        const int64_t row = s * 64 + lane;
        const bool live = row < nrows;
        double acc[BS], unused[BS];
#pragma unroll
        for (int r = 0; r < BS; ++r) acc[r] = unused[r] = 0.0;
        km_row_walk<BS, CI, MASS, LA, HASK, true>(p0, w, row, live, lane, cols, vals, mass, Y, acc, unused);
        if (live) {
#pragma unroll
            for (int r = 0; r < BS; ++r) {
                const int64_t i = row * BS + r;
                double v = acc[r];
                if (MASS == FEM_MASS_DIAG) v += mass[i] * Y[2 * i + 1];
                if (F) v += amp * F[i];
                b[i] = v;
            }
        }
    }
}

// part[workgroup][2] = the workgroup's sums of x_i (K x)_i and y_i (M y)_i, X = [x | y]: a lane adds its rows in slice
// order, then the wave tree, then the four waves in wave order
template <int BS, typename CI, int MASS, int LA>
__global__ void __launch_bounds__(T_BLOCK) k_quadform_km(int64_t nslices, int64_t nrows,
                                                         const int64_t* __restrict__ slice_ptr,
                                                         const CI* __restrict__ cols, const double* __restrict__ vals,
                                                         const double* __restrict__ mass, const double* __restrict__ X,
                                                         double* __restrict__ part) {
    __shared__ double lds[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int xcd = blockIdx.x % NXCD;
    const int64_t lb = blockIdx.x / NXCD, nlb = gridDim.x / NXCD;
    const int64_t spx = (nslices + NXCD - 1) / NXCD;
    const int64_t s_begin = (int64_t)xcd * spx;
    const int64_t s_end = s_begin + spx < nslices ? s_begin + spx : nslices;
    double qk = 0.0, qm = 0.0;
    for (int64_t s = s_begin + lb * 4 + wave; s < s_end; s += nlb * 4) {
        const int64_t p0 = slice_ptr[s];
        const int w = (int)((slice_ptr[s + 1] - p0) >> 6);
        const int64_t row = s * 64 + lane;
        const bool live = row < nrows;
        double accK[BS], accM[BS];
#pragma unroll
        for (int r = 0; r < BS; ++r) accK[r] = accM[r] = 0.0;
        km_row_walk<BS, CI, MASS, LA, true, false>(p0, w, row, live, lane, cols, vals, mass, X, accK, accM);
        if (live) {
            const double2* xp = reinterpret_cast<const double2*>(X + row * (BS * 2));
#pragma unroll
            for (int r = 0; r < BS; ++r) {
                const double2 x = xp[r];
                qk += x.x * accK[r];
                if (MASS == FEM_MASS_SELL) qm += x.y * accM[r];
                else qm += x.y * (mass[row * BS + r] * x.y);
            }
        }
    }
    qk = wave_sum(qk);
    qm = wave_sum(qm);
    if (lane == 0) {
        lds[2 * wave] = qk;
        lds[2 * wave + 1] = qm;
    }
    __syncthreads();
    if (threadIdx.x < 2)
        part[(int64_t)blockIdx.x * 2 + threadIdx.x] =
            (lds[threadIdx.x] + lds[2 + threadIdx.x]) + (lds[4 + threadIdx.x] + lds[6 + threadIdx.x]);
}

// one workgroup, a wave per value: lane l adds workgroups l, l + 64, ... in order, then the wave tree
__global__ void __launch_bounds__(128) k_quadform_sum(const double* __restrict__ part, int nblocks,
                                                      double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s = 0.0;
    for (int i = lane; i < nblocks; i += 64) s += part[(int64_t)i * 2 + wave];
    s = wave_sum(s);
    if (lane == 0) out[wave] = s;
}

// ---------------------------------------------------------------- the step's vector update
struct NewmarkCoef {
    double a0, a2, a3;      // a_new = a0 (u_new - u) - a2 v - a3 a
    double dt0, dt1;        // v_new = v + dt0 a + dt1 a_new          (dt (1 - gamma), dt gamma)
    double mu, mv, ma;      // yM = mu u_new + mv v_new + ma a_new
    double ku, kv, ka;      // yK = ku u_new + kv v_new + ka a_new    (all 0 without stiffness damping)
    double dt;              // predictor: x = u_new + dt v_new
};

struct NewmarkOut {
    double u, v, a, yk, ym, x;
};

__device__ __forceinline__ NewmarkOut newmark_dof(const NewmarkCoef& c, double un, double uo, double v, double a,
                                                  double w) {
    NewmarkOut o;
    if (w == 0.0) {   // a fixed dof stays at rest
        o.u = o.v = o.a = o.yk = o.ym = o.x = 0.0;
        return o;
    }
    o.a = c.a0 * (un - uo) - c.a2 * v - c.a3 * a;
    o.v = v + c.dt0 * a + c.dt1 * o.a;
    o.u = un;
    o.ym = c.mu * un + c.mv * o.v + c.ma * o.a;
    o.yk = c.ku * un + c.kv * o.v + c.ka * o.a;
    o.x = un + c.dt * o.v;
    return o;
}

// thread e owns dofs 2e, 2e + 1 (16-byte accesses; Y [n, 2] takes two); an odd n leaves one dof to the last thread
template <bool PRED>
__global__ void __launch_bounds__(T_BLOCK) k_newmark_update(int64_t n, NewmarkCoef c, double* __restrict__ x,
                                                            double* __restrict__ u, double* __restrict__ v,
                                                            double* __restrict__ a, const double* __restrict__ w,
                                                            double* __restrict__ Y) {
    const int64_t np = n >> 1;
    for (int64_t e = (int64_t)blockIdx.x * T_BLOCK + threadIdx.x; e <= np; e += (int64_t)gridDim.x * T_BLOCK) {
        if (e < np) {
            const double2 xn = reinterpret_cast<const double2*>(x)[e], uo = reinterpret_cast<const double2*>(u)[e];
            const double2 vo = reinterpret_cast<const double2*>(v)[e], ao = reinterpret_cast<const double2*>(a)[e];
            const double2 wv = reinterpret_cast<const double2*>(w)[e];
            const NewmarkOut p = newmark_dof(c, xn.x, uo.x, vo.x, ao.x, wv.x);
            const NewmarkOut q = newmark_dof(c, xn.y, uo.y, vo.y, ao.y, wv.y);
            reinterpret_cast<double2*>(u)[e] = make_double2(p.u, q.u);
            reinterpret_cast<double2*>(v)[e] = make_double2(p.v, q.v);
            reinterpret_cast<double2*>(a)[e] = make_double2(p.a, q.a);
            reinterpret_cast<double2*>(Y)[2 * e] = make_double2(p.yk, p.ym);
            reinterpret_cast<double2*>(Y)[2 * e + 1] = make_double2(q.yk, q.ym);
            // a fixed dof of x is zeroed in either variant: the solve leaves it at its start value
            reinterpret_cast<double2*>(x)[e] = PRED ? make_double2(p.x, q.x) : make_double2(p.u, q.u);
        } else if (n & 1) {
            const int64_t i = n - 1;
            const NewmarkOut p = newmark_dof(c, x[i], u[i], v[i], a[i], w[i]);
            u[i] = p.u;
            v[i] = p.v;
            a[i] = p.a;
            reinterpret_cast<double2*>(Y)[i] = make_double2(p.yk, p.ym);
            x[i] = PRED ? p.x : p.u;
        }
    }
}

}  // namespace fem

using namespace fem;

// ---------------------------------------------------------------- host side
static bool tr_aligned(const void* p) { return p && !((uintptr_t)p & 15); }

static bool tr_matrix_args(const char* fn, int64_t nrows, int bs, int layout_a, int mass_form) {
    if (bs != 1 && bs != 3) {
        set_error("%s: block size %d unsupported (1 or 3)", fn, bs);
        return false;
    }
    if (layout_a != 0 && (layout_a != 1 || bs != 3)) {
        set_error("%s: layout A is the bs = 3 solver layout (layout_a = %d, bs = %d)", fn, layout_a, bs);
        return false;
    }
    if (mass_form != FEM_MASS_SELL && mass_form != FEM_MASS_DIAG) {
        set_error("%s: mass form %d unsupported (FEM_MASS_SELL or FEM_MASS_DIAG)", fn, mass_form);
        return false;
    }
    if (nrows <= 0) {
        set_error("%s: needs rows, got %lld", fn, (long long)nrows);
        return false;
    }
    return true;
}

static int tr_grid_sweep(int64_t nrows) { return grid_multiple_of_xcd(cdiv(cdiv(nrows, 64), 4), T_GRID_SWEEP); }

template <int BS, int MASS, int LA, bool HASK>
static void tr_rhs_ci(int grid, hipStream_t st, int64_t nslices, int64_t nrows, const int64_t* slice_ptr,
                      const int32_t* cols, const int16_t* dcols, const double* vals, const double* mass, double amp,
                      const double* F, const double* Y, double* b) {
    if (dcols)
        hipLaunchKernelGGL((k_newmark_rhs<BS, int16_t, MASS, LA, HASK>), dim3(grid), dim3(T_BLOCK), 0, st, nslices,
                           nrows, slice_ptr, dcols, vals, mass, amp, F, Y, b);
    else
        hipLaunchKernelGGL((k_newmark_rhs<BS, int32_t, MASS, LA, HASK>), dim3(grid), dim3(T_BLOCK), 0, st, nslices,
                           nrows, slice_ptr, cols, vals, mass, amp, F, Y, b);
}

template <int BS, int MASS, int LA>
static void tr_qf_ci(int grid, hipStream_t st, int64_t nslices, int64_t nrows, const int64_t* slice_ptr,
                     const int32_t* cols, const int16_t* dcols, const double* vals, const double* mass,
                     const double* X, double* part) {
    if (dcols)
        hipLaunchKernelGGL((k_quadform_km<BS, int16_t, MASS, LA>), dim3(grid), dim3(T_BLOCK), 0, st, nslices, nrows,
                           slice_ptr, dcols, vals, mass, X, part);
    else
        hipLaunchKernelGGL((k_quadform_km<BS, int32_t, MASS, LA>), dim3(grid), dim3(T_BLOCK), 0, st, nslices, nrows,
                           slice_ptr, cols, vals, mass, X, part);
}

extern "C" {


int fem_sell_axpby_mass(int64_t nrows, int bs, int layout_a, int64_t entries, const int64_t* slice_ptr,
                        const int32_t* rowptr, const int32_t* diagpos, const double* kvals, const double* mass,
                        int mass_form, double cK, double cM, double* out, fem_stream_t stream) {
    if (!tr_matrix_args("fem_sell_axpby_mass", nrows, bs, layout_a, mass_form)) return FEM_EARG;
    if (entries < 0 || (entries & 63) || !tr_aligned(kvals) || !tr_aligned(out) || !mass ||
        (mass_form == FEM_MASS_DIAG && (!slice_ptr || !rowptr || !diagpos))) {
        set_error("fem_sell_axpby_mass: needs a SELL-64 entry count (a multiple of 64), 16-byte aligned value arrays, "
                  "the mass and, for the diagonal mass, slice_ptr / rowptr / diagpos");
        return FEM_EARG;
    }
    const int64_t npairs = entries * bs * bs / 2;
    if (npairs == 0) return FEM_OK;
    hipStream_t st = S(stream);
    const int grid = stream_grid(npairs, T_BLOCK);
    const dbl2* K2 = reinterpret_cast<const dbl2*>(kvals);
    dbl2* O2 = reinterpret_cast<dbl2*>(out);
#define TR_AX(B, A, M) \
    hipLaunchKernelGGL((k_axpby_mass<B, A, M>), dim3(grid), dim3(T_BLOCK), 0, st, npairs, K2, mass, cK, cM, O2)
    if (mass_form == FEM_MASS_SELL) {
        if (bs == 1) TR_AX(1, 0, FEM_MASS_SELL);
        else if (layout_a) TR_AX(3, 1, FEM_MASS_SELL);
        else TR_AX(3, 0, FEM_MASS_SELL);
    } else {
        if (bs == 1) TR_AX(1, 0, FEM_MASS_DIAG);
        else TR_AX(3, 0, FEM_MASS_DIAG);   // K alone is scaled: the layout does not matter
    }
#undef TR_AX
    FEM_LAUNCHED();
    if (mass_form == FEM_MASS_DIAG) {
        const int g2 = stream_grid(nrows * bs, T_BLOCK);
#define TR_DG(B, A) \
    hipLaunchKernelGGL((k_axpby_diag<B, A>), dim3(g2), dim3(T_BLOCK), 0, st, nrows, slice_ptr, rowptr, diagpos, kvals, \
                       mass, cK, cM, out)
        if (bs == 1) TR_DG(1, 0);
        else if (layout_a) TR_DG(3, 1);
        else TR_DG(3, 0);
#undef TR_DG
        FEM_LAUNCHED();
    }
    return FEM_OK;
}

int fem_newmark_rhs(int64_t nrows, int bs, int layout_a, const int64_t* slice_ptr, const int32_t* cols,
                    const int16_t* dcols, const double* kvals, const double* mass, int mass_form, double amp,
                    const double* F, const double* Y, double* b, fem_stream_t stream) {
    if (!tr_matrix_args("fem_newmark_rhs", nrows, bs, layout_a, mass_form)) return FEM_EARG;
    if (!slice_ptr || (!cols && !dcols) || !mass || !tr_aligned(Y) || !b || (layout_a && !dcols)) {
        set_error("fem_newmark_rhs: needs the pattern, a column array (16-bit deltas for layout A), the mass, the "
                  "16-byte aligned Y and b");
        return FEM_EARG;
    }
    const int64_t nslices = cdiv(nrows, 64);
    const int grid = tr_grid_sweep(nrows);
    hipStream_t st = S(stream);
#define TR_RHS(B, M, A, K) \
    tr_rhs_ci<B, M, A, K>(grid, st, nslices, nrows, slice_ptr, cols, dcols, kvals, mass, amp, F, Y, b)
#define TR_RHS_M(B, A, K)                           \
    do {                                            \
        if (mass_form == FEM_MASS_SELL) TR_RHS(B, FEM_MASS_SELL, A, K); \
        else TR_RHS(B, FEM_MASS_DIAG, A, K);        \
    } while (0)
    if (!kvals) {   // no stiffness damping: the K stream is not read
        if (bs == 1) TR_RHS_M(1, 0, false);
        else TR_RHS_M(3, 0, false);
    } else if (bs == 1) TR_RHS_M(1, 0, true);
    else if (layout_a) TR_RHS_M(3, 1, true);
    else TR_RHS_M(3, 0, true);
#undef TR_RHS_M
#undef TR_RHS
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_newmark_update(int64_t n, const double* coef, int predictor, double* x, double* u, double* v, double* a,
                       const double* w, double* Y, fem_stream_t stream) {
    if (n <= 0 || !coef || !tr_aligned(x) || !tr_aligned(u) || !tr_aligned(v) || !tr_aligned(a) || !tr_aligned(w) ||
        !tr_aligned(Y)) {
        set_error("fem_newmark_update: needs dofs, the 12 coefficients and 16-byte aligned x, u, v, a, w and Y");
        return FEM_EARG;
    }
    NewmarkCoef c;
    c.a0 = coef[0], c.a2 = coef[1], c.a3 = coef[2], c.dt0 = coef[3], c.dt1 = coef[4];
    c.mu = coef[5], c.mv = coef[6], c.ma = coef[7], c.ku = coef[8], c.kv = coef[9], c.ka = coef[10], c.dt = coef[11];
    const int grid = grid_multiple_of_xcd(cdiv(n / 2 + 1, T_BLOCK), T_GRID_VEC);
    if (predictor)
        hipLaunchKernelGGL(k_newmark_update<true>, dim3(grid), dim3(T_BLOCK), 0, S(stream), n, c, x, u, v, a, w, Y);
    else
        hipLaunchKernelGGL(k_newmark_update<false>, dim3(grid), dim3(T_BLOCK), 0, S(stream), n, c, x, u, v, a, w, Y);
    FEM_LAUNCHED();
    return FEM_OK;
}

int64_t fem_transient_work_len(void) { return 2 * (int64_t)T_GRID_SWEEP; }

int fem_quadform_km(int64_t nrows, int bs, int layout_a, const int64_t* slice_ptr, const int32_t* cols,
                    const int16_t* dcols, const double* kvals, const double* mass, int mass_form, const double* X,
                    double* work, double* out, fem_stream_t stream) {
    if (!tr_matrix_args("fem_quadform_km", nrows, bs, layout_a, mass_form)) return FEM_EARG;
    if (!slice_ptr || (!cols && !dcols) || !kvals || !mass || !tr_aligned(X) || !work || !out ||
        (layout_a && !dcols)) {
        set_error("fem_quadform_km: needs the pattern, a column array (16-bit deltas for layout A), both value arrays, "
                  "the 16-byte aligned X, the workspace and the output");
        return FEM_EARG;
    }
    const int64_t nslices = cdiv(nrows, 64);
    const int grid = tr_grid_sweep(nrows);
    hipStream_t st = S(stream);
#define TR_QF(B, A)                                                                                              \
    do {                                                                                                         \
        if (mass_form == FEM_MASS_SELL)                                                                          \
            tr_qf_ci<B, FEM_MASS_SELL, A>(grid, st, nslices, nrows, slice_ptr, cols, dcols, kvals, mass, X, work); \
        else                                                                                                     \
            tr_qf_ci<B, FEM_MASS_DIAG, A>(grid, st, nslices, nrows, slice_ptr, cols, dcols, kvals, mass, X, work); \
    } while (0)
    if (bs == 1) TR_QF(1, 0);
    else if (layout_a) TR_QF(3, 1);
    else TR_QF(3, 0);
#undef TR_QF
    FEM_LAUNCHED();
    hipLaunchKernelGGL(k_quadform_sum, dim3(1), dim3(128), 0, st, (const double*)work, grid, out);
    FEM_LAUNCHED();
    return FEM_OK;
}

}  // extern "C"
