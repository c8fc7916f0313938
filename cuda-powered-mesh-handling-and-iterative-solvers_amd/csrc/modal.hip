// Modal analysis: the tall-skinny kernels of the block LOBPCG for K u = lambda M u (system.py SellMatrix.eig_lowest;
// the reference's `vectorized_modal_solver`, `solver/solver.py:1084-1313`, promises the lowest eigenpairs).
//
// Multi-vectors are [n, NV] row-major as in pcg_multi.hip (n = nrows * bs, NV in {2, 4, 8}, 16-byte aligned). The
// solver carries nine of them -- X, W, P and their products with K and M -- and per iteration runs
//   k_modal_residual (+ k_modal_norms) : R = KX - MX diag(theta), W = w o R, ||R_j|| and ||MX_j|| over the free rows
//   k_spmm_km                          : KW = K W and MW = M W in ONE sweep of the SELL-64 pattern
//   k_modal_gram (+ k_modal_gram_sum)  : G_K = S^T (K S), G_M = S^T (M S), S = [X W P], one read of the nine
//   k_modal_rotate                     : X <- S C, P <- [W P] C_WP and the same for the K- and M-products, in place
// Plain launches only; no workgroup waits on another; no floating-point atomics. Every reduction is written as
// per-workgroup partials and summed in workgroup order by the following one-workgroup launch, so results are
// bit-reproducible. Grid sizes depend on (n, NV, a) only; rows >= n are never read nor stored.
#include "common.hpp"

namespace fem {

constexpr int E_BLOCK = 256;
constexpr int E_GRID_SPMM = 2048;   // as pcg_multi.hip's SpMM
constexpr int E_GRID_VEC = 1024;    // cap of the grids that write partials
constexpr int E_GRID_GRAM = 1024;
constexpr int E_SUM_BLOCK = 1024;   // threads of the one-workgroup Gram finish
constexpr int E_TILE = 32;          // rows of the nine multi-vectors staged per Gram tile
constexpr int E_MAXAM = 24;         // widest basis: 3 blocks of 8 columns
constexpr int E_MAXNB = (E_MAXAM / 2) * (E_MAXAM / 2 + 1) / 2;   // 2 x 2 blocks of the upper triangle: 78
constexpr int E_TILE_LD = 3 * E_MAXAM + 2;                       // LDS row: [S | KS | MS] + one 16-byte pad

// ---------------------------------------------------------------- K/M product
// k_mpcg_spmm's row walk (one wave per slice, one lane per block row, sell_row's (k, r, j) summation order) with a
// second set of accumulators: every gathered block column of X is loaded once and used for both products.
// MASS_SELL: `mass` holds the plain bs = 1 SELL values of a matrix on the SAME pattern; the mass is M_s (x) I_bs, so
//   component r of block row i gets sum_k ms[i, k] x[col_k, r] -- for BS = 1 exactly fem_spmm of the mass matrix.
// MASS_DIAG: `mass` is a vector d [n]; Z = d o X for the rows the lane owns.
template <int BS, int NV, typename CI, int MASS>
__global__ void __launch_bounds__(E_BLOCK) k_spmm_km(int64_t nslices, int64_t nrows,
                                                     const int64_t* __restrict__ slice_ptr,
                                                     const CI* __restrict__ cols, const double* __restrict__ vals,
                                                     const double* __restrict__ mass, const double* __restrict__ X,
                                                     double* __restrict__ Y, double* __restrict__ Z) {
    constexpr int U = BS == 1 ? 4 : 1;          // entries in flight per lane
    constexpr int H = NV / 2;
    constexpr int NP = BS * H;                  // 16-byte pieces of one gathered block column
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
        const double* mp = MASS == FEM_MASS_SELL ? mass + p0 + lane : mass;   // the entry's scalar mass value
        double acc[BS][NV], accm[BS][NV];
#pragma unroll
        for (int r = 0; r < BS; ++r)
#pragma unroll
            for (int j = 0; j < NV; ++j) acc[r][j] = accm[r][j] = 0.0;
        for (int k0 = 0; k0 < w; k0 += U) {
            int64_t cc[U];
            double vv[U][BS * BS], mv[U];
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
                mv[u] = 0.0;
                if (MASS == FEM_MASS_SELL && k0 + u < w) mv[u] = __builtin_nontemporal_load(mp + (int64_t)64 * (k0 + u));
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
                            for (int e = 0; e < H; ++e) {
                                acc[r][2 * e] += vv[u][r * BS + j] * xv[u][j * H + e].x;
                                acc[r][2 * e + 1] += vv[u][r * BS + j] * xv[u][j * H + e].y;
                            }
                    if (MASS == FEM_MASS_SELL) {
#pragma unroll
                        for (int r = 0; r < BS; ++r)
#pragma unroll
                            for (int e = 0; e < H; ++e) {
                                accm[r][2 * e] += mv[u] * xv[u][r * H + e].x;
                                accm[r][2 * e + 1] += mv[u] * xv[u][r * H + e].y;
                            }
                    }
                }
        }
        if (live) {
            double2* yp = reinterpret_cast<double2*>(Y + row * (BS * NV));
            double2* zp = reinterpret_cast<double2*>(Z + row * (BS * NV));
#pragma unroll
            for (int r = 0; r < BS; ++r)
#pragma unroll
                for (int e = 0; e < H; ++e) yp[r * H + e] = make_double2(acc[r][2 * e], acc[r][2 * e + 1]);
            if (MASS == FEM_MASS_SELL) {
#pragma unroll
                for (int r = 0; r < BS; ++r)
#pragma unroll
                    for (int e = 0; e < H; ++e) zp[r * H + e] = make_double2(accm[r][2 * e], accm[r][2 * e + 1]);
            } else {
                const double2* xp = reinterpret_cast<const double2*>(X + row * (BS * NV));
#pragma unroll
                for (int r = 0; r < BS; ++r) {
                    const double d = mass[row * BS + r];
#pragma unroll
                    for (int e = 0; e < H; ++e) {
                        const double2 x = xp[r * H + e];
                        zp[r * H + e] = make_double2(d * x.x, d * x.y);
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------- Gram matrices
// The basis S = [X W P] has am = a * m columns (a = 1: X alone, the first Rayleigh-Ritz; 2: no P; 3). A workgroup
// stages E_TILE rows of the 3 a multi-vectors in LDS as rows [S | KS | MS] (stride 3 am + 2 doubles: the 16-byte pad
// keeps rows of different row groups off each other's banks). The upper triangle is cut into 2 x 2 blocks (bi <= bj);
// a thread owns one block of BOTH matrices and one row group: per staged row it reads S[2bi..], KS[2bj..], MS[2bj..]
// (three 16-byte LDS reads, lanes of equal block read the same address) for 8 FMAs, rows of its group in row order,
// tiles in tile order. The row groups are then added in group order and written as the workgroup's partial.
struct ModalVecs {
    double* v[9];   // X, W, P, KX, KW, KP, MX, MW, MP
};

__global__ void __launch_bounds__(E_BLOCK) k_modal_gram(int64_t n, int m, int a, ModalVecs p,
                                                        double* __restrict__ part) {
    __shared__ double2 tile2[E_TILE * E_TILE_LD / 2];   // >= E_BLOCK * 8 doubles for the row-group sums
    double* tile = reinterpret_cast<double*>(tile2);
    const int am = a * m, h = am / 2, nb = h * (h + 1) / 2, ld = 3 * am + 2;
    int rgs = E_BLOCK / nb;
    if (rgs > E_TILE) rgs = E_TILE;
    const int blk = threadIdx.x % nb, rg = threadIdx.x / nb;
    const bool active = rg < rgs;
    int bi = 0, rem = blk;
    while (rem >= h - bi) {
        rem -= h - bi;
        ++bi;
    }
    const int bj = bi + rem;
    const int hm = m / 2;                    // 16-byte pieces per row of one multi-vector
    const int per = E_TILE * hm;             // pieces of one multi-vector per tile
    const int64_t ntiles = (n + E_TILE - 1) / E_TILE;
    double g[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = 0.0;
    // the tile's 3 a multi-vector pieces go through registers: the next tile's loads are issued before this tile's
    // sums, so their latency hides behind the LDS work (at most E_STAGE 16-byte pieces per thread: 3 * 3 * 32 * 4 / 256)
    constexpr int E_STAGE = (3 * 3 * E_TILE * 4 + E_BLOCK - 1) / E_BLOCK;
    const int cnt = 3 * a * per;
    double2 stage[E_STAGE];
    const double2* src[E_STAGE];   // piece q of this thread: its source at tile 0, its tile row, its LDS slot
    int srow[E_STAGE], slot[E_STAGE];
#pragma unroll
    for (int q = 0; q < E_STAGE; ++q) {
        const int idx = threadIdx.x + q * E_BLOCK;
        const int v = idx < cnt ? idx / per : 0, rm = idx < cnt ? idx % per : 0;
        src[q] = reinterpret_cast<const double2*>(p.v[(v / a) * 3 + v % a]) + rm;
        srow[q] = idx < cnt ? rm / hm : -1;
        slot[q] = ((rm / hm) * ld + (v / a) * am + (v % a) * m) / 2 + rm % hm;
    }
    auto fetch = [&](int64_t r0) {
#pragma unroll
        for (int q = 0; q < E_STAGE; ++q) {
            stage[q] = make_double2(0.0, 0.0);
            if (srow[q] >= 0 && r0 + srow[q] < n) stage[q] = src[q][r0 * hm];
        }
    };
    if ((int64_t)blockIdx.x < ntiles) fetch((int64_t)blockIdx.x * E_TILE);
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        __syncthreads();   // the previous tile's sums are done
#pragma unroll
        for (int q = 0; q < E_STAGE; ++q)
            if (srow[q] >= 0) tile2[slot[q]] = stage[q];
        __syncthreads();
        if (t + gridDim.x < ntiles) fetch((t + gridDim.x) * E_TILE);
        if (active) {
            for (int r = rg; r < E_TILE; r += rgs) {
                const double2 s = tile2[(r * ld) / 2 + bi];
                const double2 k = tile2[(r * ld + am) / 2 + bj];
                const double2 mm = tile2[(r * ld + 2 * am) / 2 + bj];
                g[0] += s.x * k.x;
                g[1] += s.x * k.y;
                g[2] += s.y * k.x;
                g[3] += s.y * k.y;
                g[4] += s.x * mm.x;
                g[5] += s.x * mm.y;
                g[6] += s.y * mm.x;
                g[7] += s.y * mm.y;
            }
        }
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int e = 0; e < 8; ++e) tile[(rg * nb + blk) * 8 + e] = g[e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb * 8; i += E_BLOCK) {
        double sum = 0.0;
        for (int r = 0; r < rgs; ++r) sum += tile[r * nb * 8 + i];
        part[(int64_t)blockIdx.x * (nb * 8) + i] = sum;
    }
}

// one workgroup of E_SUM_BLOCK threads, one Gram entry each: the partials added in workgroup order, the upper
// triangle stored and mirrored. out: G_K [am, am]
// row-major at 0, G_M at FEM_MODAL_OUT_GM
__global__ void __launch_bounds__(E_SUM_BLOCK) k_modal_gram_sum(const double* __restrict__ part, int nblocks, int am,
                                                                double* __restrict__ out) {
    const int h = am / 2, nb = h * (h + 1) / 2;
    for (int i = threadIdx.x; i < nb * 8; i += E_SUM_BLOCK) {
        double sum = 0.0;
        for (int b0 = 0; b0 < nblocks; b0 += 16) {   // sixteen loads in flight, added in workgroup order
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = b0 + u < nblocks ? part[(int64_t)(b0 + u) * (nb * 8) + i] : 0.0;
#pragma unroll
            for (int u = 0; u < 16; ++u) sum += v[u];
        }
        const int blk = i >> 3, e = i & 7;
        int bi = 0, rem = blk;
        while (rem >= h - bi) {
            rem -= h - bi;
            ++bi;
        }
        const int bj = bi + rem;
        const int r = 2 * bi + ((e >> 1) & 1), c = 2 * bj + (e & 1);
        if (r > c) continue;   // the lower entry of a diagonal block: its mirror image is stored
        double* G = out + (e >> 2) * FEM_MODAL_OUT_GM;
        G[r * am + c] = sum;
        G[c * am + r] = sum;
    }
}

// ---------------------------------------------------------------- residual
// Flat walk in 16-byte column pairs as pcg_multi.hip's vector kernels: thread e handles pair e % (NV / 2) of dof
// e / (NV / 2), so its two thetas sit in registers. part[block][2 NV]: sums of R_j^2, then of MX_j^2, free rows only.
template <int NV>
__global__ void __launch_bounds__(E_BLOCK) k_modal_residual(int64_t n, const double2* __restrict__ KX,
                                                            const double2* __restrict__ MX,
                                                            const double* __restrict__ w,
                                                            const double* __restrict__ theta,
                                                            double2* __restrict__ W, double* __restrict__ part) {
    constexpr int H = NV / 2;
    __shared__ double lds[4 * 2 * NV];
    const int c0 = 2 * (threadIdx.x % H);
    const double th0 = theta[c0], th1 = theta[c0 + 1];
    const int64_t total = n * H;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t e = (int64_t)blockIdx.x * E_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * E_BLOCK) {
        const double wv = w[e / H];
        const double2 kx = KX[e], mx = MX[e];
        const double2 r = make_double2(kx.x - th0 * mx.x, kx.y - th1 * mx.y);
        W[e] = make_double2(wv * r.x, wv * r.y);
        if (wv != 0.0) {
            a[0] += r.x * r.x;
            a[1] += r.y * r.y;
            a[2] += mx.x * mx.x;
            a[3] += mx.y * mx.y;
        }
    }
#pragma unroll
    for (int o = 32; o >= H; o >>= 1)
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] += __shfl_xor(a[q], o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < H) {
        lds[wave * 2 * NV + 2 * lane] = a[0];
        lds[wave * 2 * NV + 2 * lane + 1] = a[1];
        lds[wave * 2 * NV + NV + 2 * lane] = a[2];
        lds[wave * 2 * NV + NV + 2 * lane + 1] = a[3];
    }
    __syncthreads();
    if (threadIdx.x < 2 * NV) {
        const int t = threadIdx.x;
        part[(int64_t)blockIdx.x * (2 * NV) + t] =
            (lds[t] + lds[2 * NV + t]) + (lds[4 * NV + t] + lds[6 * NV + t]);
    }
}

// one workgroup, a wave per value: lane l adds blocks l, l + 64, ... in order, then the wave tree; the square roots
// go to out[FEM_MODAL_OUT_NORMS + ...]: ||R_j|| [nv], then ||MX_j|| [nv]
__global__ void __launch_bounds__(E_BLOCK) k_modal_norms(const double* __restrict__ part, int nblocks, int nv,
                                                         double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int v = wave; v < 2 * nv; v += 4) {
        double s = 0.0;
        for (int i = lane; i < nblocks; i += 64) s += part[(int64_t)i * (2 * nv) + v];
        s = wave_sum(s);
        if (lane == 0) out[FEM_MODAL_OUT_NORMS + v] = sqrt(s);
    }
}

// ---------------------------------------------------------------- rotation
// Flat walk in 16-byte column pairs, one family per blockIdx.y (the vectors, their K-products, their M-products):
// thread e owns output pair e % (NV / 2) of row e / (NV / 2) in every step of its grid-stride loop, so the 3 NV x 2
// coefficients of its two columns of C [a NV, NV] sit in registers (loaded once). It reads the whole row of X, W and P
// in 16-byte loads and stores
//   P_new = W C_W + P C_P,  X_new = X C_X + P_new
// for its pair, in place (a = 2: no old P; a = 1: X alone, P untouched). W is read only. The NV / 2 threads of one
// row are neighbouring lanes of one wave (block and grid sizes are multiples of NV / 2): a wave issues every load of a
// step before the stores that depend on them, so no lane sees a row half rotated.
template <int NV>
__global__ void __launch_bounds__(E_BLOCK) k_modal_rotate(int64_t n, int a, ModalVecs p,
                                                          const double2* __restrict__ C) {
    constexpr int H = NV / 2;
    const int jp = threadIdx.x % H;
    double2 cx[NV], cw[NV], cp[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        cx[i] = C[i * H + jp];
        cw[i] = a >= 2 ? C[(NV + i) * H + jp] : make_double2(0.0, 0.0);
        cp[i] = a == 3 ? C[(2 * NV + i) * H + jp] : make_double2(0.0, 0.0);
    }
    double2* X = reinterpret_cast<double2*>(p.v[blockIdx.y * 3]);
    const double2* W = reinterpret_cast<const double2*>(p.v[blockIdx.y * 3 + 1]);
    double2* P = reinterpret_cast<double2*>(p.v[blockIdx.y * 3 + 2]);
    const int64_t total = n * H;
    for (int64_t e = (int64_t)blockIdx.x * E_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * E_BLOCK) {
        const int64_t r0 = e - jp;   // first pair of the row
        double2 x[H], wv[H], pv[H];
#pragma unroll
        for (int q = 0; q < H; ++q) {
            x[q] = X[r0 + q];
            wv[q] = a >= 2 ? W[r0 + q] : make_double2(0.0, 0.0);
            pv[q] = a == 3 ? P[r0 + q] : make_double2(0.0, 0.0);
        }
        double2 pn = make_double2(0.0, 0.0), xn = make_double2(0.0, 0.0);
#pragma unroll
        for (int q = 0; q < H; ++q) {
            pn.x += wv[q].x * cw[2 * q].x;
            pn.y += wv[q].x * cw[2 * q].y;
            pn.x += wv[q].y * cw[2 * q + 1].x;
            pn.y += wv[q].y * cw[2 * q + 1].y;
        }
#pragma unroll
        for (int q = 0; q < H; ++q) {
            pn.x += pv[q].x * cp[2 * q].x;
            pn.y += pv[q].x * cp[2 * q].y;
            pn.x += pv[q].y * cp[2 * q + 1].x;
            pn.y += pv[q].y * cp[2 * q + 1].y;
        }
#pragma unroll
        for (int q = 0; q < H; ++q) {
            xn.x += x[q].x * cx[2 * q].x;
            xn.y += x[q].x * cx[2 * q].y;
            xn.x += x[q].y * cx[2 * q + 1].x;
            xn.y += x[q].y * cx[2 * q + 1].y;
        }
        X[e] = make_double2(xn.x + pn.x, xn.y + pn.y);
        if (a >= 2) P[e] = pn;
    }
}

}  // namespace fem

using namespace fem;

// ---------------------------------------------------------------- host side
static bool md_dims_ok(const char* fn, int bs, int nv) {
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

static int md_grid_vec(int64_t items) { return grid_multiple_of_xcd(cdiv(items, E_BLOCK), E_GRID_VEC); }
static int md_grid_gram(int64_t n) {
    const int64_t t = cdiv(n, E_TILE);
    return (int)(t < E_GRID_GRAM ? (t < 1 ? 1 : t) : E_GRID_GRAM);
}

template <int BS, int NV, int MASS>
static void md_spmm_ci(int grid, hipStream_t st, int64_t nslices, int64_t nrows, const int64_t* slice_ptr,
                       const int32_t* cols, const int16_t* dcols, const double* vals, const double* mass,
                       const double* X, double* Y, double* Z) {
    if (dcols)
        hipLaunchKernelGGL((k_spmm_km<BS, NV, int16_t, MASS>), dim3(grid), dim3(E_BLOCK), 0, st, nslices, nrows,
                           slice_ptr, dcols, vals, mass, X, Y, Z);
    else
        hipLaunchKernelGGL((k_spmm_km<BS, NV, int32_t, MASS>), dim3(grid), dim3(E_BLOCK), 0, st, nslices, nrows,
                           slice_ptr, cols, vals, mass, X, Y, Z);
}

static bool md_aligned(const void* const* v, int count) {
    for (int i = 0; i < count; ++i)
        if (!v[i] || ((uintptr_t)v[i] & 15)) return false;
    return true;
}

extern "C" {

int fem_spmm_km(int64_t nrows, int bs, int nv, const int64_t* slice_ptr, const int32_t* cols, const int16_t* dcols,
                const double* vals, const double* mass, int mass_form, const double* X, double* Y, double* Z,
                fem_stream_t stream) {
    if (!md_dims_ok("fem_spmm_km", bs, nv)) return FEM_EARG;
    if (mass_form != FEM_MASS_SELL && mass_form != FEM_MASS_DIAG) {
        set_error("fem_spmm_km: mass form %d unsupported (FEM_MASS_SELL or FEM_MASS_DIAG)", mass_form);
        return FEM_EARG;
    }
    const void* mv[3] = {X, Y, Z};
    if (nrows <= 0 || (!cols && !dcols) || !vals || !mass || !md_aligned(mv, 3)) {
        set_error("fem_spmm_km: needs rows, a column array, both value arrays and 16-byte aligned multi-vectors");
        return FEM_EARG;
    }
    const int64_t nslices = cdiv(nrows, 64);
    const int grid = grid_multiple_of_xcd(cdiv(nslices, 4), E_GRID_SPMM);
    hipStream_t st = S(stream);
#define MD_CASE(B, V)                                                                                             \
    if (bs == B && nv == V) {                                                                                     \
        if (mass_form == FEM_MASS_SELL)                                                                           \
            md_spmm_ci<B, V, FEM_MASS_SELL>(grid, st, nslices, nrows, slice_ptr, cols, dcols, vals, mass, X, Y, Z); \
        else                                                                                                      \
            md_spmm_ci<B, V, FEM_MASS_DIAG>(grid, st, nslices, nrows, slice_ptr, cols, dcols, vals, mass, X, Y, Z); \
    }
    MD_CASE(1, 2) MD_CASE(1, 4) MD_CASE(1, 8) MD_CASE(3, 2) MD_CASE(3, 4) MD_CASE(3, 8)
#undef MD_CASE
    FEM_LAUNCHED();
    return FEM_OK;
}

int64_t fem_modal_work_len(void) { return (int64_t)E_GRID_GRAM * E_MAXNB * 8 + (int64_t)E_GRID_VEC * 16; }

static bool md_vec_args(const char* fn, int64_t n, int nv, int a, int amin) {
    if (nv != 2 && nv != 4 && nv != 8) {
        set_error("%s: %d columns unsupported (2, 4 or 8)", fn, nv);
        return false;
    }
    if (n <= 0 || a < amin || a > 3) {
        set_error("%s: needs rows and %d to 3 basis blocks, got n = %lld, a = %d", fn, amin, (long long)n, a);
        return false;
    }
    return true;
}

int fem_modal_gram(int64_t n, int nv, int a, const double* const* vecs, double* work, double* out,
                   fem_stream_t stream) {
    if (!md_vec_args("fem_modal_gram", n, nv, a, 1)) return FEM_EARG;
    ModalVecs p{};
    for (int f = 0; f < 3; ++f)
        for (int b = 0; b < a; ++b) {
            const double* q = vecs ? vecs[f * 3 + b] : nullptr;
            if (!q || ((uintptr_t)q & 15)) {
                set_error("fem_modal_gram: multi-vector %d is NULL or not 16-byte aligned", f * 3 + b);
                return FEM_EARG;
            }
            p.v[f * 3 + b] = const_cast<double*>(q);
        }
    if (!work || !out) {
        set_error("fem_modal_gram: needs the workspace and the output buffer");
        return FEM_EARG;
    }
    const int grid = md_grid_gram(n);
    hipLaunchKernelGGL(k_modal_gram, dim3(grid), dim3(E_BLOCK), 0, S(stream), n, nv, a, p, work);
    hipLaunchKernelGGL(k_modal_gram_sum, dim3(1), dim3(E_SUM_BLOCK), 0, S(stream), (const double*)work, grid, a * nv, out);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_modal_residual(int64_t n, int nv, const double* KX, const double* MX, const double* w, const double* theta,
                       double* W, double* work, double* out, fem_stream_t stream) {
    if (!md_vec_args("fem_modal_residual", n, nv, 1, 1)) return FEM_EARG;
    const void* mv[3] = {KX, MX, W};
    if (!md_aligned(mv, 3) || !w || !theta || !work || !out) {
        set_error("fem_modal_residual: needs 16-byte aligned multi-vectors, w, theta, the workspace and the output");
        return FEM_EARG;
    }
    double* part = work + (int64_t)E_GRID_GRAM * E_MAXNB * 8;
    const int grid = md_grid_vec(n * (nv / 2));
    hipStream_t st = S(stream);
#define MD_RES(V)                                                                                                  \
    hipLaunchKernelGGL(k_modal_residual<V>, dim3(grid), dim3(E_BLOCK), 0, st, n, (const double2*)KX,               \
                       (const double2*)MX, w, theta, (double2*)W, part)
    if (nv == 2) MD_RES(2);
    else if (nv == 4) MD_RES(4);
    else MD_RES(8);
#undef MD_RES
    hipLaunchKernelGGL(k_modal_norms, dim3(1), dim3(E_BLOCK), 0, st, (const double*)part, grid, nv, out);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_modal_rotate(int64_t n, int nv, int a, double* const* vecs, const double* C, fem_stream_t stream) {
    if (!md_vec_args("fem_modal_rotate", n, nv, a, 1)) return FEM_EARG;
    ModalVecs p{};
    for (int f = 0; f < 3; ++f)
        for (int b = 0; b < 3; ++b) {
            double* q = vecs ? vecs[f * 3 + b] : nullptr;
            // a = 1 touches X alone; a = 2 reads W and writes P
            const bool used = b == 0 || a >= 2;
            if (used && (!q || ((uintptr_t)q & 15))) {
                set_error("fem_modal_rotate: multi-vector %d is NULL or not 16-byte aligned", f * 3 + b);
                return FEM_EARG;
            }
            p.v[f * 3 + b] = q;
        }
    if (!C || ((uintptr_t)C & 15)) {
        set_error("fem_modal_rotate: needs the 16-byte aligned coefficient matrix");
        return FEM_EARG;
    }
    const dim3 grid(md_grid_vec(n * (nv / 2)), 3);
    hipStream_t st = S(stream);
    const double2* C2 = reinterpret_cast<const double2*>(C);
    if (nv == 2) hipLaunchKernelGGL(k_modal_rotate<2>, grid, dim3(E_BLOCK), 0, st, n, a, p, C2);
    else if (nv == 4) hipLaunchKernelGGL(k_modal_rotate<4>, grid, dim3(E_BLOCK), 0, st, n, a, p, C2);
    else hipLaunchKernelGGL(k_modal_rotate<8>, grid, dim3(E_BLOCK), 0, st, n, a, p, C2);
    FEM_LAUNCHED();
    return FEM_OK;
}

}  // extern "C"
