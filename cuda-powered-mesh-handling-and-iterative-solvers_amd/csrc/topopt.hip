// Density-based topology optimisation of c3d4 elasticity on gfx950: the design loop's kernels around the
// scaled assembly (fem_assemble_tet4_scaled*) and the PCG solve -- unit strain energy and compliance, the node-average
// density filter and its adjoint, the SIMP modulus scale, and the optimality-criteria update with its bisection on
// the device. All fp64. No atomics except the atomicMin of a degenerate element's index; every sum runs in a fixed
// order (incidence order per node, a fixed tree per block, the block partials by one block in block order), so two
// runs give the same bits.
#include <math.h>

#include "common.hpp"
#include "element.hpp"

namespace fem {

constexpr int TO_GRID = 1024;   // workgroups of the grid-stride reduction kernels (partials per quantity)
// the OC state in the workspace (doubles): the bracket, the volume target and what the finish kernels leave
constexpr int TO_LO = 0, TO_HI = 1, TO_TARGET = 2, TO_VTOT = 3, TO_ACTIVE = 4, TO_STATE = 8;

__host__ __device__ inline int64_t to_blocks(int64_t M) {
    const int64_t g = (M + 255) / 256;
    return g < 1 ? 1 : (g > TO_GRID ? TO_GRID : g);
}

// n partials by one 256-thread block: thread t takes t, t + 256, ... in ascending order, then the fixed tree
__device__ __forceinline__ double to_sum(const double* __restrict__ p, int64_t n, double* lds4) {
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) v += p[i];
    return block_sum256(v, lds4);
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_maxd(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
// min / max over a 256-thread block, valid in every thread (MAX: the maximum)
template <bool MAX>
__device__ __forceinline__ double block_ext256(double v, double* lds4) {
    v = MAX ? wave_maxd(v) : wave_min(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return MAX ? fmax(fmax(lds4[0], lds4[1]), fmax(lds4[2], lds4[3]))
               : fmin(fmin(lds4[0], lds4[1]), fmin(lds4[2], lds4[3]));
}

__device__ __forceinline__ double simp_scale(double rho_t, double penal, double s_min) {
    return s_min + (1.0 - s_min) * pow(rho_t, penal);
}

// ---------------------------------------------------------------- volumes
__global__ void __launch_bounds__(256) k_tet4_vol(const double* __restrict__ X, const int64_t* __restrict__ conn,
                                                  int64_t M, double* __restrict__ V, int64_t* __restrict__ bad) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < M; e += (int64_t)gridDim.x * blockDim.x) {
        // only |det| enters: from the nodes in ascending global id, the same bits for any local order of the element
        const double det = tet4_det_sorted(X, conn + 4 * e);
        if (bad && !(fabs(det) >= 1e-12)) atomicMin((unsigned long long*)bad, (unsigned long long)e);
        V[e] = fabs(det) / 6.0;
    }
}

// MODE 0: Vn[n] = sum V_e;  1 (forward): out[n] = (sum V_e x_e) / Vn[n];  2 (adjoint): out[n] = (1/4 sum x_e) / Vn[n]
// -- over the node's incidences in ascending order; a node without elements gets 0
template <int MODE>
__global__ void __launch_bounds__(256) k_to_node(const int32_t* __restrict__ inc_ptr, const int32_t* __restrict__ inc,
                                                 int64_t N, const double* __restrict__ V,
                                                 const double* __restrict__ Vn, const double* __restrict__ x,
                                                 double* __restrict__ out) {
#pragma clang fp contract(off)
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        double acc = 0.0;
        for (int t = inc_ptr[n]; t < inc_ptr[n + 1]; ++t) {
            const int64_t e = inc[t] >> 2;
            acc += MODE == 0 ? V[e] : (MODE == 1 ? V[e] * x[e] : x[e]);
        }
        if (MODE == 0) {
            out[n] = acc;
        } else {
            const double vn = Vn[n];
            if (MODE == 2) acc *= 0.25;
            out[n] = vn > 0.0 ? acc / vn : 0.0;
        }
    }
}

// forward: out[e] = 1/4 sum_a y[e_a] (SCALE: also s[e] = s_min + (1 - s_min) out[e]^p);  adjoint: out[e] = V_e sum_a y[e_a]
template <bool ADJ, bool SCALE>
__global__ void __launch_bounds__(256) k_to_elem(const int64_t* __restrict__ conn, int64_t M,
                                                 const double* __restrict__ V, const double* __restrict__ y,
                                                 double penal, double s_min, double* __restrict__ out,
                                                 double* __restrict__ s) {
#pragma clang fp contract(off)
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < M; e += (int64_t)gridDim.x * blockDim.x) {
        const double sum = ((y[conn[4 * e]] + y[conn[4 * e + 1]]) + y[conn[4 * e + 2]]) + y[conn[4 * e + 3]];
        const double v = ADJ ? V[e] * sum : 0.25 * sum;
        out[e] = v;
        if (SCALE) s[e] = simp_scale(v, penal, s_min);
    }
}

__global__ void __launch_bounds__(256) k_simp_scale(const double* __restrict__ rho_t, int64_t M, double penal,
                                                    double s_min, double* __restrict__ s) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < M; e += (int64_t)gridDim.x * blockDim.x)
        s[e] = simp_scale(rho_t[e], penal, s_min);
}

__global__ void __launch_bounds__(256) k_to_copy(const double* __restrict__ in, int64_t M, double* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < M; e += (int64_t)gridDim.x * blockDim.x)
        out[e] = in[e];
}

// ---------------------------------------------------------------- unit strain energy and compliance
// 64 elements per 256-thread block (the shape of k_tet4_nl): thread (element, node) loads its node id (coalesced) and
// gathers the node's coordinates and displacement into LDS -- four gathers in flight per element instead of one
// lane's twenty-four dependent loads -- then one lane per element forms eps = sym(sum_a u_a (x) g_a) and
// ce = V (lam1 tr(eps)^2 + 2 mu1 eps:eps). The block's compliance share is the first wave's fixed shuffle tree.
constexpr int UE_REC = 25;   // 4 x (x, u) = 24 doubles, odd stride
__global__ void __launch_bounds__(256) k_tet4_unit_energy(const double* __restrict__ X,
                                                          const int64_t* __restrict__ conn, int64_t M,
                                                          const double* __restrict__ U, double nu,
                                                          const double* __restrict__ rho_t, double penal, double s_min,
                                                          double E0, double* __restrict__ ce, double* __restrict__ dct,
                                                          double* __restrict__ partial, int64_t* __restrict__ bad) {
#pragma clang fp contract(off)
    __shared__ double rec_s[64 * UE_REC];
    const Lame L = lame(1.0, nu);
    const int64_t e0 = (int64_t)blockIdx.x * 64;
    {
        const int le = threadIdx.x >> 2, a = threadIdx.x & 3;
        if (e0 + le < M) {
            const int64_t n = conn[4 * e0 + threadIdx.x];
            double* r = rec_s + le * UE_REC + 6 * a;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                r[k] = X[3 * n + k];
                r[3 + k] = U[3 * n + k];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const int64_t e = e0 + threadIdx.x;
    double w = 0.0;   // this element's share of the compliance
    if (e < M) {
        const double* r = rec_s + threadIdx.x * UE_REC;
        double p[4][3], g[4][3];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k) p[a][k] = r[6 * a + k];
        const double det = tet4_grads_p(p, g);
        double c = 0.0;
        if (!(fabs(det) >= 1e-12)) {
            atomicMin((unsigned long long*)bad, (unsigned long long)e);
        } else {
            double u[4][3], H[3][3];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int k = 0; k < 3; ++k) u[a][k] = r[6 * a + 3 + k];
            tet4_disp_grad(u, g, H);
            const double exy = 0.5 * (H[0][1] + H[1][0]), eyz = 0.5 * (H[1][2] + H[2][1]),
                         exz = 0.5 * (H[0][2] + H[2][0]);
            const double tr = (H[0][0] + H[1][1]) + H[2][2];
            const double ee = ((H[0][0] * H[0][0] + H[1][1] * H[1][1]) + H[2][2] * H[2][2]) +
                              2.0 * ((exy * exy + eyz * eyz) + exz * exz);
            c = (fabs(det) / 6.0) * (L.lam * (tr * tr) + 2.0 * L.mu * ee);
        }
        ce[e] = c;
        double s = 1.0;
        if (rho_t) {
            const double rt = rho_t[e];
            s = simp_scale(rt, penal, s_min);
            if (dct) dct[e] = -penal * (1.0 - s_min) * pow(rt, penal - 1.0) * E0 * c;
        }
        w = s * E0 * c;
    }
    if (partial) {
        w = wave_sum(w);
        if (threadIdx.x == 0) partial[blockIdx.x] = w;
    }
}

__global__ void __launch_bounds__(256) k_to_finish_sum(const double* __restrict__ partial, int64_t n,
                                                       double* __restrict__ out) {
    __shared__ double lds4[4];
    const double t = to_sum(partial, n, lds4);
    if (threadIdx.x == 0) *out = t;
}

// ---------------------------------------------------------------- optimality criteria
__device__ __forceinline__ double oc_b(double dc, double V) { return fmax(0.0, -dc) / V; }

// rho_new_e(l) of a free element; a solid one is 1, a void one rho_min
__device__ __forceinline__ double oc_rho(double rho, double b, double l, double move, double rho_min, int pas) {
    if (pas > 0) return 1.0;
    if (pas < 0) return rho_min;
    const double lo = fmax(rho_min, rho - move), hi = fmin(1.0, rho + move);
    return fmin(hi, fmax(lo, rho * sqrt(b / l)));
}

// per block: min over the free elements' b_e > 0, max b_e of the free elements, sum V_e
__global__ void __launch_bounds__(256) k_oc_bracket(const double* __restrict__ dc, const double* __restrict__ V,
                                                    const int8_t* __restrict__ passive, int64_t M,
                                                    double* __restrict__ part) {
    __shared__ double lds4[4];
    double mn = INFINITY, mx = 0.0, sv = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < M; e += (int64_t)gridDim.x * 256) {
        const double v = V[e];
        sv += v;
        if (passive && passive[e] != 0) continue;
        const double b = oc_b(dc[e], v);
        if (b > 0.0) mn = fmin(mn, b);
        mx = fmax(mx, b);
    }
    mn = block_ext256<false>(mn, lds4);
    mx = block_ext256<true>(mx, lds4);
    sv = block_sum256(sv, lds4);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = mn;
        part[gridDim.x + blockIdx.x] = mx;
        part[2 * gridDim.x + blockIdx.x] = sv;
    }
}

// one block: the bracket [rho_min^2 min b, max b / rho_min^2], the volume target f sum V, and whether any b_e > 0
__global__ void __launch_bounds__(256) k_oc_bracket_finish(const double* __restrict__ part, int G, double volfrac,
                                                           double rho_min, double* __restrict__ st) {
    __shared__ double lds4[4];
    double mn = INFINITY, mx = 0.0;
    for (int i = threadIdx.x; i < G; i += 256) {
        mn = fmin(mn, part[i]);
        mx = fmax(mx, part[G + i]);
    }
    mn = block_ext256<false>(mn, lds4);
    mx = block_ext256<true>(mx, lds4);
    const double sv = to_sum(part + 2 * G, G, lds4);
    if (threadIdx.x == 0) {
        const bool active = mx > 0.0;
        st[TO_LO] = active ? rho_min * rho_min * mn : 1.0;
        st[TO_HI] = active ? mx / (rho_min * rho_min) : 1.0;
        st[TO_TARGET] = volfrac * sv;
        st[TO_VTOT] = sv;
        st[TO_ACTIVE] = active ? 1.0 : 0.0;
    }
}

// FINAL = false: per-block sums of V_e rho_new_e(sqrt(l_lo l_hi));  FINAL: rho_new at l_hi written (the density itself
// where no b_e > 0), per-block sums of V_e rho_new_e and maxima of |rho_new_e - rho_e|. rho_new may alias rho.
template <bool FINAL>
__global__ void __launch_bounds__(256) k_oc_step(const double* __restrict__ rho, const double* __restrict__ dc,
                                                 const double* __restrict__ V, const int8_t* __restrict__ passive,
                                                 int64_t M, double move, double rho_min,
                                                 const double* __restrict__ st, double* __restrict__ part,
                                                 double* rho_new) {
#pragma clang fp contract(off)
    __shared__ double lds4[4];
    const bool active = st[TO_ACTIVE] != 0.0;
    const double l = FINAL ? st[TO_HI] : sqrt(st[TO_LO]) * sqrt(st[TO_HI]);
    double sv = 0.0, ch = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < M; e += (int64_t)gridDim.x * 256) {
        const double v = V[e], r = rho[e];
        double rn = r;
        if (active) rn = oc_rho(r, oc_b(dc[e], v), l, move, rho_min, passive ? (int)passive[e] : 0);
        sv += v * rn;
        if (FINAL) {
            ch = fmax(ch, fabs(rn - r));
            rho_new[e] = rn;
        }
    }
    sv = block_sum256(sv, lds4);
    if (FINAL) ch = block_ext256<true>(ch, lds4);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = sv;
        if (FINAL) part[gridDim.x + blockIdx.x] = ch;
    }
}

// one block: the partial volumes in block order; FINAL = false moves the bracket (volume above the target: the
// multiplier rises), FINAL writes out = (max |rho_new - rho|, reached volume fraction)
template <bool FINAL>
__global__ void __launch_bounds__(256) k_oc_finish(const double* __restrict__ part, int G, double* __restrict__ st,
                                                   double* __restrict__ out) {
    __shared__ double lds4[4];
    const double vol = to_sum(part, G, lds4);
    if (FINAL) {
        double ch = 0.0;
        for (int i = threadIdx.x; i < G; i += 256) ch = fmax(ch, part[G + i]);
        ch = block_ext256<true>(ch, lds4);
        if (threadIdx.x == 0) {
            out[0] = ch;
            out[1] = vol / st[TO_VTOT];
        }
    } else if (threadIdx.x == 0) {
        const double mid = sqrt(st[TO_LO]) * sqrt(st[TO_HI]);
        if (vol > st[TO_TARGET]) st[TO_LO] = mid;
        else st[TO_HI] = mid;
    }
}

}  // namespace fem

using namespace fem;

extern "C" {

int64_t fem_topopt_work_len(int64_t M) {
    const int64_t m = M > 0 ? M : 0;
    const int64_t ue = cdiv(m, 64), oc = TO_STATE + 3 * (int64_t)TO_GRID;
    return ue > oc ? ue : oc;
}

int fem_tet4_volumes(const double* coords, const int64_t* conn, int64_t M, const int32_t* inc_ptr, const int32_t* inc,
                     int64_t N, double* V, double* Vn, int64_t* bad_idx, fem_stream_t stream) {
    if (M > 0) {
        hipLaunchKernelGGL(k_tet4_vol, dim3(stream_grid(M, 256)), dim3(256), 0, S(stream), coords, conn, M, V, bad_idx);
        FEM_LAUNCHED();
    }
    if (Vn && N > 0) {
        hipLaunchKernelGGL(k_to_node<0>, dim3(stream_grid(N, 256)), dim3(256), 0, S(stream), inc_ptr, inc, N, V,
                           (const double*)nullptr, (const double*)nullptr, Vn);
        FEM_LAUNCHED();
    }
    return FEM_OK;
}

int fem_tet4_unit_energy(const double* coords, const int64_t* conn, int64_t M, const double* u, double nu,
                         const double* rho_t, double penal, double s_min, double E0, double* ce, double* dct,
                         double* work, double* compliance, int64_t* bad_idx, fem_stream_t stream) {
    if (!(nu > -1.0 && nu < 0.5)) {
        set_error("fem_tet4_unit_energy: nu must lie in (-1, 0.5)");
        return FEM_EARG;
    }
    if (!ce || !bad_idx || (dct && !rho_t) || (compliance && !work)) {
        set_error("fem_tet4_unit_energy: ce and bad_idx are required, dct needs rho_t, compliance needs work");
        return FEM_EARG;
    }
    if (M <= 0) {
        if (compliance) FEM_HIP(hipMemsetAsync(compliance, 0, sizeof(double), S(stream)));
        return FEM_OK;
    }
    const int64_t nb = cdiv(M, 64);
    hipLaunchKernelGGL(k_tet4_unit_energy, dim3((unsigned)nb), dim3(256), 0, S(stream), coords, conn, M, u, nu, rho_t,
                       penal, s_min, E0, ce, dct, compliance ? work : nullptr, bad_idx);
    FEM_LAUNCHED();
    if (compliance) {
        hipLaunchKernelGGL(k_to_finish_sum, dim3(1), dim3(256), 0, S(stream), work, nb, compliance);
        FEM_LAUNCHED();
    }
    return FEM_OK;
}

int fem_simp_scale(const double* rho_t, int64_t M, double penal, double s_min, double* s, fem_stream_t stream) {
    if (M <= 0) return FEM_OK;
    hipLaunchKernelGGL(k_simp_scale, dim3(stream_grid(M, 256)), dim3(256), 0, S(stream), rho_t, M, penal, s_min, s);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_density_filter(const int64_t* conn, int64_t M, const int32_t* inc_ptr, const int32_t* inc, int64_t N,
                       const double* V, const double* Vn, const double* in, int passes, int adjoint, double penal,
                       double s_min, double* node_tmp, double* elem_tmp, double* out, double* scale,
                       fem_stream_t stream) {
    if (passes < 0 || (adjoint && scale)) {
        set_error("fem_density_filter: passes must be >= 0, and the scale belongs to the forward filter");
        return FEM_EARG;
    }
    if (M <= 0) return FEM_OK;
    if (passes > 0 && (!node_tmp || (passes > 1 && !elem_tmp))) {
        set_error("fem_density_filter: node_tmp (and elem_tmp for more than one pass) required");
        return FEM_EARG;
    }
    hipStream_t st = S(stream);
    const dim3 gn(stream_grid(N, 256)), ge(stream_grid(M, 256)), b(256);
    if (passes == 0) {
        if (out != in) {
            hipLaunchKernelGGL(k_to_copy, ge, b, 0, st, in, M, out);
            FEM_LAUNCHED();
        }
        if (scale) return fem_simp_scale(out, M, penal, s_min, scale, stream);
        return FEM_OK;
    }
    const double* src = in;
    for (int k = 0; k < passes; ++k) {
        double* dst = ((passes - k) & 1) ? out : elem_tmp;   // the last pass lands in out
        const bool last = k == passes - 1;
        if (adjoint) {
            hipLaunchKernelGGL(k_to_node<2>, gn, b, 0, st, inc_ptr, inc, N, V, Vn, src, node_tmp);
            hipLaunchKernelGGL((k_to_elem<true, false>), ge, b, 0, st, conn, M, V, node_tmp, penal, s_min, dst,
                               (double*)nullptr);
        } else {
            hipLaunchKernelGGL(k_to_node<1>, gn, b, 0, st, inc_ptr, inc, N, V, Vn, src, node_tmp);
            if (last && scale)
                hipLaunchKernelGGL((k_to_elem<false, true>), ge, b, 0, st, conn, M, V, node_tmp, penal, s_min, dst,
                                   scale);
            else
                hipLaunchKernelGGL((k_to_elem<false, false>), ge, b, 0, st, conn, M, V, node_tmp, penal, s_min, dst,
                                   (double*)nullptr);
        }
        FEM_LAUNCHED();
        src = dst;
    }
    return FEM_OK;
}

int fem_oc_update(const double* rho, const double* dc, const double* V, const int8_t* passive, int64_t M,
                  double volfrac, double move, double rho_min, int n_bisect, double* work, double* rho_new,
                  double* out, fem_stream_t stream) {
    if (!(volfrac > 0.0 && volfrac <= 1.0) || !(move > 0.0) || !(rho_min > 0.0 && rho_min < 1.0) || n_bisect < 0) {
        set_error("fem_oc_update: volfrac in (0, 1], move > 0, rho_min in (0, 1), n_bisect >= 0 expected");
        return FEM_EARG;
    }
    if (M <= 0) return FEM_OK;
    if (!work || !rho_new || !out) {
        set_error("fem_oc_update: work, rho_new and out are required");
        return FEM_EARG;
    }
    hipStream_t st = S(stream);
    const int G = (int)to_blocks(M);
    double* state = work;
    double* part = work + TO_STATE;
    hipLaunchKernelGGL(k_oc_bracket, dim3(G), dim3(256), 0, st, dc, V, passive, M, part);
    hipLaunchKernelGGL(k_oc_bracket_finish, dim3(1), dim3(256), 0, st, part, G, volfrac, rho_min, state);
    FEM_LAUNCHED();
    for (int k = 0; k < n_bisect; ++k) {
        hipLaunchKernelGGL(k_oc_step<false>, dim3(G), dim3(256), 0, st, rho, dc, V, passive, M, move, rho_min, state,
                           part, (double*)nullptr);
        hipLaunchKernelGGL(k_oc_finish<false>, dim3(1), dim3(256), 0, st, part, G, state, (double*)nullptr);
    }
    FEM_LAUNCHED();
    hipLaunchKernelGGL(k_oc_step<true>, dim3(G), dim3(256), 0, st, rho, dc, V, passive, M, move, rho_min, state, part,
                       rho_new);
    hipLaunchKernelGGL(k_oc_finish<true>, dim3(1), dim3(256), 0, st, part, G, state, out);
    FEM_LAUNCHED();
    return FEM_OK;
}

}  // extern "C"
