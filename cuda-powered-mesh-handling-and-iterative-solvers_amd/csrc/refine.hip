// Mid-edge nodes of c3d4 meshes: the device side of topology.c3d4_to_c3d10 and topology.refine_c3d4.
// The unique edges uedges [E, 2] (a < b, lexicographic: fem_topo_unique on the edge table) are the caller's. An element
// e meets its six edges in the walk (0,1), (1,2), (2,0), (0,3), (1,3), (2,3): slot 6 e + k.
//   k_refine_slots : eid[slot] = index of the slot's edge among uedges (binary search), minslot[edge] = the lowest slot
//                    that names the edge (integer atomicMin: the result does not depend on the order of arrival)
//   k_refine_emit  : c3d10 connectivity [M, 10] = the corners, then N + mid_id[eid[slot]] in walk order
//   k_refine_nodes : coordinates and parents of the N + E nodes: node i < N is itself (parents i, i), node
//                    N + mid_id[j] is 0.5 (x[a] + x[b]) of edge j (parents a, b)
// Plain launches on the caller's stream; nothing is read or stored past the sizes given.
#include "common.hpp"

namespace fem {

constexpr int RF_BLOCK = 256;

__constant__ int RF_WALK[6][2] = {{0, 1}, {1, 2}, {2, 0}, {0, 3}, {1, 3}, {2, 3}};

__global__ void __launch_bounds__(RF_BLOCK) k_refine_slots(const int64_t* __restrict__ conn, int64_t M,
                                                           const int64_t* __restrict__ ue, int64_t E,
                                                           int32_t* __restrict__ eid,
                                                           unsigned long long* __restrict__ minslot) {
    const int64_t s = (int64_t)blockIdx.x * RF_BLOCK + threadIdx.x;
    if (s >= 6 * M) return;
    const int64_t e = s / 6;
    const int k = (int)(s - 6 * e);
    int64_t a = conn[4 * e + RF_WALK[k][0]], b = conn[4 * e + RF_WALK[k][1]];
    if (a > b) {
        const int64_t t = a;
        a = b;
        b = t;
    }
    int64_t lo = 0, hi = E;   // first edge >= (a, b)
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t ma = ue[2 * mid], mb = ue[2 * mid + 1];
        if (ma < a || (ma == a && mb < b))
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo >= E || ue[2 * lo] != a || ue[2 * lo + 1] != b) {   // not an edge of the list: the host checks for -1
        eid[s] = -1;
        return;
    }
    eid[s] = (int32_t)lo;
    atomicMin(minslot + lo, (unsigned long long)s);
}

__global__ void __launch_bounds__(RF_BLOCK) k_refine_emit(const int64_t* __restrict__ conn, int64_t M, int64_t N,
                                                          const int32_t* __restrict__ eid,
                                                          const int64_t* __restrict__ mid_id,
                                                          int64_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * RF_BLOCK + threadIdx.x;
    if (t >= 10 * M) return;
    const int64_t e = t / 10;
    const int k = (int)(t - 10 * e);
    if (k < 4) {
        out[t] = conn[4 * e + k];
    } else {
        const int32_t j = eid[6 * e + (k - 4)];
        out[t] = j >= 0 ? N + mid_id[j] : -1;
    }
}

__global__ void __launch_bounds__(RF_BLOCK) k_refine_nodes(const double* __restrict__ x, int64_t N,
                                                           const int64_t* __restrict__ ue, int64_t E,
                                                           const int64_t* __restrict__ mid_id,
                                                           double* __restrict__ xo, int32_t* __restrict__ parents) {
    const int64_t i = (int64_t)blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i < N) {
        xo[3 * i] = x[3 * i];
        xo[3 * i + 1] = x[3 * i + 1];
        xo[3 * i + 2] = x[3 * i + 2];
        parents[2 * i] = (int32_t)i;
        parents[2 * i + 1] = (int32_t)i;
    } else if (i < N + E) {
        const int64_t j = i - N;
        const int64_t a = ue[2 * j], b = ue[2 * j + 1];
        const int64_t m = mid_id[j];
        if (m < 0 || m >= E || a < 0 || a >= N || b < 0 || b >= N) return;
        const int64_t o = N + m;
        xo[3 * o] = 0.5 * (x[3 * a] + x[3 * b]);
        xo[3 * o + 1] = 0.5 * (x[3 * a + 1] + x[3 * b + 1]);
        xo[3 * o + 2] = 0.5 * (x[3 * a + 2] + x[3 * b + 2]);
        parents[2 * o] = (int32_t)a;
        parents[2 * o + 1] = (int32_t)b;
    }
}

}  // namespace fem

using namespace fem;

static bool rf_sizes_ok(const char* fn, int64_t M, int64_t N, int64_t E) {
    if (M < 0 || N < 0 || E < 0 || N + E > (int64_t)INT32_MAX || M > (int64_t)INT32_MAX) {
        set_error("%s: %lld elements, %lld nodes, %lld edges (element and node ids must fit int32)", fn, (long long)M,
                  (long long)N, (long long)E);
        return false;
    }
    return true;
}

extern "C" {

int fem_refine_edge_slots(const int64_t* conn, int64_t M, const int64_t* uedges, int64_t E, int32_t* eid,
                          int64_t* minslot, fem_stream_t stream) {
    if (!rf_sizes_ok("fem_refine_edge_slots", M, 0, E)) return FEM_EARG;
    if (M == 0) return FEM_OK;
    if (!conn || !uedges || !eid || !minslot) {
        set_error("fem_refine_edge_slots: null argument");
        return FEM_EARG;
    }
    hipLaunchKernelGGL(k_refine_slots, dim3((unsigned)cdiv(6 * M, RF_BLOCK)), dim3(RF_BLOCK), 0, S(stream), conn, M,
                       uedges, E, eid, (unsigned long long*)minslot);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_refine_emit(const int64_t* conn, int64_t M, int64_t N, const int32_t* eid, const int64_t* mid_id, int64_t* out,
                    fem_stream_t stream) {
    if (!rf_sizes_ok("fem_refine_emit", M, N, 0)) return FEM_EARG;
    if (M == 0) return FEM_OK;
    if (!conn || !eid || !mid_id || !out) {
        set_error("fem_refine_emit: null argument");
        return FEM_EARG;
    }
    hipLaunchKernelGGL(k_refine_emit, dim3((unsigned)cdiv(10 * M, RF_BLOCK)), dim3(RF_BLOCK), 0, S(stream), conn, M, N,
                       eid, mid_id, out);
    FEM_LAUNCHED();
    return FEM_OK;
}

int fem_refine_nodes(const double* coords, int64_t N, const int64_t* uedges, int64_t E, const int64_t* mid_id,
                     double* coords_out, int32_t* parents, fem_stream_t stream) {
    if (!rf_sizes_ok("fem_refine_nodes", 0, N, E)) return FEM_EARG;
    if (N + E == 0) return FEM_OK;
    if (!coords || !coords_out || !parents || (E > 0 && (!uedges || !mid_id))) {
        set_error("fem_refine_nodes: null argument");
        return FEM_EARG;
    }
    hipLaunchKernelGGL(k_refine_nodes, dim3((unsigned)cdiv(N + E, RF_BLOCK)), dim3(RF_BLOCK), 0, S(stream), coords, N,
                       uedges, E, mid_id, coords_out, parents);
    FEM_LAUNCHED();
    return FEM_OK;
}

}  // extern "C"
