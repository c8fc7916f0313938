// Lane-paired SELL-64 layout for bs = 1 with 16-bit column deltas: each lane reads two consecutive entries of its
// row with one 16-byte value load and one 4-byte column load (the plain layout issues an 8-byte and a 2-byte load
// per entry; tools/spmv_layout.py: 55.8 -> 47.8 us on the 10M Poisson matrix, warm).
// Slice s (width w, base p0 = slice_ptr[s]): entry k < 2*(w/2) of lane l at p0 + (k/2)*128 + 2*l + (k%2), the odd
// tail entry (w odd) at p0 + (w/2)*128 + l. Same footprint and slice_ptr as the plain layout.
#pragma once
#include "common.hpp"

namespace fem {

// plain -> paired layout (values and 16-bit deltas)
static __global__ void k_sell_pair(int64_t nslices, const int64_t* __restrict__ slice_ptr, const double* __restrict__ vin,
                            const int16_t* __restrict__ cin, double* __restrict__ vout, int16_t* __restrict__ cout) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nslices * 64;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = t >> 6;
        const int l = (int)(t & 63);
        const int64_t p0 = slice_ptr[s];
        const int w = (int)((slice_ptr[s + 1] - p0) >> 6);
        const int np = w >> 1;
        for (int k = 0; k < w; ++k) {
            const int64_t src = p0 + 64 * k + l;
            const int64_t dst = k < 2 * np ? p0 + (int64_t)(k >> 1) * 128 + 2 * l + (k & 1) : p0 + (int64_t)np * 128 + l;
            vout[dst] = vin[src];
            cout[dst] = cin[src];
        }
    }
}


// gathered x element: plain load (SC1 = 0), an agent-scope relaxed load (1: global_load sc1, the coherent form that
// may replace the consumer's acquire when every producer store was sc1, MI355X_MICROARCH.md, Valid forms), or a
// system-scope relaxed load (2: sc0 sc1, past this GPU's L2 -- rows another GPU wrote into this GPU's memory)
template <int SC1>
__device__ __forceinline__ double ldx(const double* p) {
    if constexpr (SC1 == 2) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else if constexpr (SC1 == 1) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}

// SC1 = 3: per element, 2 (system scope) for columns outside [own_lo, own_hi) -- rows another GPU wrote into this
// GPU's memory, never cached here -- and 1 for the rest (this GPU's rows, L2-served)
template <int SC1>
__device__ __forceinline__ double ldx_col(const double* x, int col, int own_lo, int own_hi) {
    if constexpr (SC1 == 3) {
        if (col < own_lo || col >= own_hi) return ldx<2>(x + col);
        return ldx<1>(x + col);
    } else {
        return ldx<SC1>(x + col);
    }
}

// Slice-uniform column deltas (FEM_TUNE_PK_UNI). When the 64 rows of a slice take their columns at the same
// offsets from the row (every row's deltas a subset of one sorted list of `w` deltas -- FEM meshes numbered along a
// structured sweep, e.g. every slice of the Kuhn cubes), the slice stores that list ONCE: ucol[uoff[s] + k] = delta of
// entry k for every lane, and rows lacking an offset hold a zero value there (the lane-paired value layout is kept,
// entries in list order). The SpMV then reads the deltas with wave-uniform loads: 10 -> 8 bytes per entry on the
// matrix stream. Real entries keep their order within the row (ascending column), so every row sum adds the same
// products in the same order, with +-0 terms interleaved. Other slices: uoff[s] = -1, per-lane deltas as before.
// k_sell_uniform writes the paired values / deltas of the uniform slices (pcols16 stays a valid per-lane copy: kernels
// that ignore uoff read the same entries) and, with pair_rest, the plain lane-paired copy (k_sell_pair) of every other
// slice -- one pass over the matrix instead of k_sell_pair followed by a rewrite of nearly every slice. A slice qualifies when: it is full (no rows
// past nrows), width <= SU_MAXW, the row of greatest length has exactly w entries (no extra padding), every other
// row's real deltas are a subsequence of that row's, every padded column row + delta lies in [0, nrows), and the
// trailing SELL padding entries of every row are (delta 0, value 0).
constexpr int SU_MAXW = 64;

constexpr int PK_T = 1024;               // threads per workgroup of the persistent schedule (16 waves, 4 per SIMD)
constexpr int PK_WAVES = PK_T / 64;

// gather window per logical workgroup: the first and last workgroup owning a column of its rows. A slice-uniform
// slice (sell_pair.hpp) makes every lane gather at the whole slice's delta list, i.e. also at offsets its own row
// lacks (value 0 there). So the window of a slice is taken over the UNION of its rows' deltas applied to every row
// of the slice: [s*64 + min delta, s*64 + 63 + max delta]. Every column any lane reads is then inside a window the
// workgroup waits on -- no read of an unsynchronised u, whose value (0 * Inf = NaN) would otherwise matter.
__device__ __forceinline__ void pk_slice_span(int64_t s, int64_t nrows, int dmin, int dmax, int64_t* cmin, int64_t* cmax) {
    for (int off = 32; off > 0; off >>= 1) {
        const int a2 = __shfl_xor(dmin, off), b2 = __shfl_xor(dmax, off);
        dmin = a2 < dmin ? a2 : dmin;
        dmax = b2 > dmax ? b2 : dmax;
    }
    int64_t lo = s * 64 + dmin, hi = s * 64 + 63 + dmax;
    if (hi >= nrows) hi = nrows - 1;
    if (lo < 0) lo = 0;
    if (lo > hi) lo = hi;
    *cmin = lo;
    *cmax = hi;
}

// a slice's lane-paired 16-bit deltas (pair_pos) written as one 32-bit store per pair (entries 2 k2, 2 k2 + 1 of lane
// l are adjacent halves), then the unpaired last entry of an odd width: full 256-byte rows per store instruction
template <class Delta>
__device__ __forceinline__ void sl_store_pairs(int16_t* __restrict__ out, int w, int l, const Delta& delta) {
    const int np = w >> 1;
    int32_t* o32 = reinterpret_cast<int32_t*>(out);   // out = pout + slice start: 128-byte aligned
    for (int k2 = 0; k2 < np; ++k2)
        o32[k2 * 64 + l] = (int32_t)((uint32_t)(uint16_t)delta(2 * k2) | ((uint32_t)(uint16_t)delta(2 * k2 + 1) << 16));
    if (w & 1) out[(int64_t)np * 128 + l] = (int16_t)delta(w - 1);
}

// The solver layout of one slice s of a bs = 1 pattern, by the wave whose lane l is row s * 64 + l (k_sell_sl_pattern,
// and k_sell_fill_graph right after it wrote the slice's deltas): see k_sell_sl_pattern (pcg.hip). cand: SU_MAXW ints of
// the wave's LDS. delta(k): this lane's plain 16-bit delta of entry k of the slice (each lane reads only its own row's
// entries before the shuffles) -- from memory (k_sell_sl_pattern) or from the rows the fill pass holds in LDS.
// span != null: the slice's owner-workgroup span (owner(cmin), owner(cmax)) is stored in span[s] and the windows are
// formed from all spans by k_win_from_spans, instead of two atomics per slice on `win` (the G windows share a few
// cache lines: 54,000 atomics on 16 lines serialise in the L2 -- 72 us of the 10M fill pass).
template <class Delta>
__device__ __forceinline__ void sl_pattern_slice(int64_t s, int l, int64_t nslices, int64_t nrows,
                                                 const int64_t* __restrict__ slice_ptr, const Delta& delta,
                                                 int16_t* __restrict__ pout, int16_t* __restrict__ ucol,
                                                 int32_t* __restrict__ uoff, int G, int* __restrict__ win, int* cand,
                                                 int2* __restrict__ span = nullptr) {
    const int64_t p0 = slice_ptr[s];
    const int w = (int)((slice_ptr[s + 1] - p0) >> 6);
    const int64_t row = s * 64 + l;
    if (G > 0) {   // gather window (k_pk_window): the delta union of the slice over its owner workgroup
        int dmin = 0, dmax = 0;
        if (row < nrows)
            for (int k = 0; k < w; ++k) {
                const int d = delta(k);
                dmin = d < dmin ? d : dmin;
                dmax = d > dmax ? d : dmax;
            }
        int64_t cmin, cmax;
        pk_slice_span(s, nrows, dmin, dmax, &cmin, &cmax);
        const int64_t WV = (int64_t)G * PK_WAVES;
        auto owner = [&](int64_t r) { return (int)((((r >> 6) + 1) * WV - 1) / nslices / PK_WAVES); };
        if (l == 0) {
            if (span) {
                span[s] = make_int2(owner(cmin), owner(cmax));
            } else {
                const int me = owner(row);
                atomicMin(win + me, owner(cmin));
                atomicMax(win + G + me, owner(cmax));
            }
        }
    }
    bool ok = (s + 1) * 64 <= nrows && w > 0 && w <= SU_MAXW;
    int len = 0;
    if (ok) {
        int prev = -(1 << 30);
        for (int k = 0; k < w; ++k) {
            const int d = delta(k);
            if (len == k && d > prev) {
                ++len;
                prev = d;
            } else if (d != 0) {
                ok = false;
            }
        }
    }
    ok = __all(ok);
    const unsigned long long full = __ballot(ok && len == w);
    if (ok && full) {
        const int c = __builtin_ctzll(full);
        for (int k = 0; k < w; ++k) {
            const int d = __shfl(delta(k), c, 64);
            if (l == 0) cand[k] = d;
            const int64_t col = row + d;
            if (col < 0 || col >= nrows) ok = false;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int i = 0;
        for (int k = 0; k < len && ok; ++k) {
            const int d = delta(k);
            while (i < w && cand[i] < d) ++i;
            if (i == w || cand[i] != d) ok = false;
            ++i;
        }
    } else {
        ok = false;
    }
    ok = __all(ok);
    if (!ok) {
        if (l == 0) uoff[s] = -1;
        sl_store_pairs(pout + p0, w, l, delta);
        return;
    }
    const int32_t uo = (int32_t)(2 * (p0 >> 6));   // even: the deltas are read as int32 pairs
    sl_store_pairs(pout + p0, w, l, [&](int k) { return cand[k]; });
    for (int k = l; k < w; k += 64) ucol[uo + k] = (int16_t)cand[k];
    if (l == 0) uoff[s] = uo;
}
// the gather windows from the per-slice owner spans (sl_pattern_slice with span): a wave per owner workgroup me, its
// slices {s : owner(s) = me} (owner is monotone in s) found by binary search, min / max over their spans; an owner
// without slices gets the empty window (G, -1) of k_pk_window_init
__attribute__((unused)) static __global__ void __launch_bounds__(256) k_win_from_spans(int G, int64_t nslices,
                                                                                       const int2* __restrict__ span,
                                                                                       int* __restrict__ win) {
    const int me = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int l = threadIdx.x & 63;
    if (me >= G) return;   // wave-uniform
    const int64_t WV = (int64_t)G * PK_WAVES;
    auto owner_s = [&](int64_t s) { return (int)(((s + 1) * WV - 1) / nslices / PK_WAVES); };
    auto first = [&](int o) {   // first slice whose owner is >= o
        int64_t lo = 0, hi = nslices;
        while (lo < hi) {
            const int64_t m = (lo + hi) >> 1;
            if (owner_s(m) < o) lo = m + 1;
            else hi = m;
        }
        return lo;
    };
    const int64_t s0 = first(me), s1 = first(me + 1);
    int lo = G, hi = -1;
    for (int64_t s = s0 + l; s < s1; s += 64) {
        const int2 v = span[s];
        lo = v.x < lo ? v.x : lo;
        hi = v.y > hi ? v.y : hi;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int a = __shfl_xor(lo, off), b = __shfl_xor(hi, off);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if (l == 0) {
        win[me] = lo;
        win[G + me] = hi;
    }
}

__attribute__((unused)) static __global__ void __launch_bounds__(256) k_sell_uniform(int64_t nslices, int64_t nrows,
                                                             const int64_t* __restrict__ slice_ptr,
                                                             const double* __restrict__ vin,
                                                             const int16_t* __restrict__ cin, double* __restrict__ vout,
                                                             int16_t* __restrict__ cout, int16_t* __restrict__ ucol,
                                                             int32_t* __restrict__ uoff, int pair_rest) {
    __shared__ int cand_all[4][SU_MAXW];
    const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;   // one wave per slice
    const int l = threadIdx.x & 63;
    int* cand = cand_all[(threadIdx.x >> 6) & 3];
    if (s >= nslices) return;   // wave-uniform
    const int64_t p0 = slice_ptr[s];
    const int w = (int)((slice_ptr[s + 1] - p0) >> 6);
    const int64_t row = s * 64 + l;
    bool ok = (s + 1) * 64 <= nrows && w > 0 && w <= SU_MAXW;
    // real entries of this row: the strictly increasing prefix of its deltas; the rest must be (0, 0.0) padding
    int len = 0;
    if (ok) {
        int prev = -(1 << 30);
        for (int k = 0; k < w; ++k) {
            const int d = cin[p0 + 64 * k + l];
            if (len == k && d > prev) {
                ++len;
                prev = d;
            } else if (d != 0 || vin[p0 + 64 * k + l] != 0.0) {
                ok = false;
            }
        }
    }
    ok = __all(ok);
    const unsigned long long full = __ballot(ok && len == w);
    if (ok && full) {
        const int c = __builtin_ctzll(full);   // the lowest full-length row supplies the delta list
        for (int k = 0; k < w; ++k) {
            const int d = __shfl((int)cin[p0 + 64 * k + l], c, 64);
            if (l == 0) cand[k] = d;
            const int64_t col = row + d;
            if (col < 0 || col >= nrows) ok = false;
        }
        // cand (written by lane 0) visible to the whole wave
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int i = 0;
        for (int k = 0; k < len && ok; ++k) {   // subsequence check
            const int d = cin[p0 + 64 * k + l];
            while (i < w && cand[i] < d) ++i;
            if (i == w || cand[i] != d) ok = false;
            ++i;
        }
    } else {
        ok = false;
    }
    ok = __all(ok);
    const int32_t uo = (int32_t)(2 * (p0 >> 6));   // even: the deltas are read as int32 pairs
    const int np = w >> 1;
    if (!ok) {
        if (l == 0) uoff[s] = -1;
        if (pair_rest) {   // k_sell_pair's copy of this slice
            for (int k = 0; k < w; ++k) {
                const int64_t src = p0 + 64 * k + l;
                const int64_t dst = k < 2 * np ? p0 + (int64_t)(k >> 1) * 128 + 2 * l + (k & 1) : p0 + (int64_t)np * 128 + l;
                vout[dst] = vin[src];
                cout[dst] = cin[src];
            }
        }
        return;
    }
    int kr = 0;   // next real entry of this row
    for (int k = 0; k < w; ++k) {
        const int d = cand[k];
        double v = 0.0;
        if (kr < len && (int)cin[p0 + 64 * kr + l] == d) {
            v = vin[p0 + 64 * kr + l];
            ++kr;
        }
        const int64_t dst = k < 2 * np ? p0 + (int64_t)(k >> 1) * 128 + 2 * l + (k & 1) : p0 + (int64_t)np * 128 + l;
        vout[dst] = v;
        cout[dst] = (int16_t)d;
    }
    for (int k = l; k < w; k += 64) ucol[uo + k] = (int16_t)cand[k];
    if (l == 0) uoff[s] = uo;
}

// plain SELL values of a solver-layout (paired, slice-uniform) bs = 1 matrix: lane l walks its row's plain deltas and
// the slice's list (uniform) or maps plain entry k to its paired position (other slices); padding entries zero
__attribute__((unused)) static __global__ void __launch_bounds__(256) k_sell_sl_unpair(int64_t nslices,
                                                               const int64_t* __restrict__ slice_ptr,
                                                               const int16_t* __restrict__ cin,
                                                               const int32_t* __restrict__ uoff,
                                                               const int16_t* __restrict__ ucol,
                                                               const int32_t* __restrict__ rowptr, int64_t nrows,
                                                               const double* __restrict__ vin,
                                                               double* __restrict__ vout) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nslices * 64;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = t >> 6;
        const int l = (int)(t & 63);
        const int64_t p0 = slice_ptr[s];
        const int w = (int)((slice_ptr[s + 1] - p0) >> 6);
        const int64_t row = s * 64 + l;
        const int len = row < nrows ? rowptr[row + 1] - rowptr[row] : 0;
        const int uo = uoff[s];
        int u = 0;
        for (int k = 0; k < w; ++k) {
            double v = 0.0;
            if (k < len) {
                int pos = k;
                if (uo >= 0) {   // the list position of this entry's delta (rows' deltas are subsequences of it)
                    const int d = cin[p0 + 64 * k + l];
                    while (u < w && (int)ucol[uo + u] < d) ++u;
                    pos = u++;
                }
                v = vin[p0 + pair_pos(pos, w, l)];
            }
            vout[p0 + 64 * k + l] = v;
        }
    }
}

// y_row (bs = 1) of one slice row in the paired layout; U pairs in flight. UNI: the slice's deltas from the
// wave-uniform list ucl (k_sell_uniform), else per lane from cols.
template <int U, int SC1, bool UNI>
__device__ __forceinline__ double sell_row_pair_body(int64_t p0, int w, int base, int lane,
                                                     const int16_t* __restrict__ cols, const int16_t* __restrict__ ucl,
                                                     const double* __restrict__ vals, const double* __restrict__ x,
                                                     int own_lo, int own_hi) {
    const int np = w >> 1;
    const double2* v2 = reinterpret_cast<const double2*>(vals + p0) + lane;
    const int32_t* c2 = UNI ? reinterpret_cast<const int32_t*>(ucl) : reinterpret_cast<const int32_t*>(cols + p0) + lane;
    double acc = 0.0;
    for (int j0 = 0; j0 < np; j0 += U) {
        int32_t cc[U];
        double2 vv[U];
        double x0[U], x1[U];
#pragma unroll
        for (int j = 0; j < U; ++j) cc[j] = (j0 + j < np) ? c2[UNI ? (j0 + j) : 64 * (j0 + j)] : 0;
#pragma unroll
        for (int j = 0; j < U; ++j) vv[j] = (j0 + j < np) ? v2[64 * (j0 + j)] : double2{0.0, 0.0};
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int lo = (int)(int16_t)(cc[j] & 0xffff), hi = (int)(int16_t)(cc[j] >> 16);
            x0[j] = (j0 + j < np) ? ldx_col<SC1>(x, base + lo, own_lo, own_hi) : 0.0;
            x1[j] = (j0 + j < np) ? ldx_col<SC1>(x, base + hi, own_lo, own_hi) : 0.0;
        }
#pragma unroll
        for (int j = 0; j < U; ++j)
            if (j0 + j < np) {
                acc += vv[j].x * x0[j];
                acc += vv[j].y * x1[j];
            }
    }
    if (w & 1) {
        const int64_t t = p0 + (int64_t)np * 128 + lane;
        const int d = UNI ? (int)ucl[w - 1] : (int)cols[t];
        acc += vals[t] * ldx_col<SC1>(x, base + d, own_lo, own_hi);
    }
    return acc;
}

// Per-slice descriptor record of the diagonal-free stream (FEM_TUNE_PK_DESC), written by k_sell_offdiag beside the
// stream and read by k_pcg_persist<.., DESC = true> with scalar loads: everything the SpMV of a slice needs before its
// first value load, at an address that depends on the slice index alone. 12 words: the value base p0 (words 0-1), the
// streamed width (2), word 3 = kd (bits 0-7, signed; -1: nothing left out) | kind (bits 8-15) | the delta of an odd
// width's last entry (bits 16-31), then the streamed delta list two per word, zero-padded to PKD_CAP entries.
// Kinds: PKD_OD a slice-uniform slice without its diagonal, PKD_FULL a slice-uniform slice that kept its full rows,
// PKD_LANE per-lane deltas or a list past PKD_CAP -- such a slice is read as before (uoff, the lists, kd's list slot).
constexpr int PKD_CAP = 16;
enum { PKD_OD = 0, PKD_FULL = 1, PKD_LANE = 2 };
struct alignas(64) PkDesc {
    uint32_t w[4 + PKD_CAP / 2];
    uint32_t pad[4];   // (never written or read: the stride keeps a record inside one 64-byte line)
};
static_assert(sizeof(PkDesc) == 64, "persistent PCG: one 64-byte descriptor record per slice");

// Diagonal-free value stream of the persistent schedule (FEM_TUNE_PK_OFFDIAG), private to one solver context. A
// slice-uniform slice whose delta list holds delta 0 at list index kd stores its other w - 1 list entries, in list
// order, lane-paired as a slice of width w - 1 at the slice's own base (slice_ptr is kept, so one pointer array
// serves both streams and the slice's last 512-byte row is simply never read); its delta list without the 0 sits at
// the slice's uoff in a second list array, so delta pairs line up with value pairs; the last of the slice's 2 w list
// slots (uoff[s] + 2 w - 1, never part of a list) holds kd, so the kernel needs no further array. The row's diagonal
// goes to the dense diag[n]. Every other slice (per-lane deltas, or a list without 0) is copied as it is: kd = -1
// (kd[s] holds the same per slice for the host).
// One wave per slice; ovals / oucol are read only by k_pcg_persist<.., OD = true>.
__attribute__((unused)) static __global__ void __launch_bounds__(256) k_sell_offdiag(int64_t nslices, int64_t nrows,
                                                             const int64_t* __restrict__ slice_ptr,
                                                             const double* __restrict__ pvals,
                                                             const int32_t* __restrict__ uoff,
                                                             const int16_t* __restrict__ ucol,
                                                             double* __restrict__ ovals, int16_t* __restrict__ oucol,
                                                             int32_t* __restrict__ kd, double* __restrict__ diag,
                                                             PkDesc* __restrict__ desc) {
    const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int l = threadIdx.x & 63;
    if (s >= nslices) return;   // wave-uniform
    const int64_t p0 = slice_ptr[s];
    const int w = (int)((slice_ptr[s + 1] - p0) >> 6);
    const int uo = uoff[s];
    const int64_t row = s * 64 + l;
    int kdv = -1;
    if (uo >= 0) {   // w <= SU_MAXW = 64: one list entry per lane
        const unsigned long long z = __ballot(l < w && ucol[uo + l] == 0);
        if (z) kdv = __builtin_ctzll(z);
    }
    if (l == 0) {
        kd[s] = kdv;
        if (uo >= 0) oucol[uo + 2 * w - 1] = (int16_t)kdv;
    }
    if (desc) {   // the slice's record (PkDesc): the header by lane 0, one word of two streamed deltas per lane
        const int ws = w - (kdv >= 0);
        const int kind = (uo < 0 || ws > PKD_CAP) ? PKD_LANE : kdv >= 0 ? PKD_OD : PKD_FULL;
        auto sd = [&](int k) {   // streamed list entry k (the list without its 0), 0 past the list
            return (kind != PKD_LANE && k < ws) ? (int)ucol[uo + k + (kdv >= 0 && k >= kdv)] : 0;
        };
        uint32_t* rec = reinterpret_cast<uint32_t*>(desc + s);
        if (l < PKD_CAP / 2) rec[4 + l] = (uint32_t)(uint16_t)sd(2 * l) | ((uint32_t)(uint16_t)sd(2 * l + 1) << 16);
        if (l == 0) {
            const int tail = (ws & 1) ? sd(ws - 1) : 0;
            rec[0] = (uint32_t)((uint64_t)p0 & 0xffffffffu);
            rec[1] = (uint32_t)((uint64_t)p0 >> 32);
            rec[2] = (uint32_t)ws;
            rec[3] = (uint32_t)(uint8_t)(int8_t)(kind == PKD_LANE ? -1 : kdv) | ((uint32_t)kind << 8) |
                     ((uint32_t)(uint16_t)tail << 16);
        }
    }
    if (kdv < 0) {
        for (int k = 0; k < w; ++k) ovals[p0 + 64 * k + l] = pvals[p0 + 64 * k + l];
        if (uo >= 0)
            for (int k = l; k < w; k += 64) oucol[uo + k] = ucol[uo + k];
        if (row < nrows) diag[row] = 0.0;
        return;
    }
    diag[row] = pvals[p0 + pair_pos(kdv, w, l)];   // a uniform slice is full: row < nrows
    const int w1 = w - 1, np1 = w1 >> 1;
    double2* o2 = reinterpret_cast<double2*>(ovals + p0) + l;
    for (int j = 0; j < np1; ++j) {
        const int k0 = 2 * j + (2 * j >= kdv), k1 = 2 * j + 1 + (2 * j + 1 >= kdv);
        o2[64 * j] = double2{pvals[p0 + pair_pos(k0, w, l)], pvals[p0 + pair_pos(k1, w, l)]};
    }
    if (w1 & 1) ovals[p0 + (int64_t)np1 * 128 + l] = pvals[p0 + pair_pos(w1 - 1 + (w1 - 1 >= kdv), w, l)];
    for (int k = l; k < w1; k += 64) oucol[uo + k] = ucol[uo + k + (k >= kdv)];
}

// plain SELL values rebuilt from the diagonal-free stream and diag (test-only: fem_pcg_debug_offdiag): k_sell_sl_unpair
// with the list position mapped through kd. ucol is the FULL list of the shared layout.
__attribute__((unused)) static __global__ void __launch_bounds__(256) k_sell_od_unpair(int64_t nslices,
                                                               const int64_t* __restrict__ slice_ptr,
                                                               const int16_t* __restrict__ cin,
                                                               const int32_t* __restrict__ uoff,
                                                               const int16_t* __restrict__ ucol,
                                                               const int32_t* __restrict__ kd,
                                                               const double* __restrict__ diag,
                                                               const int32_t* __restrict__ rowptr, int64_t nrows,
                                                               const double* __restrict__ ovals,
                                                               double* __restrict__ vout) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nslices * 64;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = t >> 6;
        const int l = (int)(t & 63);
        const int64_t p0 = slice_ptr[s];
        const int w = (int)((slice_ptr[s + 1] - p0) >> 6);
        const int64_t row = s * 64 + l;
        const int len = row < nrows ? rowptr[row + 1] - rowptr[row] : 0;
        const int uo = uoff[s];
        const int kdv = kd[s];
        int u = 0;
        for (int k = 0; k < w; ++k) {
            double v = 0.0;
            if (k < len) {
                int pos = k;
                if (uo >= 0) {
                    const int d = cin[p0 + 64 * k + l];
                    while (u < w && (int)ucol[uo + u] < d) ++u;
                    pos = u++;
                }
                if (kdv < 0) v = ovals[p0 + pair_pos(pos, w, l)];
                else if (pos == kdv) v = diag[row];
                else v = ovals[p0 + pair_pos(pos - (pos > kdv), w - 1, l)];
            }
            vout[p0 + 64 * k + l] = v;
        }
    }
}

// y_row of one slice-uniform slice row in the diagonal-free stream: the w1 streamed list entries in list order, with
// the row's diagonal term (diagonal times own u, both held by the lane) added by acc = diag(acc), which must be
// `acc + d * u` like the streamed terms; it is called only where the term belongs, so what it forms or loads occupies
// no registers while the slice's loads are in flight. The term goes where the full list had
// delta 0, i.e. before streamed entry kd (wave-uniform; kd = w1: after the last; kd < 0: a uniform slice that kept
// its full rows, nothing inserted). Every term is `acc += a * b` like the streamed ones, so the row sum is the one
// sell_row_pair_body<.., UNI = true> forms on the full slice, bit for bit.
template <int U, int SC1, class Diag>
__device__ __forceinline__ double sell_row_pair_od_body(int64_t p0, int w1, int base, int lane,
                                                        const int16_t* __restrict__ ucl,
                                                        const double* __restrict__ vals, const double* __restrict__ x,
                                                        int own_lo, int own_hi, int kd, const Diag& diag) {
    const int np = w1 >> 1;
    const double2* v2 = reinterpret_cast<const double2*>(vals + p0) + lane;
    const int32_t* c2 = reinterpret_cast<const int32_t*>(ucl);
    double acc = 0.0;
    for (int j0 = 0; j0 < np; j0 += U) {
        int32_t cc[U];
        double2 vv[U];
        double x0[U], x1[U];
#pragma unroll
        for (int j = 0; j < U; ++j) cc[j] = (j0 + j < np) ? c2[j0 + j] : 0;
#pragma unroll
        for (int j = 0; j < U; ++j) vv[j] = (j0 + j < np) ? v2[64 * (j0 + j)] : double2{0.0, 0.0};
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int lo = (int)(int16_t)(cc[j] & 0xffff), hi = (int)(int16_t)(cc[j] >> 16);
            x0[j] = (j0 + j < np) ? ldx_col<SC1>(x, base + lo, own_lo, own_hi) : 0.0;
            x1[j] = (j0 + j < np) ? ldx_col<SC1>(x, base + hi, own_lo, own_hi) : 0.0;
        }
#pragma unroll
        for (int j = 0; j < U; ++j)
            if (j0 + j < np) {
                const int k = 2 * (j0 + j);
                if (k == kd) acc = diag(acc);
                acc += vv[j].x * x0[j];
                if (k + 1 == kd) acc = diag(acc);
                acc += vv[j].y * x1[j];
            }
    }
    if (w1 & 1) {
        const int64_t t = p0 + (int64_t)np * 128 + lane;
        const double xt = ldx_col<SC1>(x, base + (int)ucl[w1 - 1], own_lo, own_hi);
        if (kd == w1 - 1) acc = diag(acc);
        acc += vals[t] * xt;
    }
    if (kd == w1) acc = diag(acc);
    return acc;
}

// a slice of the diagonal-free stream (k_sell_offdiag): uoff as in the shared layout, ucol the private lists, kd read
// from the slice's list slot 2 w - 1
template <int U, int SC1, class Diag>
__device__ __forceinline__ double sell_row_pair_od(int64_t s, int lane, const int64_t* __restrict__ slice_ptr,
                                                   const int16_t* __restrict__ cols, const double* __restrict__ vals,
                                                   const double* __restrict__ x, const int32_t* __restrict__ uoff,
                                                   const int16_t* __restrict__ ucol, const Diag& diag) {
    const int64_t p0 = slice_ptr[s];
    const int w = (int)((slice_ptr[s + 1] - p0) >> 6);
    const int base = (int)(s * 64 + lane);
    const int uo = __builtin_amdgcn_readfirstlane(uoff[s]);
    if (uo >= 0) {
        const int kdv = __builtin_amdgcn_readfirstlane((int)ucol[uo + 2 * w - 1]);
        return sell_row_pair_od_body<U, SC1>(p0, w - (kdv >= 0), base, lane, ucol + uo, vals, x, 0, 0, kdv, diag);
    }
    return sell_row_pair_body<U, SC1, false>(p0, w, base, lane, cols, nullptr, vals, x, 0, 0);
}

// A slice's record held in scalar registers: read through the constant address space (the records are written before
// the launch and never during it), so the loads are scalar loads that touch neither a vector register nor the
// vector-memory counter, and may be requested long before their slice's turn.
typedef uint32_t pk_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t pk_u32x8 __attribute__((ext_vector_type(8)));
typedef const __attribute__((address_space(4))) PkDesc* PkDescPtr;
struct PkRec {
    pk_u32x4 h;
    pk_u32x8 d;
    __device__ __forceinline__ int kind() const { return (int)((h.w >> 8) & 0xffu); }
};
__device__ __forceinline__ PkRec pk_rec_load(PkDescPtr desc, int s) {
    typedef const __attribute__((address_space(4))) pk_u32x4* P4;
    typedef const __attribute__((address_space(4))) pk_u32x8* P8;
    P4 q = reinterpret_cast<P4>(desc + s);
    PkRec r;
    r.h = q[0];
    r.d = *reinterpret_cast<P8>(q + 1);
    return r;
}

// y_row of a record slice (PKD_OD / PKD_FULL): sell_row_pair_od_body's sum -- the same terms `acc += a * b` in list
// order, the diagonal term before streamed entry kd -- with the value base, the width, kd and every delta taken from
// the record's scalar registers. A round's value loads and gathers depend on no earlier load, so they are issued
// together and the wave waits once per round, before the round's first product. The delta words move down by U after
// each round (scalar moves), which keeps every register index a constant. Every address is written as a wave-uniform
// 64-bit base (value row of the round, x + first row of the slice + delta: scalar arithmetic) plus the lane's 32-bit
// offset; the compiler turns that into two per-lane bases per slice and one 64-bit add per load, and keeps no
// per-lane address across the slots (written per lane as in sell_row_pair_od_body, the 7-slot build spilled 84 bytes).
// row0: the slice's first row.
template <int U, int SC1, class Diag>
__device__ __forceinline__ double sell_row_pair_rec(const PkRec& rc, int row0, int lane, const double* __restrict__ vals,
                                                    const double* __restrict__ x, const Diag& diag) {
    const int64_t p0 = (int64_t)((uint64_t)rc.h.x | ((uint64_t)rc.h.y << 32));
    const int w1 = (int)rc.h.z;
    const int kd = (int)(int8_t)(rc.h.w & 0xffu);
    const int dtail = (int)(int16_t)(rc.h.w >> 16);
    const int np = w1 >> 1;
    const double2* v2 = reinterpret_cast<const double2*>(vals + p0);
    const double* xb = x + row0;
    const unsigned ul = (unsigned)lane;
    uint32_t d[PKD_CAP / 2] = {rc.d.s0, rc.d.s1, rc.d.s2, rc.d.s3, rc.d.s4, rc.d.s5, rc.d.s6, rc.d.s7};
    double acc = 0.0;
#pragma nounroll
    for (int j0 = 0; j0 < np; j0 += U) {
        double2 vv[U];
        double x0[U], x1[U];
#pragma unroll
        for (int j = 0; j < U; ++j) vv[j] = (j0 + j < np) ? (v2 + 64 * (j0 + j))[ul] : double2{0.0, 0.0};
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int lo = (int)(int16_t)(d[j] & 0xffffu), hi = (int)(int16_t)(d[j] >> 16);
            x0[j] = (j0 + j < np) ? ldx<SC1>((xb + lo) + ul) : 0.0;
            x1[j] = (j0 + j < np) ? ldx<SC1>((xb + hi) + ul) : 0.0;
        }
#pragma unroll
        for (int j = 0; j < U; ++j)
            if (j0 + j < np) {
                const int k = 2 * (j0 + j);
                if (k == kd) acc = diag(acc);
                acc += vv[j].x * x0[j];
                if (k + 1 == kd) acc = diag(acc);
                acc += vv[j].y * x1[j];
            }
#pragma unroll
        for (int i = 0; i + U < PKD_CAP / 2; ++i) d[i] = d[i + U];
    }
    if (w1 & 1) {
        const double xt = ldx<SC1>((xb + dtail) + ul);
        if (kd == w1 - 1) acc = diag(acc);
        acc += (vals + p0 + (int64_t)np * 128)[ul] * xt;
    }
    if (kd == w1) acc = diag(acc);
    return acc;
}

// uoff / ucol (nullable): the slice-uniform deltas of k_sell_uniform
template <int U, int SC1 = 0>
__device__ __forceinline__ double sell_row_pair(int64_t s, int lane, const int64_t* __restrict__ slice_ptr,
                                                const int16_t* __restrict__ cols, const double* __restrict__ vals,
                                                const double* __restrict__ x, int own_lo = 0, int own_hi = 0,
                                                const int32_t* __restrict__ uoff = nullptr,
                                                const int16_t* __restrict__ ucol = nullptr) {
    const int64_t p0 = slice_ptr[s];
    const int w = (int)((slice_ptr[s + 1] - p0) >> 6);
    const int base = (int)(s * 64 + lane);
    if (uoff) {
        const int uo = __builtin_amdgcn_readfirstlane(uoff[s]);
        if (uo >= 0) return sell_row_pair_body<U, SC1, true>(p0, w, base, lane, cols, ucol + uo, vals, x, own_lo, own_hi);
    }
    return sell_row_pair_body<U, SC1, false>(p0, w, base, lane, cols, nullptr, vals, x, own_lo, own_hi);
}

}  // namespace fem
