// Persistent PCG kernels: what they share outside the iteration itself -- the slot and LDS constants, the sync words,
// the bounded spins, the counter grid barrier (pk_barrier) and the reduction through tagged granules (pk_gran_*).
// A header of its own so that the bs = 3 and pipelined kernels and tools/probes/granule_reduce_probe.hip can use the
// same code.
#pragma once
#include "sell_pair.hpp"

namespace fem {

// PK_T / PK_WAVES (threads / waves per workgroup) and pk_slice_span live in sell_pair.hpp: the pattern pass that
// forms the gather windows (sl_pattern_slice) needs them outside this header
constexpr int PK_MAXS = 7;               // slices per wave (10M Poisson: 27,000 slices over 4,096 waves -> 7)
constexpr int PK_U = 2;                  // pairs in flight per lane (4 spills the slot state; persist_probe: 4 = 8)
// pairs in flight of a build: one slot per wave (small systems: every wave owns at most one slice, e.g. 1M tets or
// a rank's share at N = 8) leaves the registers for 8 pairs, so a slice's loads go out in one round instead of 4;
// up to four slots for 4 pairs (the instrumented builds keep PK_U there: their clock registers would spill)
template <int MAXS, bool PROF>
constexpr int pk_u() { return MAXS <= 1 ? 8 : (MAXS <= 4 && !PROF) ? 4 : PK_U; }
// pairs in flight of a record slot (DESC builds): the one-slot build takes 4 there, since its 8-pair round beside the
// 8-pair round of the slices read without a record spills into the SpMV (96 bytes of scratch per lane)
template <int MAXS, bool PROF>
constexpr int pk_u_rec() { return MAXS <= 1 ? 4 : pk_u<MAXS, PROF>(); }
constexpr int PK_LINE = 32;              // unsigned words per 128-byte line
// sync words (zeroed by fem_pcg_start; epochs continue across launches from PcgState::pk_epoch), in lines: [0, 8) group arrivals, 8 (unused), [9, 17) replicas of the
// top counter (one per group),
// 17 give-up word, 18 + L: u-flag of workgroup L
enum { PK_GRP = 0, PK_TOP = 8 * PK_LINE, PK_GEN = 9 * PK_LINE, PK_TMO = 17 * PK_LINE, PK_UFLAG = 18 * PK_LINE };
// every spin is bounded in TIME (s_memrealtime, 100 MHz on gfx9 parts: hipDeviceAttributeWallClockRate), checked
// every 64 polls: 2 s for a wait inside one GPU (the longest legitimate one is a grid barrier behind one ~50 us
// SpMV phase), 5 s for the rank exchange of the DIST build (ranks start their launches up to milliseconds apart).
// A give-up therefore costs at most ~5 s per launch whatever the poll latency (xGMI system-scope loads included);
// the spin-count bound this replaces scaled with that latency (4M polls: 4-50 s)
constexpr uint64_t PK_WAIT_TICKS = 200000000ull;
constexpr uint64_t PK_RANK_WAIT_TICKS = 500000000ull;
__device__ __forceinline__ uint64_t pk_now() { return __builtin_amdgcn_s_memrealtime(); }
__device__ __forceinline__ bool pk_expired(uint64_t t0, uint64_t ticks) { return pk_now() - t0 > ticks; }
constexpr int PK_NPROF = 8;   // phases: u wait, SpMV, block sum, barrier + sums, step, update + drain + flag,
                               // prologue (state loads), epilogue (chunk-end barrier + state stores)
// dynamic LDS (statics would shift the dynamic base off 16 B, cdna_hip_programming.md Guideline 17): 16 wave sums,
// the barrier verdict (own 16-byte slot), then x and w of the workgroup's rows
constexpr size_t PK_LDS_HEAD = 256;
constexpr int PK_VL = 5;                 // slots of v = A u kept in LDS (the rest in registers): fills the LDS left
                                         // by x and w, frees 2 PK_VL VGPRs for the SpMV (no spills at PK_U = 2)
constexpr size_t PK_LDS = PK_LDS_HEAD + sizeof(double) * (2 * PK_MAXS + PK_VL) * PK_WAVES * 64;
static_assert(PK_LDS <= 160 * 1024, "persistent PCG: LDS over the 160 KB of a CU");

// an opaque copy of a global pointer (the compiler cannot hoist address arithmetic on it out of the iteration loop)
// that keeps its address space: laundering a generic pointer turns every access through it into a FLAT access
// (lgkmcnt-coupled, and `flat_` sc1 loads are not a valid hand-off form, MI355X_MICROARCH.md)
template <class T>
__device__ __forceinline__ T* pk_launder(T* p) {
    __attribute__((address_space(1))) T* q = (__attribute__((address_space(1))) T*)p;
    asm volatile("" : "+s"(q));
    return (T*)q;
}

__device__ __forceinline__ unsigned pk_ld(const unsigned* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void pk_st(unsigned* p, unsigned v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one lane spins until *p >= target; false on give-up (own or another spinner's)
// the give-up word holds the site of the first give-up (diagnostics, reported by fem_pcg_sync_site for a
// FEM_PCG_SYNC_TIMEOUT): 1 + 16 * epoch local grid barrier, 2 + 16 * epoch u-flag window, 3 + 16 * epoch
// rank sums (DIST), 5 + 16 * epoch granule reduction (PK_SITE_GRAN), PK_SITE_WINDOW: a gather window outside the flag array (status FEM_PCG_BAD_WINDOW)
// (PK_SITE_WINDOW, pk_window_bad, pk_fail_status: common.hpp)
__device__ __forceinline__ bool pk_wait_ge(const unsigned* p, unsigned target, unsigned* tmo) {
    const uint64_t t0 = pk_now();
    for (unsigned spins = 0;; ++spins) {
        if (pk_ld(p) >= target) return true;
        if ((spins & 63) == 63 && pk_ld(tmo)) return false;
        if ((spins & 63) == 63 && pk_expired(t0, PK_WAIT_TICKS)) {
            pk_st(tmo, 1u + 16u * (target / NXCD));
            return false;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

// fixed-order sum of n sc1-loaded partials by one wave (identical result in every lane)
__device__ __forceinline__ double pk_sum(const double* part, int n) {
    const int lane = threadIdx.x & 63;
    double v = 0.0;
    for (int i = lane; i < n; i += 64) v += __hip_atomic_load(part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return wave_sum(v);
}

// grid barrier of epoch e over 8 groups of nper workgroups, then the fixed-order sums of the partial vectors pd
// (and pg when given) by wave 0 alone, handed to the other waves through LDS (out[0], out[1]). One wave per
// workgroup reads the G partials instead of all 16 (4,096 waves loading the same 4 KB with sc1 loads queue on the
// memory channels that hold those lines).
// entry_sync = false: the caller's own workgroup barrier (pk_block_sum's) already separates every wave's prior work
__device__ __forceinline__ bool pk_barrier(unsigned* sy, int grp, unsigned nper, unsigned e, int* lds_ok,
                                           const double* pd, const double* pg, int G, double* out,
                                           bool entry_sync = true) {
    if (entry_sync) __syncthreads();
    if (threadIdx.x < 64) {
        int okv = 0;
        if (threadIdx.x == 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            unsigned* tmo = sy + PK_TMO;
            bool ok;
            const unsigned old = __hip_atomic_fetch_add(sy + PK_GRP + grp * PK_LINE, 1u, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
            // last of its group: arrive on all 8 replicas of the top counter (one line each); every workgroup polls
            // its group's replica (32 pollers per line, no leader -> generation hop)
            if (old == e * nper - 1)
                for (int r = 0; r < NXCD; ++r)
                    __hip_atomic_fetch_add(sy + PK_GEN + r * PK_LINE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok = pk_wait_ge(sy + PK_GEN + grp * PK_LINE, e * NXCD, tmo);
            okv = ok ? 1 : 0;
        }
        okv = __builtin_amdgcn_readfirstlane(okv);
        if (okv && pd) {   // both partial vectors in one round of loads (same per-lane order as two pk_sums)
            const int lane = threadIdx.x & 63;
            double vd = 0.0, vg = 0.0;
            if (pg) {
#pragma unroll 4
                for (int i = lane; i < G; i += 64) {
                    const double a = __hip_atomic_load(pd + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const double b = __hip_atomic_load(pg + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    vd += a;
                    vg += b;
                }
            } else {
#pragma unroll 4
                for (int i = lane; i < G; i += 64) vd += __hip_atomic_load(pd + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const double d = wave_sum(vd);
            const double g = pg ? wave_sum(vg) : 0.0;
            if (threadIdx.x == 0) {
                out[0] = d;
                out[1] = g;
            }
        }
        if (threadIdx.x == 0) *lds_ok = okv;
    }
    __syncthreads();
    return *lds_ok != 0;
}

// fixed-order workgroup sum (PK_WAVES waves), valid in thread 0
__device__ __forceinline__ double pk_block_sum(double v, double* lds16) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds16[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < PK_WAVES; ++i) t += lds16[i];
    }
    return t;
}

// ---- the reduction through tagged granules (FEM_TUNE_PK_GRAN): "the data IS the flag" (cdna_hip_programming.md
// Guideline 16, form R2). Every workgroup keeps, per parity bank (epoch & 1), one record of four 8-byte granules
// d_lo, d_hi, g_lo, g_hi, each (epoch << 32) | one half of the double, each written by ONE aligned 8-byte relaxed
// agent-scope store and read by vector sc1 loads only. A reader re-reads a record until all its tags equal the epoch:
// no drain, no counter, no replica and no poll of a separate word stand between a partial and its sum, and a
// workgroup that holds every d record of epoch e also knows that every workgroup has finished SpMV(e), which is the
// barrier's second job (no update overwrites u while a neighbour still gathers it).
// Two banks suffice: a workgroup writes bank e & 1 again only in epoch e + 2 (d after SpMV(e + 2), g tagged e + 2 in
// update(e + 1)). Either needs it to have passed reduction e + 1, hence to have seen every workgroup's d record
// e + 1, and each of those was written after its owner finished reading epoch e. A reader never meets a tag past
// the one it waits for either (record e + 2 needs the reader's own record e + 1, written after its reduction e), so
// the test is equality. Tag 0 is never a valid epoch: the block is zeroed wherever the sync words are.
// Records are PK_GRAN_STRIDE granules apart and both d granules (both g granules) come from one 16-byte load
// (PK_GRAN_L16; layout and polling form: tools/probes/granule_reduce_probe.hip, profiles/granule_probe.json).
typedef unsigned long long pk_u64;
constexpr unsigned PK_SITE_GRAN = 5u;    // give-up site code of the granule reduction (5 + 16 * epoch)
constexpr int PK_GRAN_STRIDE = 4;        // 8-byte words per record: the four granules, contiguous (32 bytes)
// one 16-byte load per pair: with two 8-byte loads the 10M iteration ran 42.6 us against the counter barrier's
// 39.4, with 16-byte loads 37.7
constexpr bool PK_GRAN_L16 = true;
// between passes: a short sleep while at most PK_GRAN_NEAR lanes still miss a record (the end is near), a longer one
// (PK_GRAN_NAP x 64 clocks) while more do -- hundreds of waves re-reading the same few lines back to back hold up
// the stores they wait for
constexpr int PK_GRAN_NEAR = 8;
#define PK_GRAN_NAP 8
// 8-byte words of the granule block of a G-workgroup grid (two banks); a multiple of 16 bytes for every stride
constexpr size_t pk_gran_words(int G, int stride = PK_GRAN_STRIDE) { return (size_t)2 * G * stride; }

__device__ __forceinline__ void pk_gran_put(pk_u64* g, unsigned e, double v) {   // g: the lo granule of the pair
    const pk_u64 b = (pk_u64)__double_as_longlong(v), t = (pk_u64)e << 32;
    __hip_atomic_store(g, t | (b & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(g + 1, t | (b >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double pk_gran_val(pk_u64 lo, pk_u64 hi) {
    return __longlong_as_double((long long)((lo & 0xffffffffull) | (hi << 32)));
}
// one pair of granules (word i of the bank, 16-byte aligned) by two 8-byte loads or by one 16-byte buffer load (aux
// 16 = sc1, bit 31 = volatile: a poll, never to be hoisted out of its loop or merged with the pass before; the
// descriptor spans the bank's `bytes`), all sc1 vector loads
template <bool L16>
__device__ __forceinline__ void pk_gran_ld(const pk_u64* bank, size_t bytes, unsigned i, pk_u64& lo, pk_u64& hi) {
    if constexpr (L16) {
        typedef unsigned pk_v4u __attribute__((ext_vector_type(4)));
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)bank, 0, (int)bytes, 0x00027000);
        const pk_v4u r = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(i * sizeof(pk_u64)), 0, (int)0x80000010u);
        lo = (pk_u64)r.x | ((pk_u64)r.y << 32);
        hi = (pk_u64)r.z | ((pk_u64)r.w << 32);
    } else {
        lo = __hip_atomic_load(bank + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        hi = __hip_atomic_load(bank + i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One wave collects one granule pair per record (word `woff`: 0 d, 2 g) of epoch e from one bank (`bank`: its first
// record) and sums the values: lane l owns records l, l + 64, ... (pk_barrier's ownership), summed per lane in
// increasing record index, then wave_sum -- the operations and the order of pk_barrier's sums, so the bits are the
// same. Every pass loads all pairs still wanted before it tests any; MASKED: later passes reload only the records
// still missing (otherwise every owned record, until all match in one pass). One pair at a time keeps the loads in
// flight at pk_barrier's 16 registers (d and g together spilled the seven-slot builds): pk_gran_reduce gives the g
// pairs to a second wave.
// Bounded in time like every spin here; false on give-up. `moved` (COUNT, the probe's): bytes this lane's loads
// asked for.
template <int STRIDE, bool L16, bool MASKED, bool COUNT = false>
__device__ __forceinline__ bool pk_gran_sum(const pk_u64* bank, int G, unsigned e, int woff, unsigned* tmo, double* sum,
                                            unsigned long long* moved = nullptr) {
    const int lane = threadIdx.x & 63;
    const pk_u64 tag = e;
    const size_t bytes = (size_t)G * STRIDE * sizeof(pk_u64);
    double v = 0.0;
    bool ok = true;
    for (int base = 0; base < G && ok; base += 256) {   // (one round on a 256-CU part)
        pk_u64 w[4][2] = {};
        bool miss[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) miss[r] = base + lane + 64 * r < G;
        const uint64_t t0 = pk_now();
        for (unsigned spins = 0;; ++spins) {
            asm volatile("" ::: "memory");   // every pass reads memory anew (the buffer load is no atomic)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (miss[r]) {
                    pk_gran_ld<L16>(bank, bytes, (unsigned)((base + lane + 64 * r) * STRIDE + woff), w[r][0], w[r][1]);
                    if constexpr (COUNT) *moved += 16;
                }
            }
            bool any = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (miss[r]) {
                    const bool m = (w[r][0] >> 32) == tag && (w[r][1] >> 32) == tag;
                    if (MASKED) miss[r] = !m;
                    any = any || !m;
                }
            }
            const int nmiss = __popcll(__ballot(any));
            if (nmiss == 0) break;
            if ((spins & 63) == 63) {
                if (__builtin_amdgcn_readfirstlane(pk_ld(tmo))) ok = false;
                else if (pk_expired(t0, PK_WAIT_TICKS)) {
                    if (lane == 0) pk_st(tmo, PK_SITE_GRAN + 16u * e);
                    ok = false;
                }
                if (!ok) break;
            }
            if (nmiss > PK_GRAN_NEAR) __builtin_amdgcn_s_sleep(PK_GRAN_NAP);
            else __builtin_amdgcn_s_sleep(1);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (ok && base + lane + 64 * r < G) v += pk_gran_val(w[r][0], w[r][1]);
    }
    *sum = wave_sum(v);
    return ok;
}

// the calling wave collects the pairs at woff of epoch e from bank e & 1 of `gran` (every lane gets the sum)
__device__ __forceinline__ bool pk_gran_collect(const pk_u64* gran, unsigned* sy, unsigned e, int G, int woff,
                                                double* sum) {
    return pk_gran_sum<PK_GRAN_STRIDE, PK_GRAN_L16, true>(gran + (size_t)(e & 1u) * G * PK_GRAN_STRIDE, G, e, woff,
                                                          sy + PK_TMO, sum);
}
// pk_barrier's place in a build that reduces through granules. what = PKG_D: wave 0 collects the d pairs of epoch e
// -> out[0]; PKG_DG: also, beside it, the workgroup's last wave the g pairs -> out[1] (they were published a whole
// SpMV phase earlier, so that wave is done before wave 0 is; two waves with one pair each keep the loads in flight at
// pk_barrier's 16 registers); PKG_G (chunk end): wave 0 collects the g pairs -> out[0]. Handed to the other waves
// through LDS; verdicts in ok[0] (wave 0) and ok[PKG_OK2] (the last wave)
enum { PKG_D = 0, PKG_DG = 1, PKG_G = 2 };
constexpr int PKG_OK2 = 8;   // ints between the two verdict words (byte 128 and byte 160 of the LDS head)
__device__ __forceinline__ bool pk_gran_reduce(const pk_u64* gran, unsigned* sy, unsigned e, int* ok, int G, int what,
                                               double* out, bool entry_sync = true) {
    if (entry_sync) __syncthreads();
    const int wvx = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool second = what == PKG_DG && wvx == PK_WAVES - 1;
    if (wvx == 0 || second) {
        double sum;
        const bool okw = pk_gran_collect(gran, sy, e, G, (second || what == PKG_G) ? 2 : 0, &sum);
        if ((threadIdx.x & 63) == 0) {
            if (okw) out[second ? 1 : 0] = sum;
            ok[second ? PKG_OK2 : 0] = okw ? 1 : 0;
        }
    }
    __syncthreads();
    return ok[0] != 0 && (what != PKG_DG || ok[PKG_OK2] != 0);
}
// the granule pair at word woff (0: d, 2: g) of workgroup L's record of epoch e
__device__ __forceinline__ pk_u64* pk_gran_at(pk_u64* gran, int G, int L, unsigned e, int woff) {
    return gran + ((size_t)(e & 1u) * G + L) * PK_GRAN_STRIDE + woff;
}

}  // namespace fem
