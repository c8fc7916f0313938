// Grid reduction of the persistent PCG, counter barrier against tagged granules (run on the GPU box; stand-alone):
// G workgroups of PK_T threads, one per CU (pinned by the kernel's LDS size). Per round every workgroup's thread 0
// sleeps a workgroup-dependent time, publishes its (d, g) partial, and wave 0 collects and sums all G of them.
//   counter      : pk_barrier as the kernel runs it (partials in a parity bank, group counters, replicas, poll, sums)
//   packed / line: tagged granules (pk_gran_sum), records 32 bytes apart / one 128-byte line per workgroup; full or
//                  masked re-poll; 8-byte loads or 16-byte loads of two granules. As in the kernel, wave 0 collects
//                  the d pairs after the publication and the last wave the g pairs (published a round earlier)
//                  before it
// Delays: "uniform" (every workgroup the same sleep) and "late" (four workgroups ~5 us behind the rest).
// Per variant and delay form, over the measured rounds: the time from the last publication to the last workgroup
// holding the sums, the last publisher's own wait, every workgroup's wait (mean, and the smallest per-workgroup
// mean), and the bytes the collecting loads asked for per round. Times: s_memrealtime (100 MHz, one clock for the
// chip) for what spans workgroups, s_memtime for a workgroup's own wait (scaled by the two clocks' ratio over the
// launch). Prints one JSON document; with a path argument also writes it there.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>
#include "../../cuda-powered-mesh-handling-and-iterative-solvers_amd/csrc/pcg_persist_sync.hpp"

using namespace fem;

struct ProbeArgs {
    unsigned* sync;
    double* part;               // counter variant: [2 banks][2][G]
    pk_u64* gran;               // granule variants: [2 banks][G][STRIDE]
    const int* delay;           // [G] sleeps of 512 clocks before publishing
    unsigned long long* tpub;   // [rounds][G] s_memrealtime at the publication
    unsigned long long* tdone;  // [rounds][G] s_memrealtime with the sums in hand
    unsigned long long* wait;   // [rounds][G] s_memtime between the two
    double* sums;               // [rounds][G] d + g as this workgroup summed them
    unsigned long long* moved;  // bytes the collecting loads asked for, all workgroups
    unsigned long long* clk;    // workgroup 0: s_memtime and s_memrealtime at start and end
    int rounds;
};

#define HIPCHECK(c)                                                                     \
    do {                                                                                \
        hipError_t e_ = (c);                                                            \
        if (e_ != hipSuccess) {                                                         \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));   \
            return 2;                                                                   \
        }                                                                               \
    } while (0)

template <int STRIDE, bool L16, bool MASKED, bool COUNTER>
__global__ void __launch_bounds__(PK_T) k_probe(ProbeArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    int* lds_ok = reinterpret_cast<int*>(lds + PK_WAVES);
    double* lds_dg = lds + PK_WAVES + 2;
    const int G = gridDim.x;
    const unsigned nper = (unsigned)(G / NXCD);
    const int L = (blockIdx.x % NXCD) * (G / NXCD) + blockIdx.x / NXCD;
    const int grp = L / (int)nper;
    unsigned long long moved = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.clk[0] = __builtin_amdgcn_s_memtime();
        a.clk[1] = pk_now();
    }
    const int nsleep = a.delay[L];
    double want_g0 = 0.0;   // round 0 has no g records (the kernel takes g from the state): the sum they would have
    for (int i = 0; i < G; ++i) want_g0 += 2.0 + 0.25 * i;
    for (int k = 0; k < a.rounds; ++k) {
        const unsigned e = (unsigned)k + 1;
        const double dv = 1.0 + 0.5 * L + k, gv = 2.0 + 0.25 * L + k;   // exact in any order of summation
        unsigned long long tp = 0, tm = 0;
        if (threadIdx.x == 0)
            for (int i = 0; i < nsleep; ++i) __builtin_amdgcn_s_sleep(8);
        __syncthreads();
        bool ok;
        if constexpr (COUNTER) {
            double* pd = a.part + (size_t)(k & 1) * 2 * G;
            if (threadIdx.x == 0) {
                tp = pk_now();
                tm = __builtin_amdgcn_s_memtime();
                __hip_atomic_store(pd + L, dv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(pd + G + L, gv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            ok = pk_barrier(a.sync, grp, nper, e, lds_ok, pd, pd + G, G, lds_dg, false);
        } else {
            pk_u64* bank = a.gran + (size_t)(e & 1u) * G * STRIDE;
            // as the kernel: g of epoch e + 1 goes out beside d of epoch e (the kernel's update publishes it a little
            // later) and is collected by the last wave before the publication; only d is collected after it
            pk_u64* nbank = a.gran + (size_t)((e + 1) & 1u) * G * STRIDE;
            if (k > 0 && threadIdx.x >= PK_T - 64) {
                double s1;
                const bool okg = pk_gran_sum<STRIDE, L16, MASKED, true>(bank, G, e, 2, a.sync + PK_TMO, &s1, &moved);
                if (threadIdx.x == PK_T - 64) {
                    lds_dg[1] = s1;
                    lds_ok[1] = okg ? 1 : 0;
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                tp = pk_now();
                tm = __builtin_amdgcn_s_memtime();
                pk_gran_put(bank + (size_t)L * STRIDE, e, dv);
                pk_gran_put(nbank + (size_t)L * STRIDE + 2, e + 1, gv + 1.0);
            }
            if (threadIdx.x < 64) {
                double s0;
                const bool okw = pk_gran_sum<STRIDE, L16, MASKED, true>(bank, G, e, 0, a.sync + PK_TMO, &s0, &moved);
                if (threadIdx.x == 0) {
                    lds_dg[0] = s0;
                    if (k == 0) lds_dg[1] = want_g0;
                    *lds_ok = okw ? 1 : 0;
                }
            }
            __syncthreads();
            ok = *lds_ok != 0 && (k == 0 || lds_ok[1] != 0);
        }
        if (!ok) break;
        if (threadIdx.x == 0) {
            const unsigned long long tm1 = __builtin_amdgcn_s_memtime(), td = pk_now();
            const size_t o = (size_t)k * G + L;
            a.tpub[o] = tp;
            a.tdone[o] = td;
            a.wait[o] = tm1 - tm;
            a.sums[o] = lds_dg[0] + lds_dg[1];
        }
    }
    if (threadIdx.x < 64 || threadIdx.x >= PK_T - 64) {   // the two collecting waves
        for (int o = 32; o > 0; o >>= 1) moved += __shfl_xor(moved, o, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(a.moved, moved);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.clk[2] = __builtin_amdgcn_s_memtime();
        a.clk[3] = pk_now();
    }
}

struct Variant {
    const char* name;
    void (*fn)(ProbeArgs);
    int stride;   // 8-byte words per record (0: counter)
};

static double mean(const std::vector<double>& v) {
    double s = 0;
    for (double x : v) s += x;
    return v.empty() ? 0.0 : s / v.size();
}
static double median(std::vector<double> v) {
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char** argv) {
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, 0));
    const int G = (prop.multiProcessorCount / NXCD) * NXCD;
    const int rounds = 400, warm = 50;
    const Variant vars[] = {
        {"counter", k_probe<4, false, false, true>, 0},
        {"packed_full_8", k_probe<4, false, false, false>, 4},
        {"packed_masked_8", k_probe<4, false, true, false>, 4},
        {"packed_full_16", k_probe<4, true, false, false>, 4},
        {"packed_masked_16", k_probe<4, true, true, false>, 4},
        {"line_full_8", k_probe<16, false, false, false>, 16},
        {"line_masked_8", k_probe<16, false, true, false>, 16},
        {"line_full_16", k_probe<16, true, false, false>, 16},
        {"line_masked_16", k_probe<16, true, true, false>, 16},
    };
    const size_t sync_words = (size_t)(18 + G) * PK_LINE, gran_words = pk_gran_words(G, 16), rg = (size_t)rounds * G;
    ProbeArgs a{};
    int* delay;
    HIPCHECK(hipMalloc(&a.sync, sizeof(unsigned) * sync_words));
    HIPCHECK(hipMalloc(&a.part, sizeof(double) * 4 * G));
    HIPCHECK(hipMalloc(&a.gran, sizeof(pk_u64) * gran_words));
    HIPCHECK(hipMalloc(&delay, sizeof(int) * G));
    HIPCHECK(hipMalloc(&a.tpub, 8 * rg));
    HIPCHECK(hipMalloc(&a.tdone, 8 * rg));
    HIPCHECK(hipMalloc(&a.wait, 8 * rg));
    HIPCHECK(hipMalloc(&a.sums, 8 * rg));
    HIPCHECK(hipMalloc(&a.moved, 8));
    HIPCHECK(hipMalloc(&a.clk, 32));
    a.delay = delay;
    for (const Variant& v : vars) {
        HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(v.fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)PK_LDS));
        int nb = 0;
        HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, v.fn, PK_T, PK_LDS));
        if (nb != 1) {
            fprintf(stderr, "%s: %d workgroups per CU, want 1\n", v.name, nb);
            return 2;
        }
    }
    std::string js = "{\"device\": \"" + std::string(prop.gcnArchName) + "\", \"G\": " + std::to_string(G) +
                     ", \"rounds\": " + std::to_string(rounds - warm) + ", \"results\": [";
    bool first = true, bad = false;
    for (int mode = 0; mode < 2 && !bad; ++mode) {
        std::vector<int> hd(G, 4);   // ~1 us
        if (mode == 1)
            for (int L : {37, 101, 170, 233})
                if (L < G) hd[L] = 28;   // ~5 us behind
        HIPCHECK(hipMemcpy(delay, hd.data(), sizeof(int) * G, hipMemcpyHostToDevice));
        for (const Variant& v : vars) {
            HIPCHECK(hipMemset(a.sync, 0, sizeof(unsigned) * sync_words));
            HIPCHECK(hipMemset(a.part, 0, sizeof(double) * 4 * G));
            HIPCHECK(hipMemset(a.gran, 0, sizeof(pk_u64) * gran_words));
            HIPCHECK(hipMemset(a.moved, 0, 8));
            HIPCHECK(hipMemset(a.tdone, 0, 8 * rg));
            a.rounds = rounds;
            hipLaunchKernelGGL(v.fn, dim3(G), dim3(PK_T), PK_LDS, 0, a);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipDeviceSynchronize());
            std::vector<unsigned long long> tp(rg), td(rg), tw(rg);
            std::vector<double> sm(rg);
            unsigned long long moved = 0, clk[4];
            unsigned tmo = 0;
            HIPCHECK(hipMemcpy(tp.data(), a.tpub, 8 * rg, hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(td.data(), a.tdone, 8 * rg, hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(tw.data(), a.wait, 8 * rg, hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(sm.data(), a.sums, 8 * rg, hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(&moved, a.moved, 8, hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(clk, a.clk, 32, hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(&tmo, a.sync + PK_TMO, 4, hipMemcpyDeviceToHost));
            if (tmo) {
                fprintf(stderr, "%s: gave up, site %u\n", v.name, tmo);
                bad = true;   // nothing more runs on the device after a give-up
                break;
            }
            const double us_rt = 0.01;   // s_memrealtime: 100 MHz
            const double us_mt = clk[2] > clk[0] ? us_rt * (double)(clk[3] - clk[1]) / (double)(clk[2] - clk[0]) : us_rt;
            std::vector<double> lat, lastw, allw, wgw(G, 0.0);
            int wrong = 0;
            for (int k = warm; k < rounds; ++k) {
                unsigned long long pmax = 0, dmax = 0;
                int who = 0;
                double want = 0.0;
                for (int L = 0; L < G; ++L) want += (1.0 + 0.5 * L + k) + (2.0 + 0.25 * L + k);
                for (int L = 0; L < G; ++L) {
                    const size_t o = (size_t)k * G + L;
                    if (tp[o] > pmax) pmax = tp[o], who = L;
                    dmax = std::max(dmax, td[o]);
                    const double w = us_mt * (double)tw[o];
                    allw.push_back(w);
                    wgw[L] += w / (rounds - warm);
                    if (sm[o] != want) ++wrong;
                }
                lat.push_back(us_rt * (double)(dmax - pmax));
                lastw.push_back(us_rt * (double)(td[(size_t)k * G + who] - pmax));
            }
            const double bytes = v.stride ? (double)moved / rounds : (double)G * G * 16;   // counter: the partial loads
            char buf[640];
            snprintf(buf, sizeof buf,
                     "%s\n  {\"variant\": \"%s\", \"delay\": \"%s\", \"last_pub_to_last_sum_us\": {\"mean\": %.3f, "
                     "\"median\": %.3f, \"min\": %.3f}, \"last_publisher_wait_us\": {\"mean\": %.3f, \"median\": %.3f}, "
                     "\"wg_wait_us\": {\"mean\": %.3f, \"min_wg_mean\": %.3f, \"max_wg_mean\": %.3f}, "
                     "\"poll_bytes_per_round\": %.0f, \"wrong_sums\": %d}",
                     first ? "" : ",", v.name, mode ? "late" : "uniform", mean(lat), median(lat),
                     *std::min_element(lat.begin(), lat.end()), mean(lastw), median(lastw), mean(allw),
                     *std::min_element(wgw.begin(), wgw.end()), *std::max_element(wgw.begin(), wgw.end()), bytes, wrong);
            js += buf;
            first = false;
            if (wrong) bad = true;
        }
    }
    js += "\n]}\n";
    fputs(js.c_str(), stdout);
    if (argc > 1) {
        FILE* f = fopen(argv[1], "w");
        if (!f) return 2;
        fputs(js.c_str(), f);
        fclose(f);
    }
    return bad ? 1 : 0;
}
