// Stamp harness for conv_pool_mm alone (C2 shape): per-wave phase cycles and SIMD placement of the
// filter-bank waves, and the phases of BatchNorm1's auxiliary workgroups (cpm_bn1) beside them.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/cpm_stamp.hip -o tools/_bin/cpm_stamp
// (-DCPM_SRC='"path/convpool.hip"' stamps another copy of the kernel file, e.g. an older revision's)
#define EXPLAINN_STAMP 1
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdarg.h>
#include <algorithm>
#include <map>
#include <vector>
// (the shader-clock counters of different XCDs are not aligned: differences are meaningful within a
// wave only -- "kernel span" and "start skew" mix waves and are not; times across waves come from the
// wall clock)
// per wave: [0..5] shader-clock stamps, [8] / [9] the 100 MHz wall clock at stamps 0 / 5, [10] placement
#define SLOTS 16
__device__ unsigned long long g_stamps[1 << 20];
void explainn_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); printf("\n"); }
#include "../explainn_amd/csrc/common.h"
#undef STAMP
#define STAMP(i)                                                                                  \
    do {                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();                               \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        if ((threadIdx.x & 63) == 0) {                                                            \
            const size_t s_ = ((size_t)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) * (blockDim.x / 64) + threadIdx.x / 64) * SLOTS; \
            g_stamps[s_ + (i)] = t_;                                                              \
            if ((i) == 0) g_stamps[s_ + 8] = __builtin_amdgcn_s_memrealtime();                       \
            if ((i) == 5) g_stamps[s_ + 9] = __builtin_amdgcn_s_memrealtime();                       \
            if ((i) == 0) g_stamps[s_ + 10] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | \
                                              ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32); \
        }                                                                                         \
    } while (0)
#ifndef CPM_SRC
#define CPM_SRC "../explainn_amd/csrc/convpool.hip"
#endif
#include CPM_SRC
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

static void pcts(const char* name, std::vector<double>& d) {
    std::sort(d.begin(), d.end());
    if (!d.empty()) printf("  %-14s p10 %.0f p50 %.0f p90 %.0f max %.0f\n", name, d[d.size() / 10], d[d.size() / 2], d[d.size() * 9 / 10], d.back());
}

// naux > 0: the launch carries BatchNorm1's workgroups (IDX forms only), as launch_conv_pool_train does
template <int UT, bool IDX> static void run(int parts, int naux) {
    const int U = 300, U4 = 300, k = 19, L = 200, n = 26, B = 1024, Bs = 1088, NW = (L + 31) / 32 + 2, PW = 2 * NW, KS = 5;
    const int K4 = 4 * k, NT = (B + 63) / 64, Lp = ((NW * 32 + 63) / 64) * 64;
    auto dalloc = [](size_t bytes) { void* p; CK(hipMalloc(&p, bytes)); CK(hipMemset(p, 0, bytes)); return p; };
    const int tiles = conv_tiles_padded(U, k);
    uint32_t* pk2 = (uint32_t*)dalloc((size_t)PW * Bs * 4); uint32_t* nm = (uint32_t*)dalloc((size_t)NW * Bs * 4);
    std::vector<uint32_t> hp((size_t)PW * Bs); for (auto& v : hp) v = (uint32_t)rand() * 2654435761u;
    CK(hipMemcpy(pk2, hp.data(), hp.size() * 4, hipMemcpyHostToDevice));
    cu32x4* Wf = (cu32x4*)dalloc((size_t)tiles * KS * 3 * 1024);
    std::vector<uint16_t> hw((size_t)tiles * KS * 3 * 512); for (auto& v : hw) v = (uint16_t)(0x3c00 + (rand() & 0xff));
    CK(hipMemcpy(Wf, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
    cu32x4* g1 = (cu32x4*)dalloc((size_t)tiles * 32 * 4); float* ext = (float*)dalloc(((size_t)32 * tiles * n * Bs + 64 + 64 * 8192) * 4); uint8_t* idx = (uint8_t*)dalloc((size_t)32 * tiles * n * Bs + 64 + 64 * 8192);
    // BatchNorm1's side: real bit masks of a random one-hot batch (bm[a][tile][position], bit = sequence)
    cpm_bn1_args bn1 = {};
    if (naux > 0) {
        std::vector<unsigned long long> hb((size_t)4 * (Bs / 64) * Lp, 0ull);
        for (int t = 0; t < NT; ++t)
            for (int q = 0; q < L; ++q)
                for (int b = 0; b < 64 && 64 * t + b < B; ++b) hb[((size_t)(rand() & 3) * NT + t) * Lp + q] |= 1ull << b;
        unsigned long long* bm = (unsigned long long*)dalloc(hb.size() * 8);
        CK(hipMemcpy(bm, hb.data(), hb.size() * 8, hipMemcpyHostToDevice));
        auto fl = [&](size_t cnt, float lo, float hi) {
            std::vector<float> h(cnt); for (auto& v : h) v = lo + (hi - lo) * (float)(rand() & 0xffff) / 65535.f;
            float* p = (float*)dalloc(cnt * 4); CK(hipMemcpy(p, h.data(), cnt * 4, hipMemcpyHostToDevice)); return p;
        };
        bn1.bm = bm; bn1.G = (double*)dalloc((size_t)K4 * K4 * 8); bn1.m = (double*)dalloc((size_t)K4 * 8);
        bn1.conv_w = fl((size_t)U * K4, -0.5f, 0.5f); bn1.conv_b = fl(U4, -0.1f, 0.1f); bn1.g1 = fl(U4, 0.6f, 1.4f); bn1.b1 = fl(U4, -0.1f, 0.1f);
        bn1.rm = fl(U4, -0.5f, 0.5f); bn1.rv = fl(U4, 0.5f, 2.f); bn1.nbt = (int64_t*)dalloc(8);
        bn1.alpha = (float*)dalloc((size_t)U4 * 4); bn1.shift = (float*)dalloc((size_t)U4 * 4);
        bn1.mug = (double*)dalloc((size_t)U4 * 8); bn1.sig1 = (double*)dalloc((size_t)U4 * 8); bn1.Gw = (double*)dalloc((size_t)U4 * K4 * 8);
        bn1.ticket = (int*)dalloc(256); bn1.flags = (int*)dalloc(256);
        bn1.naux = naux; bn1.U = U; bn1.U4 = U4; bn1.k = k; bn1.B = B; bn1.L = L; bn1.Lp = Lp;
    }
    const int wper = (n + parts - 1) / parts;
    dim3 grid((B + 31) / 32, UT == 1 ? (U + 31) / 32 : tiles / UT, (n + wper - 1) / wper);
    const int slice = (int)(grid.x * grid.y);
    bn1.nz = (naux + slice - 1) / slice;
    grid.z += bn1.nz;
    const int waves = grid.x * grid.y * grid.z, first_fb = bn1.nz * slice;      // ids below first_fb: the auxiliary slices
    if ((size_t)waves * SLOTS > ((size_t)1 << 20)) { printf("grid too large for the stamp buffer\n"); exit(1); }
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1)); float ms = 0;
    void* sp = nullptr; CK(hipGetSymbolAddress(&sp, HIP_SYMBOL(g_stamps)));
    std::vector<double> evs;
    for (int rep = 0; rep < 30; ++rep) {
        CK(hipMemset(sp, 0, sizeof(unsigned long long) << 20));
        if (naux > 0) CK(hipMemset(bn1.ticket, 0, 4));
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL((conv_pool_mm_kernel<5, UT, IDX>), grid, dim3(64), 0, 0, pk2, nm, Wf, g1, ext, idx, n, Bs, PW, NW, wper, bn1);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep >= 10) evs.push_back(ms * 1e3);
    }
    std::sort(evs.begin(), evs.end());
    std::vector<unsigned long long> h((size_t)waves * SLOTS);
    CK(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_stamps), h.size() * 8));
    printf("UT=%d IDX=%d parts=%d (wper %d) naux=%d: %d workgroups, event last %.1f us, median of 20 %.1f us\n", UT, (int)IDX, parts, wper, naux, waves, ms * 1e3, evs[evs.size() / 2]);
    auto S = [&](int w, int i) { return h[(size_t)w * SLOTS + i]; };
    unsigned long long tmin = ~0ull, tmax = 0, rmin = ~0ull;
    for (int w = 0; w < waves; ++w) { if (S(w, 0)) { tmin = std::min(tmin, S(w, 0)); rmin = std::min(rmin, S(w, 8)); } tmax = std::max(tmax, S(w, 5)); }
    printf("  kernel span (first stamp 0 -> last stamp 5): %.0f cyc\n", (double)(tmax - tmin));
    const char* ph[5] = {"table", "prologue", "first window", "other windows", "drain"};
    for (int p = 1; p <= 5; ++p) {
        std::vector<double> d;
        for (int w = first_fb; w < waves; ++w) if (S(w, p) && S(w, p - 1)) d.push_back((double)(S(w, p) - S(w, p - 1)));
        pcts(ph[p - 1], d);
    }
    {
        std::vector<double> mhz;
        for (int w = first_fb; w < waves; ++w) if (S(w, 9) > S(w, 8) && S(w, 5) > S(w, 0)) mhz.push_back(100.0 * (double)(S(w, 5) - S(w, 0)) / (double)(S(w, 9) - S(w, 8)));
        std::sort(mhz.begin(), mhz.end());
        if (!mhz.empty()) printf("  shader clock over the wave's life: p10 %.0f p50 %.0f p90 %.0f MHz\n", mhz[mhz.size() / 10], mhz[mhz.size() / 2], mhz[mhz.size() * 9 / 10]);
    }
    std::map<unsigned, int> simd; std::vector<double> skew, tot;
    for (int w = first_fb; w < waves; ++w) {
        const unsigned long long id = S(w, 10); const unsigned hw_ = (unsigned)id, xcc = (unsigned)(id >> 32) & 15;
        simd[(xcc << 16) | (((hw_ >> 13) & 7) << 12) | (((hw_ >> 8) & 15) << 4) | ((hw_ >> 4) & 3)]++;
        skew.push_back((double)(S(w, 0) - tmin)); tot.push_back((double)(S(w, 5) - S(w, 0)));
    }
    std::sort(skew.begin(), skew.end()); std::sort(tot.begin(), tot.end());
    std::map<int, int> hist; for (auto& kv : simd) hist[kv.second]++;
    printf("  SIMDs used %zu; waves per SIMD histogram:", simd.size()); for (auto& kv : hist) printf(" %d:%d", kv.first, kv.second);
    printf("\n  start skew p50 %.0f p90 %.0f max %.0f; wave total p50 %.0f max %.0f\n", skew[skew.size() / 2], skew[skew.size() * 9 / 10], skew.back(), tot[tot.size() / 2], tot.back());
    if (naux > 0) {
        // the auxiliary workgroups: stamps 0 entry, 1 phase 1 drained, 2 ticket complete, 3 acquired, 4 G passes done, 5 end
        const char* ax[5] = {"phase 1", "ticket wait", "acquire", "G passes", "sums + finish"};
        printf("  auxiliary workgroups (cycles of each one's own clock):\n");
        for (int p = 1; p <= 5; ++p) {
            std::vector<double> d;
            for (int w = 0; w < naux; ++w) if (S(w, p) && S(w, p - 1)) d.push_back((double)(S(w, p) - S(w, p - 1)));
            printf("  "); pcts(ax[p - 1], d);
        }
        std::vector<double> at;
        for (int w = 0; w < naux; ++w) if (S(w, 5) && S(w, 0)) at.push_back((double)(S(w, 5) - S(w, 0)));
        printf("  "); pcts("whole chain", at);
        // who ends last, on the wall clock the XCDs share (100 MHz: 0.01 us steps) from the launch's first stamp
        unsigned long long a_end = 0, f_end = 0, a_start = 0;
        int missing = 0;
        for (int w = 0; w < naux; ++w) { a_end = std::max(a_end, S(w, 9)); a_start = std::max(a_start, S(w, 8)); if (!S(w, 5)) ++missing; }
        for (int w = first_fb; w < waves; ++w) f_end = std::max(f_end, S(w, 9));
        printf("  last auxiliary workgroup starts at %.2f us, ends at %.2f us; last filter-bank wave ends at %.2f us (%d auxiliary without an end stamp)\n",
               (double)(a_start - rmin) / 100.0, (double)(a_end - rmin) / 100.0, (double)(f_end - rmin) / 100.0, missing);
        int flags = 0; CK(hipMemcpy(&flags, bn1.flags, 4, hipMemcpyDeviceToHost));
        printf("  flags word %d\n", flags);
    }
}
int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    run<2, true>(6, 152); run<2, true>(6, 0); run<2, false>(6, 0);
    return 0;
}
