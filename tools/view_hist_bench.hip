// The display histogram's hot-bin choices on gfx950 (developer tool): one pass over a 4096 x 4096 plane into 512 display bins held in
// LDS, with csrc/view_hist.hpp's view_hist_add<MODE> -- 0: one ds_add per lane; 1: the lanes that share the first lane's bin counted
// with a ballot, one instruction; 2: the same, two instructions -- with one copy of the bins per wave or one per workgroup, on a sky
// frame (background in two or three display bins) and on a plane spread evenly over all 512.  Mode -1 is the same loop without the
// histogram (the traffic floor of this grid), mode -2 computes every bin and adds nothing (the arithmetic's floor).
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/view_hist_bench.hip -o build/view_hist_bench
#include "../astroburst_amd/csrc/view_hist.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

constexpr int kBlock = 256, kBins = 512, kShift = 7;

template <int MODE, int COPIES>
__global__ __launch_bounds__(kBlock) void k(const float *__restrict__ src, long long quads, double dmin, double inv, unsigned int *__restrict__ out) {
    __shared__ unsigned int lds[kBins * 4];
    for (int i = threadIdx.x; i < kBins * COPIES; i += kBlock) lds[i] = 0;
    __syncthreads();
    unsigned int *mine = lds + (COPIES > 1 ? (threadIdx.x >> 6) * kBins : 0);
    unsigned int acc = 0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < quads; q += stride) {
        const float4 v4 = reinterpret_cast<const float4 *>(src)[q];
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool valid = __builtin_isfinite(v[j]) && v[j] > 1e-7f;
            if constexpr (MODE == -1) {
                acc += valid ? __float_as_uint(v[j]) : 0u;
            } else if constexpr (MODE == -2) {
                acc += valid ? view_bin(v[j], dmin, inv) >> kShift : 0u;
            } else {
                view_hist_add<(MODE < 0 ? 0 : MODE)>(mine, valid, view_bin(v[j], dmin, inv) >> kShift);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kBins; i += kBlock) {
        unsigned int s = 0;
        for (int c = 0; c < COPIES; ++c) s += lds[c * kBins + i];
        if (s) atomicAdd(&out[i], s);
    }
    if (acc == 0x12345678u) out[0] = acc;
}

template <int MODE, int COPIES>
static void run(const char *plane, const float *d, long long n, double dmin, double dmax, unsigned int *out, int grid) {
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    std::vector<float> ms;
    for (int rep = 0; rep < 13; ++rep) {
        hipMemsetAsync(out, 0, kBins * sizeof(unsigned int), 0);
        hipEventRecord(a, 0);
        hipLaunchKernelGGL((k<MODE, COPIES>), dim3(grid), dim3(kBlock), 0, 0, d, n / 4, dmin, 65536.0 / (dmax - dmin), out);
        hipEventRecord(b, 0);
        hipEventSynchronize(b);
        float t = 0.f;
        hipEventElapsedTime(&t, a, b);
        if (rep >= 3) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    unsigned int h[kBins];
    hipMemcpy(h, out, sizeof h, hipMemcpyDeviceToHost);
    unsigned long long total = 0;
    unsigned int top = 0;
    for (unsigned int v : h) total += v, top = std::max(top, v);
    printf("%-8s mode %2d copies %d   min %.4f ms  median %.4f ms  (%.0f GB/s at the median; counted %llu, fullest bin %u)\n", plane, MODE, COPIES,
           ms.front(), ms[ms.size() / 2], 4.0 * (double)n / ms[ms.size() / 2] / 1e6, total, top);
}

int main() {
    const long long n = 4096ll * 4096ll;
    std::vector<float> sky((size_t)n), flat((size_t)n);
    std::mt19937 rng(7);
    std::normal_distribution<float> noise(1000.f, 30.f);
    std::uniform_real_distribution<float> uni(0.f, 1.f);
    for (long long i = 0; i < n; ++i) {
        sky[(size_t)i] = noise(rng);
        if (uni(rng) < 1e-3f) sky[(size_t)i] += 60000.f * uni(rng);  // stars up to the full well: the background fills two or three of 512 bins
        flat[(size_t)i] = 1.f + 999.f * uni(rng);
    }
    float *d = nullptr;
    unsigned int *out = nullptr;
    hipMalloc(&d, (size_t)n * sizeof(float));
    hipMalloc(&out, kBins * sizeof(unsigned int));
    hipDeviceProp_t prop;
    hipGetDeviceProperties(&prop, 0);
    const int grid = prop.multiProcessorCount * 8;
    for (int which = 0; which < 2; ++which) {
        const std::vector<float> &p = which ? flat : sky;
        const char *name = which ? "spread" : "sky";
        const auto mm = std::minmax_element(p.begin(), p.end());
        const double lo = *mm.first, hi = *mm.second;
        hipMemcpy(d, p.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice);
        run<-1, 1>(name, d, n, lo, hi, out, grid);
        run<-2, 1>(name, d, n, lo, hi, out, grid);
        run<0, 4>(name, d, n, lo, hi, out, grid);
        run<1, 4>(name, d, n, lo, hi, out, grid);
        run<2, 4>(name, d, n, lo, hi, out, grid);
        run<0, 1>(name, d, n, lo, hi, out, grid);
        run<1, 1>(name, d, n, lo, hi, out, grid);
    }
    hipFree(d);
    hipFree(out);
    return 0;
}
