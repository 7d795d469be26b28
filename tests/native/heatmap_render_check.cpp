// Host emulation of k_hm_render (echoglad_amd/csrc/heatmap_render.hip): the kernel's own source compiled for the CPU with stand-ins
// for the few HIP names it uses, every thread of every workgroup run in turn, on heap buffers of EXACTLY the documented sizes -- under
// AddressSanitizer + UndefinedBehaviorSanitizer an index past an end, a store across a frame's end or a misaligned dword store is
// an error.  The results are compared with a scalar evaluation of the header's arithmetic, bit for bit (both sides are this
// machine's fp32).  Nothing is launched; no library, no GPU.
//   clang++ -fsanitize=address,undefined -std=c++17 -ffp-contract=off -I <repo> tests/native/heatmap_render_check.cpp
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "include/echoglad_hip.h"

#define __global__
#define __device__
#define __launch_bounds__(x)
#define __restrict__
struct float4 { float x, y, z, w; };
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static dim3 blockIdx, threadIdx;
using std::min;
typedef void* hipStream_t;
namespace eg { static std::string last; inline int set_error(int code, const std::string& msg) { last = msg; return code; } }
#define EG_HIP_TRY(expr)
static long g_threads = 0;
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...)                       \
    for (unsigned b_ = 0; b_ < (grid).x; ++b_)                                          \
        for (unsigned t_ = 0; t_ < (block).x; ++t_) {                                   \
            blockIdx.x = b_; threadIdx.x = t_; ++g_threads;                             \
            kernel(__VA_ARGS__);                                                        \
        }
#define EG_HOST_EMULATION
#include "echoglad_amd/csrc/heatmap_render.hip"

static unsigned byte_of(float v) {
    const float s = v * 255.0f;
    if (!(s > 0.0f)) return 0;
    return s >= 255.0f ? 255u : (unsigned)(int)s;
}

static uint32_t rng_state = 1;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (float)(rng_state >> 8) / 16777216.0f; }

int main() {
    const float COL[4][3] = {{0, 1, 1}, {1, 0.7f, 0.9f}, {0, 1, 0}, {1, 0, 0}};
    const float NEG = -INFINITY;
    long wrong = 0, runs = 0, misaligned_frames = 0, partial_threads = 0;
    for (int side : {1, 2, 3, 5, 33, 64}) for (int count : {1, 3}) for (int start : {0, 21}) for (int behind : {0, 4}) for (int ch : {1, 4})
    for (int mask : {1, 2, 4, 8, 15}) {
        const int n = side * side;
        const long long n_rows = start + n + behind;
        rng_state = (uint32_t)(side * 131 + count * 7 + start + behind + ch + mask);
        std::vector<float> lg((size_t)count * n_rows * 4), lb((size_t)count * n_rows * 4), stats((size_t)count * 8);
        const size_t n_img = (size_t)(count - 1) * ch * n + n;              // the last frame ends with its channel 0
        float* img = (float*)malloc(sizeof(float) * n_img);
        for (auto& v : lg) v = (rnd() - 0.5f) * 12;
        for (auto& v : lb) v = rnd() < 0.2f ? rnd() : 0.f;
        for (size_t i = 0; i < n_img; ++i) img[i] = rnd() * 1.6f - 0.2f;     // below 0 and above 1.25 included
        for (int f = 0; f < count; ++f)
            for (int r = 0; r < n; ++r) {
                float* x = &lg[((size_t)f * n_rows + start + r) * 4];
                x[2] = NEG;                                                 // a channel without a finite logit
                if (r % 4 == 1) x[3] = NEG;
            }
        for (int f = 0; f < count; ++f)
            for (int c = 0; c < 4; ++c) {
                float M = NEG;
                double S = 0;
                for (int r = 0; r < n; ++r) M = std::max(M, lg[((size_t)f * n_rows + start + r) * 4 + c]);
                for (int r = 0; r < n; ++r) S += M == NEG ? 0.0 : (double)expf(lg[((size_t)f * n_rows + start + r) * 4 + c] - M);
                stats[f * 8 + 2 * c] = M;
                stats[f * 8 + 2 * c + 1] = (float)S;
            }
        float* heat = (mask & 1) ? (float*)aligned_alloc(16, sizeof(float) * 4 * (size_t)count * n) : nullptr;
        uint8_t* pred = (mask & 2) ? (uint8_t*)malloc((size_t)count * n * 3) : nullptr;
        uint8_t* gt = (mask & 4) ? (uint8_t*)malloc((size_t)count * n * 3) : nullptr;
        uint8_t* base = (mask & 8) ? (uint8_t*)malloc((size_t)count * n * 3) : nullptr;
        const int rc = eg_heatmap_render(lg.data(), (mask & 4) ? lb.data() : nullptr, img, (int64_t)ch * n, stats.data(), count, n_rows,
                                         start, side, heat, pred, gt, base, nullptr);
        ++runs;
        if (rc != EG_OK) { printf("rc %d: %s\n", rc, eg::last.c_str()); ++wrong; }
        if (mask == 15) {
            for (int f = 1; f < count; ++f) misaligned_frames += ((size_t)f * n * 3) % 4 != 0;
            partial_threads += (long)count * (n % 4 != 0);
        }
        for (int f = 0; f < count; ++f)
            for (int r = 0; r < n; ++r) {
                const float* x = &lg[((size_t)f * n_rows + start + r) * 4];
                const float* y = &lb[((size_t)f * n_rows + start + r) * 4];
                float e[4];
                for (int c = 0; c < 4; ++c) {
                    const float M = stats[f * 8 + 2 * c];
                    e[c] = M == NEG ? 0.f : expf(x[c] - M);
                    const float want = M == NEG ? 0.f : e[c] / stats[f * 8 + 2 * c + 1];
                    if (heat && heat[((size_t)f * n + r) * 4 + c] != want) ++wrong;
                }
                const float grey = std::max(0.f, 0.8f * img[(size_t)f * ch * n + r]);
                for (int k = 0; k < 3; ++k) {
                    float vp = grey, vg = grey;
                    for (int c = 0; c < 4; ++c) { vp = std::max(vp, COL[c][k] * e[c]); vg = std::max(vg, COL[c][k] * y[c]); }
                    const size_t o = ((size_t)f * n + r) * 3 + k;
                    if (pred && pred[o] != byte_of(vp)) ++wrong;
                    if (gt && gt[o] != byte_of(vg)) ++wrong;
                    if (base && base[o] != byte_of(grey)) ++wrong;
                }
            }
        free(img); free(heat); free(pred); free(gt); free(base);
    }
    // the refusals come before the launch: no thread runs
    const long before = g_threads;
    float dummy[8];
    int refused = 0;
    refused += eg_heatmap_render(nullptr, nullptr, nullptr, 0, dummy, 1, 4, 0, 2, dummy, nullptr, nullptr, nullptr, nullptr) == EG_ERR_ARG;
    refused += eg_heatmap_render(dummy, nullptr, nullptr, 0, dummy, 1, 3, 0, 2, nullptr, nullptr, nullptr, (uint8_t*)dummy, nullptr) == EG_ERR_ARG;
    refused += (g_threads == before);
    printf("heatmap_render_check: %ld runs, %ld values wrong, %ld misaligned frames, %ld partial groups, %d of 3 refusals\n", runs, wrong,
           misaligned_frames, partial_threads, refused);
    return (wrong == 0 && refused == 3 && misaligned_frames > 0 && partial_threads > 0) ? 0 : 1;
}
