// The landmark evaluator's pictures of one level, on the device (gfx950): the softmax heat map and the overlay images.
// Replaces, without moving the logits to the host:
//   src/core/evaluators.py:485-495  get_softmaxed_heatmap (softmax over the main grid's rows)
//   src/core/evaluators.py:510-515  the per-channel normalisation p / max p and the two overlays of get_heatmaps
//   src/core/evaluators.py:595-616  create_overlay_image + torchvision's ToPILImage (mul(255).byte(), HWC)
// The softmax statistics (M, S) per frame and channel come from eg_heatmap_expect_fwd's `stats`; p / max p is exp(x - M)
// (max p = exp(M - M) / S = 1 / S), so no second reduction is needed and the whole figure is ONE elementwise launch.
//
// One thread owns HR_PIX consecutive pixels of one frame: one float4 load per pixel serves the 4 channels of the logits, one
// those of the labels; the 3 * HR_PIX RGB bytes leave as three dword stores where the address is 4-byte aligned.  A frame
// holds side * side * 3 bytes, no multiple of 4 for an odd side: frames after the first may start misaligned, and the frame's
// last thread may own fewer than HR_PIX pixels -- both take byte stores, and only of the pixels the thread owns (never past
// the frame's end).  About 3 MB per frame at 224: bandwidth is trivial, the edges are the work.
#ifndef EG_HOST_EMULATION          // (tests/native/heatmap_render_check.cpp compiles this file for the host, with its own stand-ins)
#include "common.h"
#endif

namespace eg {

constexpr int HR_THREADS = 256;
constexpr int HR_PIX = 4;           // consecutive pixels per thread: 12 RGB bytes = 3 dwords

// channel colours of create_overlay_image (evaluators.py:608)
__device__ constexpr float HR_COL[4][3] = {{0.f, 1.f, 1.f}, {1.f, 0.7f, 0.9f}, {0.f, 1.f, 0.f}, {1.f, 0.f, 0.f}};

// ToPILImage's mul(255).byte() with saturation: truncated toward zero, 255 and above -> 255, NaN (and anything <= 0) -> 0
__device__ inline unsigned hr_byte(float v) {
    const float s = v * 255.0f;
    return s >= 255.0f ? 255u : (s > 0.0f ? (unsigned)(int)s : 0u);
}

// the thread's 3 * np bytes at d: dwords where all HR_PIX pixels are there and d is 4-byte aligned, else bytes
__device__ inline void hr_store_rgb(uint8_t* __restrict__ d, const unsigned (&b)[3 * HR_PIX], int np) {
    if (np == HR_PIX && ((uintptr_t)d & 3) == 0) {
        uint32_t* q = reinterpret_cast<uint32_t*>(d);
#pragma unroll
        for (int k = 0; k < 3 * HR_PIX / 4; ++k) q[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 3 * HR_PIX; ++k)
            if (k < 3 * np) d[k] = (uint8_t)b[k];
    }
}

struct HrArgs {
    const float *logits, *labels, *image, *stats;
    long long image_stride, n_rows;
    int level_start, n_pix, blocks_per_frame;
    float* heat;
    uint8_t *pred, *gt, *base;
};

__global__ __launch_bounds__(HR_THREADS) void k_hm_render(const HrArgs a) {
#pragma clang fp contract(off)
    const int frame = (int)(blockIdx.x / (unsigned)a.blocks_per_frame);
    const int blk = (int)(blockIdx.x - (unsigned)frame * (unsigned)a.blocks_per_frame);
    const long long p0 = ((long long)blk * HR_THREADS + threadIdx.x) * HR_PIX;
    if (p0 >= a.n_pix) return;
    const int np = (int)min((long long)HR_PIX, (long long)a.n_pix - p0);
    // (M, S) of the frame's 4 channels: one address per workgroup, so these are scalar loads into scalar registers
    const float* st = a.stats + (size_t)frame * 8;
    const float M[4] = {st[0], st[2], st[4], st[6]}, S[4] = {st[1], st[3], st[5], st[7]};
    const float NEG = -__builtin_inff();
    const size_t row0 = (size_t)frame * (size_t)a.n_rows + (size_t)a.level_start + (size_t)p0;
    const size_t pix0 = (size_t)frame * (size_t)a.n_pix + (size_t)p0;
    const bool want_e = a.heat || a.pred;

    // every load in front of the first use; a pixel the thread does not own reads the thread's first pixel instead
    float4 xs[HR_PIX], ys[HR_PIX];
    float im[HR_PIX];
#pragma unroll
    for (int k = 0; k < HR_PIX; ++k) {
        const int kk = k < np ? k : 0;
        xs[k] = want_e ? *reinterpret_cast<const float4*>(a.logits + (row0 + kk) * 4) : float4{0.f, 0.f, 0.f, 0.f};
        ys[k] = a.gt ? *reinterpret_cast<const float4*>(a.labels + (row0 + kk) * 4) : float4{0.f, 0.f, 0.f, 0.f};
        im[k] = a.image ? a.image[(long long)frame * a.image_stride + p0 + kk] : 0.f;
    }

    unsigned bp[3 * HR_PIX], bg[3 * HR_PIX], bb[3 * HR_PIX];
#pragma unroll
    for (int k = 0; k < HR_PIX; ++k) {
        const float xv[4] = {xs[k].x, xs[k].y, xs[k].z, xs[k].w}, yv[4] = {ys[k].x, ys[k].y, ys[k].z, ys[k].w};
        float e[4], p[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            // (a channel without a finite logit has M = -inf: -inf - -inf is NaN and S is 0 -- it holds no mass, the map is 0)
            e[c] = M[c] == NEG ? 0.f : expf(xv[c] - M[c]);
            p[c] = M[c] == NEG ? 0.f : e[c] / S[c];
        }
        if (a.heat && k < np) *reinterpret_cast<float4*>(a.heat + (pix0 + k) * 4) = float4{p[0], p[1], p[2], p[3]};
        const float base = fmaxf(0.f, 0.8f * im[k]);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float vp = base, vg = base;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                vp = fmaxf(vp, HR_COL[c][j] * e[c]);
                vg = fmaxf(vg, HR_COL[c][j] * yv[c]);
            }
            bp[3 * k + j] = hr_byte(vp);
            bg[3 * k + j] = hr_byte(vg);
            bb[3 * k + j] = hr_byte(base);
        }
    }
    if (a.pred) hr_store_rgb(a.pred + pix0 * 3, bp, np);
    if (a.gt) hr_store_rgb(a.gt + pix0 * 3, bg, np);
    if (a.base) hr_store_rgb(a.base + pix0 * 3, bb, np);
}

}  // namespace eg

using namespace eg;

extern "C" {

int eg_heatmap_render(const float* logits, const float* labels, const float* image, int64_t image_stride, const float* stats,
                      int count, int64_t n_rows, int level_start, int side, float* heat, uint8_t* pred_rgb, uint8_t* gt_rgb,
                      uint8_t* base_rgb, eg_stream_t stream) {
    if (!logits || !stats) return set_error(EG_ERR_ARG, "logits and stats must not be NULL");
    if (!heat && !pred_rgb && !gt_rgb && !base_rgb) return set_error(EG_ERR_ARG, "no output requested");
    if (gt_rgb && !labels) return set_error(EG_ERR_ARG, "gt_rgb needs labels");
    if (((uintptr_t)logits | (uintptr_t)labels | (uintptr_t)heat) & 15) return set_error(EG_ERR_ARG, "logits / labels / heat must be 16-byte aligned");
    if (count < 1 || side < 1 || level_start < 0) return set_error(EG_ERR_ARG, "count and side must be >= 1, level_start >= 0");
    const long long n_pix = (long long)side * side;
    if ((long long)level_start + n_pix > (long long)n_rows) return set_error(EG_ERR_ARG, "level outside the frame's rows");
    if (image && image_stride < n_pix) return set_error(EG_ERR_ARG, "image_stride is smaller than a frame of the level");
    const long long bpf = ((n_pix + HR_PIX - 1) / HR_PIX + HR_THREADS - 1) / HR_THREADS;
    if ((long long)count * (long long)n_rows >= (1ll << 31) || bpf * count >= (1ll << 31)) return set_error(EG_ERR_ARG, "count * rows exceeds int32");
    const HrArgs a{logits, labels, image, stats, (long long)image_stride, (long long)n_rows, level_start, (int)n_pix, (int)bpf,
                   heat, pred_rgb, gt_rgb, base_rgb};
    hipLaunchKernelGGL(k_hm_render, dim3((unsigned)(bpf * count)), dim3(HR_THREADS), 0, (hipStream_t)stream, a);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

}  // extern "C"
