// Frame preparation on the device: what the reference's datasets do per sample on the host between "a uint8 frame was read" and
// "g.x / coords exist" (src/core/datasets.py: frame.float().div(255), UICLVLandmark.transform_image :317-349 = affine_grid +
// grid_sample(bilinear, zeros, align_corners=False), dataset_builder's Resize((F, F)) / Grayscale, hflip with probability flip_p, and
// the landmarks through the same matrix, :232-236) -- ONE launch for a batch.
//
// Rules: include/echoglad_hip.h, eg_frame_prep.  The warped image (608^2 in the reference) is never materialised: an output pixel is
// the 2 x 2 blend of the non-antialiased bilinear resize, each of its four operands the 2 x 2 blend of grid_sample, 4 x 4 source
// taps per channel.  One thread owns one output pixel: it computes the sixteen tap positions and weights once and applies them to
// every channel.  Positions are computed in fp64 (a handful of operations per pixel against 16 C gathers: the rounding of a source
// coordinate in fp32, ~6e-5 of a pixel at 640, is what dominates the error of an all-fp32 route), weights and blends are fp32.
// Consecutive lanes own consecutive pixels of an output row, so the stores are coalesced (a flip only reverses them) and a
// workgroup's taps fall on four or five source rows: byte gathers that rest on L2.  Every output element is written once; no
// atomics, no allocation, no synchronisation with the host.
//
// The landmarks (8 numbers per frame) are transformed by the first wave of the first workgroup, in fp64.
#include <climits>

#include "common.h"

namespace eg {

constexpr int FP_THREADS = 256;
constexpr int FP_MAX_SIDE = 32768;          // sides up to here: a frame's pixel index fits an int

struct FpDims {
    int channels, src_h, src_w;             // C, Hs, Ws
    int warp, frame;                        // W (0: no warp stage), F
    int mid_h, mid_w;                       // sides of the image the resize reads: W, W with a warp stage, else Hs, Ws
    int gray;
    unsigned blocks_per_frame;
    double inv_warp;                        // 1 / W
    double scale_h, scale_w;                // mid_h / F, mid_w / F
};

struct FpCoords {
    const float* coords_in;                 // [B, 4, 2] or NULL: no coordinate part
    const float* matrix_fwd;                // [B, 2, 3] with a warp stage
    int* label_coords;                      // [B, 4, 2]
    float* coord_y;                         // [B * 4, 2] or NULL
    int n;                                  // 4 B
    int crop;
};

template <bool U8> __device__ inline float fp_value(const void* __restrict__ src, size_t off) {
    if (U8) return (float)((const unsigned char*)src)[off] / 255.f;
    return ((const float*)src)[off];
}

// one axis of grid_sample's unnormalisation: s in [-1, 1] -> first tap, fraction.  The position is clamped to [-2, size + 1] first
// (every tap of a position out there is padding anyway), so the conversion to int is defined whatever the matrix holds.
__device__ inline void fp_axis(double s, int size, int& i0, float& f) {
    double p = ((s + 1.0) * (double)size - 1.0) * 0.5;
    p = fmin(fmax(p, -2.0), (double)size + 1.0);
    const double fl = floor(p);
    i0 = (int)fl;
    f = (float)(p - fl);
}

// one axis of interpolate(bilinear, align_corners=False): output index o -> taps i0, i1 of a side of `size`, weight of i1
__device__ inline void fp_resize_axis(int o, double scale, int size, int& i0, int& i1, float& lam) {
    const double s = fmax(((double)o + 0.5) * scale - 0.5, 0.0);
    i0 = min((int)s, size - 1);
    i1 = min(i0 + 1, size - 1);
    lam = (float)(s - (double)i0);
}

__device__ inline int fp_to_int(double q) {                 // astype(int): toward zero; saturating, NaN -> INT_MIN
    if (!(q == q)) return INT_MIN;
    return (int)fmin(fmax(q, -2147483648.0), 2147483647.0);
}

__device__ inline void fp_landmarks(const FpDims& D, const FpCoords& K, const unsigned char* __restrict__ flip, int t) {
    for (int k = t; k < K.n; k += 64) {
        const int b = k >> 2;
        double h = (double)K.coords_in[2 * (size_t)k], w = (double)K.coords_in[2 * (size_t)k + 1];
        if (D.warp > 0) {
            const float* M = K.matrix_fwd + (size_t)b * 6;
            const double nh = h * 2.0 / (double)K.crop - 1.0, nw = w * 2.0 / (double)K.crop - 1.0;
            const double th = (double)M[0] * nh + (double)M[1] * nw + (double)M[2];
            const double tw = (double)M[3] * nh + (double)M[4] * nw + (double)M[5];
            h = (th + 1.0) * (double)D.warp / 2.0 * (double)D.frame / (double)D.warp;
            w = (tw + 1.0) * (double)D.warp / 2.0 * (double)D.frame / (double)D.warp;
        }
        const int ih = fp_to_int(h);
        int iw = fp_to_int(w);
        if (flip && flip[b]) {
            const long long f = (long long)D.frame - (long long)iw - 1;
            iw = (int)min(max(f, (long long)INT_MIN), (long long)INT_MAX);
        }
        K.label_coords[2 * (size_t)k] = ih;
        K.label_coords[2 * (size_t)k + 1] = iw;
        if (K.coord_y) {
            K.coord_y[2 * (size_t)k] = (float)ih;
            K.coord_y[2 * (size_t)k + 1] = (float)iw;
        }
    }
}

template <bool U8, bool WARP, int C>
__global__ __launch_bounds__(FP_THREADS) void k_frame_prep(const void* __restrict__ src, const float* __restrict__ matrix_inv,
                                                           const unsigned char* __restrict__ flip, float* __restrict__ out,
                                                           const FpDims D, const FpCoords K) {
    const int t = threadIdx.x;
    if (blockIdx.x == 0 && K.coords_in && t < 64) fp_landmarks(D, K, flip, t);
    const unsigned b = blockIdx.x / D.blocks_per_frame;
    const int p = (int)(blockIdx.x - b * D.blocks_per_frame) * FP_THREADS + t;
    const int F = D.frame;
    if (p >= F * F) return;
    const int i = p / F, j = p - i * F;
    int ri[2], rj[2];
    float ly, lx;
    fp_resize_axis(i, D.scale_h, D.mid_h, ri[0], ri[1], ly);
    fp_resize_axis(j, D.scale_w, D.mid_w, rj[0], rj[1], lx);
    const float wr[2] = {1.f - ly, ly}, wc[2] = {1.f - lx, lx};
    const size_t plane = (size_t)D.src_h * D.src_w;
    const size_t base = (size_t)b * C * plane;
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    if (WARP) {
        const float* M = matrix_inv + (size_t)b * 6;
        const double a00 = M[0], a01 = M[1], b0 = M[2], a10 = M[3], a11 = M[4], b1 = M[5];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const double nh = (double)(2 * ri[a] + 1) * D.inv_warp - 1.0;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const double nw = (double)(2 * rj[e] + 1) * D.inv_warp - 1.0;
                int y0, x0;
                float fy, fx;
                fp_axis(a00 * nh + a01 * nw + b0, D.src_h, y0, fy);
                fp_axis(a10 * nh + a11 * nw + b1, D.src_w, x0, fx);
                // the four taps: a tap outside the source reads the nearest pixel inside and counts as 0
                const bool yin0 = y0 >= 0 && y0 < D.src_h, yin1 = y0 + 1 >= 0 && y0 + 1 < D.src_h;
                const bool xin0 = x0 >= 0 && x0 < D.src_w, xin1 = x0 + 1 >= 0 && x0 + 1 < D.src_w;
                const size_t r0 = (size_t)min(max(y0, 0), D.src_h - 1) * D.src_w, r1 = (size_t)min(max(y0 + 1, 0), D.src_h - 1) * D.src_w;
                const size_t c0 = (size_t)min(max(x0, 0), D.src_w - 1), c1 = (size_t)min(max(x0 + 1, 0), D.src_w - 1);
                const float w00 = (1.f - fy) * (1.f - fx), w01 = (1.f - fy) * fx, w10 = fy * (1.f - fx), w11 = fy * fx;
                const float rw = wr[a] * wc[e];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const size_t o = base + (size_t)c * plane;
                    const float v00 = fp_value<U8>(src, o + r0 + c0), v01 = fp_value<U8>(src, o + r0 + c1);
                    const float v10 = fp_value<U8>(src, o + r1 + c0), v11 = fp_value<U8>(src, o + r1 + c1);
                    const float warped = w00 * (yin0 && xin0 ? v00 : 0.f) + w01 * (yin0 && xin1 ? v01 : 0.f) +
                                         w10 * (yin1 && xin0 ? v10 : 0.f) + w11 * (yin1 && xin1 ? v11 : 0.f);
                    acc[c] += rw * warped;
                }
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const size_t o = base + (size_t)c * plane;
            const size_t r0 = (size_t)ri[0] * D.src_w, r1 = (size_t)ri[1] * D.src_w;
            acc[c] = wr[0] * wc[0] * fp_value<U8>(src, o + r0 + rj[0]) + wr[0] * wc[1] * fp_value<U8>(src, o + r0 + rj[1]) +
                     wr[1] * wc[0] * fp_value<U8>(src, o + r1 + rj[0]) + wr[1] * wc[1] * fp_value<U8>(src, o + r1 + rj[1]);
        }
    }
    const int col = (flip && flip[b]) ? F - 1 - j : j;
    const size_t fplane = (size_t)F * F;
    const size_t pix = (size_t)i * F + col;
    if (C == 3 && D.gray) {
        out[(size_t)b * fplane + pix] = 0.2989f * acc[0] + 0.587f * acc[C > 1 ? 1 : 0] + 0.114f * acc[C > 2 ? 2 : 0];
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) out[((size_t)b * C + c) * fplane + pix] = acc[c];
    }
}

template <bool U8, bool WARP, int C>
static void fp_launch(dim3 grid, hipStream_t stream, const void* src, const float* matrix_inv, const unsigned char* flip, float* out,
                      const FpDims& D, const FpCoords& K) {
    hipLaunchKernelGGL((k_frame_prep<U8, WARP, C>), grid, dim3(FP_THREADS), 0, stream, src, matrix_inv, flip, out, D, K);
}

}  // namespace eg

using namespace eg;

extern "C" {

int eg_frame_prep(const void* src, int src_is_u8, int batch, int channels, int src_h, int src_w, const float* matrix_inv, int warp_size,
                  int frame_size, const unsigned char* flip, int gray, float* out, const float* coords_in, const float* matrix_fwd,
                  int crop_size, int* label_coords, float* coord_y, eg_stream_t stream) {
    if (batch < 1 || src_h < 1 || src_w < 1 || frame_size < 1) return set_error(EG_ERR_ARG, "batch, src_h, src_w and frame_size must be >= 1");
    if (src_h > FP_MAX_SIDE || src_w > FP_MAX_SIDE || frame_size > FP_MAX_SIDE || warp_size > FP_MAX_SIDE)
        return set_error(EG_ERR_ARG, "sides up to 32768 are supported");
    if (channels != 1 && channels != 3) return set_error(EG_ERR_ARG, "channels must be 1 or 3");
    if (gray && channels != 3) return set_error(EG_ERR_ARG, "gray needs a 3-channel source");
    if (warp_size < 0) return set_error(EG_ERR_ARG, "warp_size must be >= 0 (0: no warp stage)");
    if (warp_size > 0 && !matrix_inv) return set_error(EG_ERR_ARG, "a warp stage (warp_size > 0) needs matrix_inv");
    if (warp_size == 0 && matrix_inv) return set_error(EG_ERR_ARG, "matrix_inv without a warp stage (warp_size == 0)");
    if (!src || !out) return set_error(EG_ERR_ARG, "src and out must not be NULL");
    if (coords_in) {
        if (!label_coords) return set_error(EG_ERR_ARG, "coords_in needs label_coords");
        if (warp_size > 0 && (!matrix_fwd || crop_size < 1))
            return set_error(EG_ERR_ARG, "coords_in with a warp stage needs matrix_fwd and crop_size >= 1");
        if (batch > (1 << 28)) return set_error(EG_ERR_ARG, "batch too large for the coordinate part");
    }
    if ((uintptr_t)out % 4 || (!src_is_u8 && (uintptr_t)src % 4) || (uintptr_t)matrix_inv % 4 || (uintptr_t)matrix_fwd % 4 ||
        (uintptr_t)coords_in % 4 || (uintptr_t)label_coords % 4 || (uintptr_t)coord_y % 4)
        return set_error(EG_ERR_ARG, "out, a float32 src, the matrices and the coordinate arrays must be 4-byte aligned");
    const long long blocks_per_frame = ((long long)frame_size * frame_size + FP_THREADS - 1) / FP_THREADS;
    if (blocks_per_frame * batch >= (1ll << 31)) return set_error(EG_ERR_ARG, "batch * frame_size^2 too large for one launch");
    FpDims D{};
    D.channels = channels;
    D.src_h = src_h;
    D.src_w = src_w;
    D.warp = warp_size;
    D.frame = frame_size;
    D.mid_h = warp_size > 0 ? warp_size : src_h;
    D.mid_w = warp_size > 0 ? warp_size : src_w;
    D.gray = gray ? 1 : 0;
    D.blocks_per_frame = (unsigned)blocks_per_frame;
    D.inv_warp = warp_size > 0 ? 1.0 / (double)warp_size : 0.0;
    D.scale_h = (double)D.mid_h / (double)frame_size;
    D.scale_w = (double)D.mid_w / (double)frame_size;
    FpCoords K{};
    if (coords_in) {
        K.coords_in = coords_in;
        K.matrix_fwd = matrix_fwd;
        K.label_coords = label_coords;
        K.coord_y = coord_y;
        K.n = 4 * batch;
        K.crop = crop_size;
    }
    const dim3 grid((unsigned)(blocks_per_frame * batch));
    hipStream_t s = (hipStream_t)stream;
    const int which = (src_is_u8 ? 4 : 0) | (warp_size > 0 ? 2 : 0) | (channels == 3 ? 1 : 0);
    switch (which) {
        case 0: fp_launch<false, false, 1>(grid, s, src, matrix_inv, flip, out, D, K); break;
        case 1: fp_launch<false, false, 3>(grid, s, src, matrix_inv, flip, out, D, K); break;
        case 2: fp_launch<false, true, 1>(grid, s, src, matrix_inv, flip, out, D, K); break;
        case 3: fp_launch<false, true, 3>(grid, s, src, matrix_inv, flip, out, D, K); break;
        case 4: fp_launch<true, false, 1>(grid, s, src, matrix_inv, flip, out, D, K); break;
        case 5: fp_launch<true, false, 3>(grid, s, src, matrix_inv, flip, out, D, K); break;
        case 6: fp_launch<true, true, 1>(grid, s, src, matrix_inv, flip, out, D, K); break;
        default: fp_launch<true, true, 3>(grid, s, src, matrix_inv, flip, out, D, K); break;
    }
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

}  // extern "C"
