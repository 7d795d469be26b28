// The UNet front-end, both modes.  Where things are:
//   frontend.hip        the two convolution kernels in their three modes (FE_EVAL, FE_RELU, FE_DGRAD) with their launcher and shape
//                       check, and the eval-mode entry points eg_conv3x3_relu_bn_fwd and eg_adaptive_max_pool_fwd
//   frontend_train.hip  the training-mode entry points and the kernels only they launch: BatchNorm with batch statistics and its
//                       backward, the slice sums, the resize backward, the weight gradient, the pool's backward
//   frontend.h (here)   what both use: the limits, FeConv and the nearest-resize rule, the x1 / c1 test, and the adaptive max pool's
//                       forward kernel and checks (the eval pool instantiates it without indices, the training pool with them)
#pragma once
#include "common.h"

namespace eg {

constexpr int FE_MAX_SIDE = 512;
constexpr int FE_MAX_CH = 512;
constexpr int FE_DEEP_MAX_SIDE = 16;      // sides up to this one take k_conv3x3_deep (and the weight gradient's whole-plane tiles)
constexpr int FE_THREADS = 256;           // the workgroup of every kernel but the convolutions: one element per lane, or a 256-lane tree

// what a convolution launch does with a finished chain (fe_store)
enum { FE_EVAL = 0,       // eval: (relu(acc + bias) - mean) * gamma / sqrt(var + eps) + beta
       FE_RELU = 1,       // train forward: r = relu(acc + bias)
       FE_DGRAD = 2 };    // data gradient: the plain sum, weights read transposed with the taps flipped, output split in two

// A launch fills the fields its mode reads, by name; the rest stay NULL / 0.
struct FeConv {
    const float* x0 = nullptr;        // [batch, c0, side0, side0], nearest-resized to side
    const float* x1 = nullptr;        // [batch, c1, side, side] or NULL
    const float* weight = nullptr;    // [c_out, c0 + c1, 3, 3]; FE_DGRAD: [c0, c_out, 3, 3] (x0 is dz, c_out counts the convolution's inputs)
    const float* bias = nullptr;      // [c_out] or NULL; FE_EVAL, FE_RELU
    const float* gamma = nullptr;     // [c_out] or NULL (1); FE_EVAL
    const float* beta = nullptr;      // [c_out] or NULL (0); FE_EVAL
    const float* mean = nullptr;      // [c_out]; FE_EVAL
    const float* var = nullptr;       // [c_out]; FE_EVAL
    float* out = nullptr;             // [batch, c_out, side, side]; FE_DGRAD: channels < split, [batch, split, side, side] or NULL
    float eps = 0.f;                  // FE_EVAL
    int c0 = 0, c1 = 0, c_out = 0, batch = 0, side = 0, side0 = 0;
    float* out1 = nullptr;            // FE_DGRAD: channels >= split, [batch, c_out - split, side, side] or NULL
    int split = 0;                    // FE_DGRAD
};

// nearest resize: the source row / column of destination d (nn.Upsample(size=side) on a side0 map)
__host__ __device__ inline int fe_src(int d, int side0, int side) {
    const int s = (d * side0) / side;              // d < 512, side0 <= 512: no overflow
    return s < side0 - 1 ? s : side0 - 1;
}

// shapes every convolution entry point checks the same way; EG_OK or the error that was set
int fe_check_shapes(int batch, int c0, int c1, int c_out, int side, int side0);
int fe_launch_conv(const FeConv& A, int mode, hipStream_t stream);
// out[q] = the sum over S slices of part[s][q], q < Q (frontend_train.hip's k_sum_slices: 8 lane groups x chains of <= 256)
void fs_launch(const float* part, long long S, int Q, float* out, hipStream_t stream);

// the second source and its channel count come together or not at all; EG_OK or the error that was set
inline int fe_check_x1(const float* x1, int c1) {
    if ((c1 > 0) != (x1 != nullptr)) return set_error(EG_ERR_ARG, "x1 must be given exactly when c1 > 0");
    return EG_OK;
}

// workgroups of a launch with one lane per element
inline long long fe_blocks(long long total) { return (total + FE_THREADS - 1) / FE_THREADS; }

// ---------------------------------------------------------------------------
// nn.AdaptiveMaxPool2d: one thread per output element, window [floor(i in / out), ceil((i + 1) in / out)); INDEXED: the offset of
// the window's first maximum inside its plane goes to idx (the backward's gather reads it), otherwise idx is not touched
// ---------------------------------------------------------------------------
template <bool INDEXED>
__global__ __launch_bounds__(FE_THREADS) void k_adaptive_max_pool(const float* __restrict__ x, long long total, int side_in,
                                                                  int side_out, float* __restrict__ out, int* __restrict__ idx) {
    const long long e = (long long)blockIdx.x * FE_THREADS + threadIdx.x;
    if (e >= total) return;
    const int plane_out = side_out * side_out;
    const long long pl = e / plane_out;
    const int r = (int)(e - pl * plane_out);
    const int i = r / side_out, j = r - i * side_out;
    const int y0 = (i * side_in) / side_out, y1 = ((i + 1) * side_in + side_out - 1) / side_out;
    const int x0 = (j * side_in) / side_out, x1 = ((j + 1) * side_in + side_out - 1) / side_out;
    const float* src = x + pl * side_in * side_in;
    float m = -INFINITY;
    int at = y0 * side_in + x0;
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) {
            const float v = src[yy * side_in + xx];
            if (v > m || v != v) {                       // torch's rule: the first maximum in scan order; a NaN always takes over
                m = v;
                if (INDEXED) at = yy * side_in + xx;
            }
        }
    out[e] = m;
    if (INDEXED) idx[e] = at;
}

// the caller has checked its arguments (fe_pool_check, and that planes * side_out^2 fits one launch)
template <bool INDEXED>
static int fe_pool_forward(const float* x, int planes, int side_in, int side_out, float* out, int* idx, hipStream_t stream) {
    const long long total = (long long)planes * side_out * side_out;
    hipLaunchKernelGGL(k_adaptive_max_pool<INDEXED>, dim3((unsigned)fe_blocks(total)), dim3(FE_THREADS), 0, stream, x, total, side_in,
                       side_out, out, idx);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

// what the three pool entry points check the same way: the map read, the map written (NULL: `null_msg`, each entry point's own
// words) and the shape.  The aliasing test and the launch limit (fe_pool_too_large) follow in each entry point's own order.
static int fe_pool_check(const void* in, const void* out, const char* null_msg, int planes, int side_in, int side_out) {
    if (!in || !out) return set_error(EG_ERR_ARG, null_msg);
    if (planes < 1) return set_error(EG_ERR_ARG, "planes must be >= 1");
    if (side_out < 1 || side_in < 1) return set_error(EG_ERR_ARG, "side_in and side_out must be >= 1");
    if (side_out > side_in) return set_error(EG_ERR_ARG, "side_out must not exceed side_in");
    if (side_in > FE_MAX_SIDE) return set_error(EG_ERR_UNSUPPORTED, "sides above 512 are not covered");
    return EG_OK;
}

// one lane per element of `planes` maps of side `side` is more than one launch takes.  The eval forward asks for side_out, its
// own launch; the training pair asks for side_in in both directions, so that a forward that ran can always be followed by its backward
inline bool fe_pool_too_large(int planes, int side) { return fe_blocks((long long)planes * side * side) >= (1ll << 31); }

}  // namespace eg
