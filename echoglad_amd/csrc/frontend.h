// What frontend.hip (the two convolution kernels) and frontend_train.hip (everything else of the train-mode front-end) share.
#pragma once
#include "common.h"

namespace eg {

constexpr int FE_MAX_SIDE = 512;
constexpr int FE_MAX_CH = 512;
constexpr int FE_DEEP_MAX_SIDE = 16;      // sides up to this one take k_conv3x3_deep (and the weight gradient's whole-plane tiles)

// what a convolution launch does with a finished chain (fe_store)
enum { FE_EVAL = 0,       // eval: (relu(acc + bias) - mean) * gamma / sqrt(var + eps) + beta
       FE_RELU = 1,       // train forward: r = relu(acc + bias)
       FE_DGRAD = 2 };    // data gradient: the plain sum, weights read transposed with the taps flipped, output split in two

struct FeConv {
    const float* x0;        // [batch, c0, side0, side0], nearest-resized to side
    const float* x1;        // [batch, c1, side, side] or NULL
    const float* weight;    // [c_out, c0 + c1, 3, 3]; FE_DGRAD: [c0, c_out, 3, 3] (x0 is dz, c_out counts the convolution's inputs)
    const float* bias;      // [c_out] or NULL
    const float* gamma;     // [c_out] or NULL (1)
    const float* beta;      // [c_out] or NULL (0)
    const float* mean;      // [c_out]
    const float* var;       // [c_out]
    float* out;             // [batch, c_out, side, side]; FE_DGRAD: channels < split, [batch, split, side, side] or NULL
    float eps;
    int c0, c1, c_out, batch, side, side0;
    float* out1;            // FE_DGRAD: channels >= split, [batch, c_out - split, side, side] or NULL
    int split;
};

// nearest resize: the source row / column of destination d (nn.Upsample(size=side) on a side0 map)
__host__ __device__ inline int fe_src(int d, int side0, int side) {
    const int s = (d * side0) / side;              // d < 512, side0 <= 512: no overflow
    return s < side0 - 1 ? s : side0 - 1;
}

// shapes every convolution entry point checks the same way; EG_OK or the error that was set
int fe_check_shapes(int batch, int c0, int c1, int c_out, int side, int side0);
int fe_launch_conv(const FeConv& A, int mode, hipStream_t stream);

}  // namespace eg
