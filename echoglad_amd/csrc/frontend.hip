// The UNet front-end of the reference's unet_hierarchical_patch model in eval mode (src/core/models.py:639-756; DownConv :841-856,
// UpConv :859-876): conv3x3 (zero padding 1) -> ReLU -> BatchNorm with running statistics as ONE launch, whose input is the
// channel concatenation of a nearest-resized map and an optional second map (so nn.Upsample and torch.cat never materialise), and
// nn.AdaptiveMaxPool2d (the kernel is frontend.h's: the training mode runs it too).  fp32 NCHW throughout; weights are read in
// torch's own [c_out, c_in, 3, 3] layout, in place, every call: there is no cached re-layout and no cached folded parameter that
// could go stale.
//
// Two kernels serve the convolution:
//   k_conv3x3_tile   side > 16: many pixels, few channels.  A workgroup owns a 32 x 8 pixel tile and OCB output channels of one
//                    frame; the input tile with its halo goes through LDS CIB channels at a time, the weights are wave-uniform and
//                    come through the scalar cache.  One lane = one pixel, OCB accumulators.
//   k_conv3x3_deep   side <= 16: few pixels, many channels, megabytes of weights.  A workgroup owns 64 consecutive pixels of the
//                    batch (one lane each) and OCW output channels; its 16 waves split K = 9 * c_in by input channel, stream their
//                    weights through the scalar cache, and the 16 partial sums meet in LDS and are added in wave order.
// Every output element is a chain of fused multiply-adds in a fixed order (input channel ascending, tap ascending; the deep kernel
// adds its 16 chains in wave order): no atomics, the same bits on every run.  Nothing is allocated and nothing waits for the host.
#include "common.h"
#include "frontend.h"

namespace eg {

// out = (relu(acc + bias) - mean) * (gamma / sqrt(var + eps)) + beta of output channel o
__device__ inline float fe_epilogue(const FeConv& A, int o, float acc) {
    const float r = fmaxf(acc + (A.bias ? A.bias[o] : 0.f), 0.f);
    const float k = (A.gamma ? A.gamma[o] : 1.f) / sqrtf(A.var[o] + A.eps);
    return (r - A.mean[o]) * k + (A.beta ? A.beta[o] : 0.f);
}

// the nine taps of (output channel oc, input channel c) of the launch: W[oc][c] in place, or, for the data gradient (whose output
// channels are the convolution's INPUT channels, c_out of them, and whose taps run backwards), W[c][oc]; contiguous either way
template <int MODE>
__device__ inline const float* fe_taps(const FeConv& A, int oc, int c, int c_in) {
    return A.weight + (MODE == FE_DGRAD ? (size_t)c * A.c_out + oc : (size_t)oc * c_in + c) * 9;
}

// what one finished chain becomes, and where it goes: the eval epilogue, relu(acc + bias) (the train forward's r), or the plain sum
// split at channel `split` into the gradients of the two sources (either may be absent)
template <int MODE>
__device__ inline void fe_store(const FeConv& A, int b, int o, int plane, int r, float acc) {
    if (MODE == FE_EVAL) {
        A.out[((size_t)b * A.c_out + o) * plane + r] = fe_epilogue(A, o, acc);
    } else if (MODE == FE_RELU) {
        A.out[((size_t)b * A.c_out + o) * plane + r] = fmaxf(acc + (A.bias ? A.bias[o] : 0.f), 0.f);
    } else if (o < A.split) {
        if (A.out) A.out[((size_t)b * A.split + o) * plane + r] = acc;
    } else if (A.out1) {
        A.out1[((size_t)b * (A.c_out - A.split) + o - A.split) * plane + r] = acc;
    }
}

// ---------------------------------------------------------------------------
// side > 16: LDS tile with a halo
// ---------------------------------------------------------------------------
constexpr int FT_W = 32, FT_H = 8;                       // pixel tile of a workgroup: a half-wave reads one contiguous LDS row
constexpr int FT_THREADS = FT_W * FT_H;
constexpr int FT_LW = FT_W + 2, FT_LH = FT_H + 2;
constexpr int FT_POS = FT_LW * FT_LH;                    // 340 positions with the halo
constexpr int FT_PER = (FT_POS + FT_THREADS - 1) / FT_THREADS;      // positions a thread stages: 2
constexpr int FT_CIB = 8;                                // input channels per LDS stage

template <int OCB, int MODE>
__global__ __launch_bounds__(FT_THREADS) void k_conv3x3_tile(const FeConv A, int tiles_x) {
    __shared__ float s_in[FT_CIB][FT_POS];
    const int t = threadIdx.x;
    const int tx = t % FT_W, ty = t / FT_W;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x_lo = tile_x * FT_W, y_lo = tile_y * FT_H;
    const int o0 = blockIdx.y * OCB;
    const int b = blockIdx.z;
    const int side = A.side, side0 = A.side0, c0 = A.c0, c_in = A.c0 + A.c1;
    const int plane = side * side, plane0 = side0 * side0;
    const float* xb0 = A.x0 + (size_t)b * c0 * plane0;
    const float* xb1 = A.x1 ? A.x1 + (size_t)b * A.c1 * plane : nullptr;

    // the positions of the haloed tile this thread stages: their offsets inside a plane of either source, -1 in the zero padding
    int off0[FT_PER], off1[FT_PER];
#pragma unroll
    for (int j = 0; j < FT_PER; ++j) {
        const int pos = t + j * FT_THREADS;
        const int ly = pos / FT_LW, lx = pos - ly * FT_LW;
        const int y = y_lo + ly - 1, x = x_lo + lx - 1;
        const bool in = pos < FT_POS && y >= 0 && y < side && x >= 0 && x < side;
        off1[j] = in ? y * side + x : -1;
        off0[j] = in ? (side0 == side ? y * side + x : fe_src(y, side0, side) * side0 + fe_src(x, side0, side)) : -1;
    }

    float acc[OCB];
#pragma unroll
    for (int o = 0; o < OCB; ++o) acc[o] = 0.f;

    for (int cb = 0; cb < c_in; cb += FT_CIB) {
        const int nci = c_in - cb < FT_CIB ? c_in - cb : FT_CIB;
#pragma unroll
        for (int j = 0; j < FT_PER; ++j) {
            const int pos = t + j * FT_THREADS;
            if (pos < FT_POS) {
                for (int ci = 0; ci < nci; ++ci) {
                    const int c = cb + ci;
                    float v = 0.f;
                    if (off1[j] >= 0) v = c < c0 ? xb0[c * plane0 + off0[j]] : xb1[(c - c0) * plane + off1[j]];
                    s_in[ci][pos] = v;
                }
            }
        }
        __syncthreads();
        for (int ci = 0; ci < nci; ++ci) {
            float v[9];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) v[dy * 3 + dx] = s_in[ci][(ty + dy) * FT_LW + tx + dx];
#pragma unroll
            for (int o = 0; o < OCB; ++o) {
                const int oc = o0 + o < A.c_out ? o0 + o : A.c_out - 1;            // wave-uniform: scalar loads
                const float* w = fe_taps<MODE>(A, oc, cb + ci, c_in);
#pragma unroll
                for (int k = 0; k < 9; ++k) acc[o] = fmaf(v[k], w[MODE == FE_DGRAD ? 8 - k : k], acc[o]);
            }
        }
        __syncthreads();
    }

    const int y = y_lo + ty, x = x_lo + tx;
    if (y < side && x < side) {
#pragma unroll
        for (int o = 0; o < OCB; ++o)
            if (o0 + o < A.c_out)
                fe_store<MODE>(A, b, o0 + o, plane, y * side + x, acc[o]);
    }
}

// ---------------------------------------------------------------------------
// side <= 16: K split over the waves of a workgroup
// ---------------------------------------------------------------------------
constexpr int FD_WAVES = 16;
constexpr int FD_THREADS = FD_WAVES * 64;
constexpr int FD_OCW = 4;                                // output channels per workgroup

// input channels [lo, hi) of one source into acc: the lane's 9 taps come straight from global memory (the maps are a few KB per
// channel and stay in L1 / L2), an out-of-map tap loads the centre instead and is replaced by 0
template <int MODE>
__device__ inline void fd_accumulate(const float* __restrict__ src, int plane_src, const int (&off)[9], unsigned ok, const FeConv& A,
                                     int c_in, int c_shift, int lo, int hi, int o0, float (&acc)[FD_OCW]) {
#pragma unroll 2
    for (int c = lo; c < hi; ++c) {
        float v[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float l = src[(c - c_shift) * plane_src + off[k]];
            v[k] = (ok >> k) & 1u ? l : 0.f;
        }
#pragma unroll
        for (int o = 0; o < FD_OCW; ++o) {
            const int oc = o0 + o < A.c_out ? o0 + o : A.c_out - 1;                // wave-uniform: scalar loads
            const float* w = fe_taps<MODE>(A, oc, c, c_in);
#pragma unroll
            for (int k = 0; k < 9; ++k) acc[o] = fmaf(v[k], w[MODE == FE_DGRAD ? 8 - k : k], acc[o]);
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(FD_THREADS) void k_conv3x3_deep(const FeConv A, int total_px) {
    __shared__ float s_red[FD_WAVES][FD_OCW][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int side = A.side, side0 = A.side0, c0 = A.c0, c_in = A.c0 + A.c1;
    const int plane = side * side, plane0 = side0 * side0;
    const int p_raw = blockIdx.x * 64 + lane;
    const bool live = p_raw < total_px;
    const int p = live ? p_raw : 0;                      // a dead lane computes pixel 0 and stores nothing
    const int b = p / plane, r = p - b * plane;
    const int y = r / side, x = r - y * side;
    const int o0 = blockIdx.y * FD_OCW;

    int off0[9], off1[9];
    unsigned ok = 0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int yy = y + dy - 1, xx = x + dx - 1;
            const bool in = yy >= 0 && yy < side && xx >= 0 && xx < side;
            const int yc = in ? yy : y, xc = in ? xx : x;
            off1[dy * 3 + dx] = yc * side + xc;
            off0[dy * 3 + dx] = side0 == side ? yc * side + xc : fe_src(yc, side0, side) * side0 + fe_src(xc, side0, side);
            ok |= (in ? 1u : 0u) << (dy * 3 + dx);
        }

    float acc[FD_OCW];
#pragma unroll
    for (int o = 0; o < FD_OCW; ++o) acc[o] = 0.f;
    const int per = (c_in + FD_WAVES - 1) / FD_WAVES;
    const int lo = wave * per, hi = lo + per < c_in ? lo + per : c_in;
    // [lo, hi) splits at c0 into the part of x0 and the part of x1
    fd_accumulate<MODE>(A.x0 + (size_t)b * c0 * plane0, plane0, off0, ok, A, c_in, 0, lo, hi < c0 ? hi : c0, o0, acc);
    if (A.x1)
        fd_accumulate<MODE>(A.x1 + (size_t)b * A.c1 * plane, plane, off1, ok, A, c_in, c0, lo > c0 ? lo : c0, hi, o0, acc);

#pragma unroll
    for (int o = 0; o < FD_OCW; ++o) s_red[wave][o][lane] = acc[o];
    __syncthreads();
    if (wave < FD_OCW && o0 + wave < A.c_out && live) {
        float sum = s_red[0][wave][lane];
#pragma unroll
        for (int w = 1; w < FD_WAVES; ++w) sum += s_red[w][wave][lane];
        fe_store<MODE>(A, b, o0 + wave, plane, r, sum);
    }
}

template <int MODE>
static int fe_launch_mode(const FeConv& A, hipStream_t stream) {
    const long long total_px = (long long)A.batch * A.side * A.side;
    const int side = A.side, c_out = A.c_out, batch = A.batch;
    if (side <= FE_DEEP_MAX_SIDE) {
        const dim3 grid((unsigned)((total_px + 63) / 64), (unsigned)((c_out + FD_OCW - 1) / FD_OCW));
        hipLaunchKernelGGL(k_conv3x3_deep<MODE>, grid, dim3(FD_THREADS), 0, stream, A, (int)total_px);
    } else {
        const int tiles_x = (side + FT_W - 1) / FT_W, tiles_y = (side + FT_H - 1) / FT_H;
        // 8 output channels per lane halve the LDS reads per multiply-add; 4 where that would leave most of the chip without a tile
        const bool wide = c_out >= 8 && (long long)tiles_x * tiles_y * ((c_out + 7) / 8) * batch >= 512;
        if (wide)
            hipLaunchKernelGGL((k_conv3x3_tile<8, MODE>), dim3(tiles_x * tiles_y, (c_out + 7) / 8, batch), dim3(FT_THREADS), 0,
                               stream, A, tiles_x);
        else
            hipLaunchKernelGGL((k_conv3x3_tile<4, MODE>), dim3(tiles_x * tiles_y, (c_out + 3) / 4, batch), dim3(FT_THREADS), 0,
                               stream, A, tiles_x);
    }
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

int fe_check_shapes(int batch, int c0, int c1, int c_out, int side, int side0) {
    if (batch < 1) return set_error(EG_ERR_ARG, "batch must be >= 1");
    if (c0 < 1 || c1 < 0 || c_out < 1) return set_error(EG_ERR_ARG, "c0 and c_out must be >= 1, c1 >= 0");
    if (side < 1 || side0 < 1) return set_error(EG_ERR_ARG, "side and side0 must be >= 1");
    if (c0 > FE_MAX_CH || c1 > FE_MAX_CH || c0 + c1 > FE_MAX_CH || c_out > FE_MAX_CH)
        return set_error(EG_ERR_UNSUPPORTED, "channels (c0 + c1, c_out) above 512 are not covered");
    if (side > FE_MAX_SIDE || side0 > FE_MAX_SIDE) return set_error(EG_ERR_UNSUPPORTED, "sides above 512 are not covered");
    if (batch > 65535 || (long long)batch * side * side >= (1ll << 31))
        return set_error(EG_ERR_UNSUPPORTED, "batch too large for one launch");
    return EG_OK;
}

// the one launcher of both convolution kernels: the caller has checked A (fe_check_shapes)
int fe_launch_conv(const FeConv& A, int mode, hipStream_t stream) {
    if (mode == FE_EVAL) return fe_launch_mode<FE_EVAL>(A, stream);
    if (mode == FE_RELU) return fe_launch_mode<FE_RELU>(A, stream);
    return fe_launch_mode<FE_DGRAD>(A, stream);
}

}  // namespace eg

using namespace eg;

extern "C" {

int eg_conv3x3_relu_bn_fwd(const float* x0, int c0, int side0, const float* x1, int c1, int batch, int side, const float* weight,
                           const float* bias, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                           const float* bn_var, float bn_eps, int c_out, float* out, eg_stream_t stream) {
    if (!x0 || !weight || !bn_mean || !bn_var || !out)
        return set_error(EG_ERR_ARG, "x0, weight, bn_mean, bn_var and out must not be NULL");
    if (const int rc = fe_check_x1(x1, c1)) return rc;
    if (!(bn_eps >= 0.f)) return set_error(EG_ERR_ARG, "bn_eps must be >= 0");
    if (out == x0 || out == x1) return set_error(EG_ERR_ARG, "out must not alias an input");
    if (const int rc = fe_check_shapes(batch, c0, c1, c_out, side, side0)) return rc;
    FeConv A;
    A.x0 = x0; A.x1 = x1; A.weight = weight; A.bias = bias; A.out = out;
    A.gamma = bn_weight; A.beta = bn_bias; A.mean = bn_mean; A.var = bn_var; A.eps = bn_eps;
    A.c0 = c0; A.c1 = c1; A.c_out = c_out; A.batch = batch; A.side = side; A.side0 = side0;
    return fe_launch_conv(A, FE_EVAL, (hipStream_t)stream);
}

int eg_adaptive_max_pool_fwd(const float* x, int planes, int side_in, int side_out, float* out, eg_stream_t stream) {
    if (const int rc = fe_pool_check(x, out, "x and out must not be NULL", planes, side_in, side_out)) return rc;
    if (out == x) return set_error(EG_ERR_ARG, "out must not alias x");
    if (fe_pool_too_large(planes, side_out)) return set_error(EG_ERR_UNSUPPORTED, "planes * side_out^2 too large for one launch");
    return fe_pool_forward<false>(x, planes, side_in, side_out, out, nullptr, (hipStream_t)stream);
}

}  // extern "C"
