// The CNN-pyramid variant's residual block (reference: CNNHierarchicalPatchModel, src/core/models.py:556-636): seven
// CNNResBlock(128 -> 128, kernel 3, AdaptiveMaxPool2d(side_out)) in a row, eval mode:
//     z = conv3x3(x, W3, zero padding 1) + b3,  v = relu(BatchNorm_eval(z) + x),  out = AdaptiveMaxPool2d(side_out)(v)
// (the reference pools before the ReLU; ReLU is monotone, so relu(max S) == max relu(S) exactly).  fp32 NCHW, square maps, weights
// read in torch's [128][128][3][3] layout, in place, every call.
//   side >= 4    k_pyramid_conv: the convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32.  A = weights (row = output channel),
//                B = input (column = 32 pixels contiguous in x), so C/D has col = lane & 31 = pixel and every accumulator register
//                is one 128-byte store into an NCHW plane.  A workgroup (4 waves) owns a 32 x 8 pixel tile of one frame and 32 MA
//                output channels (MA = 2, or 1 where there are few tiles); wave w owns pixel rows 2w, 2w + 1 and all MA channel
//                blocks: 2 MA independent accumulators.  The haloed input tile and the weight slice go through LDS 8 input
//                channels (72 values of k) at a time; the next chunk's global loads are issued in front of the current chunk's
//                MFMAs and land in LDS behind them.  Pixels outside the map are staged as zeros and never stored, so every side
//                runs (a side of 4 uses 4 of a wave's 32 columns): the threshold is what was measured, down to side 4, where this
//                kernel still beats the vector kernel by more than the spreads.
//   side < 4     eg_embed_block_fwd (embedder.hip's k_embed_conv_tile<., true>), unchanged, through its public entry point: the
//                declaration in echoglad_hip.h is the internal header, embedder.hip exposes nothing new.
//   the pool     eg_adaptive_max_pool_fwd (frontend.hip) from scratch to out, only where side_out != side.
// THE ORDER OF SUMMATION is the contract: k = c * 9 + 3 dy + dx (the memory order of a weight row), MFMA step m takes k = 2m (lane
// half 0) and 2m + 1 (lane half 1), m = 0 .. 575 ascending, one accumulator chain per output from 0, never split.  The f32-input
// MFMA is bit for bit a k-ordered fmaf chain, so this is k_embed_conv_tile's chain, and the epilogue below is its expression:
// both routes give the same bits.  9 is odd, so a pair straddles channels ((c, tap 8) with (c + 1, tap 0)); a chunk of 8
// channels holds 36 whole pairs, and once a chunk is unrolled each lane half's LDS offset is a compile-time constant.
// No atomics, no allocation, nothing waits for the host; capturable.
// TRAINING MODE (the order is pool, then ReLU, then dropout, as in the reference) takes the same kernel in two more modes:
//   PY_PLAIN   eg_pyramid_conv_fwd: z = chain + b3, the chain above, so z equals eg_embed_conv_fwd's bit for bit at every side
//              (from side 8 on; below, eg_embed_conv_fwd itself: the measured threshold of this epilogue).
//   PY_DGRAD   eg_pyramid_conv_bwd_data: the B operand is dz, row c of A is the transposed, tap-flipped weight matrix: value
//              k = o * 9 + tap is w3[o][c][8 - tap] (a thread stages whole nine-float pieces, stride 128 * 9 floats between them,
//              into the same LDS rows).  The chain is k_conv3x3_tile<., FE_DGRAD>'s: o ascending, tap 0 .. 8 within o, one fmaf
//              chain from 0; the epilogue adds ds.  From side 17 on: up to 16 eg_conv3x3_bwd_data sums 16 partial chains.
#include "common.h"

namespace eg {

constexpr int PY_C = EG_CHANNELS;                        // c_in == c_out == 128
constexpr int PY_MAX_SIDE = 512;
constexpr int PY_MFMA_MIN_SIDE = 4;                      // below (not measured): the embedder's kernel, the same bits
constexpr int PY_PLAIN_MFMA_MIN_SIDE = 8;                // the training forward: at side 4 the plain epilogue measured 0.91 - 0.93 x of the
                                                         // vector kernel (sides 5 - 7 not measured); the bits are the same on both routes
constexpr int PY_DGRAD_MFMA_MIN_SIDE = 17;               // the data gradient: up to side 16 the existing route is 16 partial chains
constexpr int PY_THREADS = 256;
constexpr int PT_W = 32, PT_H = 8;                       // pixel tile of a workgroup
constexpr int PT_LW = PT_W + 2, PT_LH = PT_H + 2;
constexpr int PT_POS = PT_LW * PT_LH;                    // 340 positions with the halo
constexpr int PT_PER = (PT_POS + PY_THREADS - 1) / PY_THREADS;      // positions a thread stages: 2
constexpr int PT_CIB = 8;                                // input channels per LDS stage
constexpr int PT_K = PT_CIB * 9;                         // 72 values of k per stage = 36 MFMA steps
constexpr int PY_MA1_BELOW = 256;                        // tiles (32 x 8 pixels, all frames) below which a workgroup owns 32 channels
constexpr int PT_WS = PT_K + 1;                          // LDS stride of a weight row: 73 = 9 mod 32, 32 rows on 32 banks

typedef float py_f32x16 __attribute__((ext_vector_type(16)));

// what a launch does with a finished chain, and how it reads the weights
enum { PY_EVAL = 0,         // the eval block: relu(bn(acc + b3) + x)
       PY_PLAIN = 1,        // the training forward: z = acc + b3
       PY_DGRAD = 2 };      // the data gradient: x is dz, the weights are read transposed with the taps flipped, dx = acc + ds

struct PyConv {
    const float* x;         // [batch, 128, side, side]; PY_DGRAD: dz
    const float* w3;        // [128, 128, 3, 3]
    const float* b3;        // [128] or NULL; PY_DGRAD: ds [batch, 128, side, side] or NULL
    const float* gamma;     // [128] or NULL (1)
    const float* beta;      // [128] or NULL (0)
    const float* mean;      // [128]
    const float* var;       // [128]
    float* out;             // [batch, 128, side, side]
    float eps;
    int batch, side;
};

// offset inside the staged chunk of value kk = ci * 9 + 3 dy + dx for the pixel at tile position (0, 0)
__device__ constexpr int pt_tap(int kk) { return (kk / 9) * PT_POS + ((kk % 9) / 3) * PT_LW + (kk % 9) % 3; }

template <int MA, int MODE>
__global__ __launch_bounds__(PY_THREADS) void k_pyramid_conv(const PyConv A, int tiles_x) {
    constexpr int ROWS = 32 * MA;                        // output channels of the workgroup
    constexpr int TPR = PY_THREADS / ROWS;               // threads that stage one weight row: 2, 4, 8
    constexpr int NW = PT_K / TPR;                       // consecutive weights a thread stages: 36, 18, 9
    __shared__ float s_in[PT_CIB * PT_POS];
    __shared__ float s_w[ROWS * PT_WS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int px = lane & 31, half = lane >> 5;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x_lo = tile_x * PT_W, y_lo = tile_y * PT_H;
    const int o0 = blockIdx.y * ROWS;
    const int b = blockIdx.z;
    const int side = A.side, plane = side * side;
    const float* xb = A.x + (size_t)b * PY_C * plane;

    // the positions of the haloed tile this thread stages: their offsets inside a plane, -1 in the zero padding
    int off[PT_PER];
#pragma unroll
    for (int j = 0; j < PT_PER; ++j) {
        const int pos = t + j * PY_THREADS;
        const int ly = pos / PT_LW, lx = pos - ly * PT_LW;
        const int y = y_lo + ly - 1, x = x_lo + lx - 1;
        off[j] = pos < PT_POS && y >= 0 && y < side && x >= 0 && x < side ? y * side + x : -1;
    }
    // the weights this thread stages: NW consecutive values of row w_row, from w_k on.  PY_DGRAD: row c of the transposed matrix,
    // value kk = o * 9 + tap is w3[o][c][8 - tap]; NW is a multiple of 9 (MA <= 2), so a thread stages whole (o, c) pieces of nine
    static_assert(MODE != PY_DGRAD || NW % 9 == 0, "the transposed staging takes whole taps");
    const int w_row = t / TPR, w_k = (t - w_row * TPR) * NW;
    const float* wg = MODE == PY_DGRAD ? A.w3 + ((size_t)(w_k / 9) * PY_C + o0 + w_row) * 9
                                       : A.w3 + (size_t)(o0 + w_row) * (PY_C * 9) + w_k;
    float* wl = s_w + w_row * PT_WS + w_k;

    float rin[PT_PER][PT_CIB], rw[NW];
    auto fetch = [&](int cb) {                           // global -> registers
#pragma unroll
        for (int j = 0; j < PT_PER; ++j)
#pragma unroll
            for (int ci = 0; ci < PT_CIB; ++ci) rin[j][ci] = off[j] >= 0 ? xb[(size_t)(cb + ci) * plane + off[j]] : 0.f;
#pragma unroll
        for (int j = 0; j < NW; ++j)
            rw[j] = MODE == PY_DGRAD ? wg[(size_t)(cb + j / 9) * (PY_C * 9) + 8 - j % 9] : wg[cb * 9 + j];
    };

    py_f32x16 acc[MA][2];
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[a][r][j] = 0.f;

    const float* a_lane = s_w + px * PT_WS + half;                       // A[i = lane & 31][k = lane >> 5]
    const float* b_lane = s_in + (2 * wave) * PT_LW + px;                // B[k = lane >> 5][j = lane & 31], pixel row 2 wave

    fetch(0);
    for (int cb = 0; cb < PY_C; cb += PT_CIB) {
#pragma unroll
        for (int j = 0; j < PT_PER; ++j) {
            const int pos = t + j * PY_THREADS;
            if (pos < PT_POS)
#pragma unroll
                for (int ci = 0; ci < PT_CIB; ++ci) s_in[ci * PT_POS + pos] = rin[j][ci];
        }
#pragma unroll
        for (int j = 0; j < NW; ++j) wl[j] = rw[j];
        __syncthreads();
        if (cb + PT_CIB < PY_C) fetch(cb + PT_CIB);
#pragma unroll
        for (int s = 0; s < PT_K / 2; ++s) {
            const int tap = half ? pt_tap(2 * s + 1) : pt_tap(2 * s);
            const float b0 = b_lane[tap], b1 = b_lane[tap + PT_LW];
            float av[MA];
#pragma unroll
            for (int a = 0; a < MA; ++a) av[a] = a_lane[a * 32 * PT_WS + 2 * s];
#pragma unroll
            for (int a = 0; a < MA; ++a) {
                acc[a][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], b0, acc[a][0], 0, 0, 0);
                acc[a][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], b1, acc[a][1], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // C/D: col = lane & 31 = pixel, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) = output channel inside the block of 32
    const int x = x_lo + px;
    if (x < side) {
#pragma unroll
        for (int a = 0; a < MA; ++a)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int oc = o0 + a * 32 + (j & 3) + 8 * (j >> 2) + 4 * half;
                if (MODE == PY_EVAL) {
                    // embedder.hip's epilogue, verbatim (k once for the two rows)
                    const float k = (A.gamma ? A.gamma[oc] : 1.f) / sqrtf(A.var[oc] + A.eps);
                    const float bias = A.b3 ? A.b3[oc] : 0.f, mean = A.mean[oc], beta = A.beta ? A.beta[oc] : 0.f;
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        const int y = y_lo + 2 * wave + r;
                        if (y < side) {
                            const size_t at = ((size_t)b * PY_C + oc) * plane + y * side + x;
                            const float res = A.x[at];
                            const float z = acc[a][r][j] + bias;
                            const float v = fmaxf((z - mean) * k + beta + res, 0.f);
                            A.out[at] = v;
                        }
                    }
                } else {
                    // PY_PLAIN: eg_embed_conv_fwd's z = acc + b3.  PY_DGRAD: the chain, then the residual's share (b3 holds ds)
                    const float bias = MODE == PY_PLAIN && A.b3 ? A.b3[oc] : 0.f;
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        const int y = y_lo + 2 * wave + r;
                        if (y < side) {
                            const size_t at = ((size_t)b * PY_C + oc) * plane + y * side + x;
                            if (MODE == PY_PLAIN) A.out[at] = acc[a][r][j] + bias;
                            else A.out[at] = A.b3 ? acc[a][r][j] + A.b3[at] : acc[a][r][j];
                        }
                    }
                }
            }
    }
}

template <int MA, int MODE>
static void py_launch(const PyConv& A, int tiles_x, int tiles_y, hipStream_t stream) {
    hipLaunchKernelGGL((k_pyramid_conv<MA, MODE>), dim3(tiles_x * tiles_y, PY_C / (32 * MA), A.batch), dim3(PY_THREADS), 0, stream, A, tiles_x);
}

template <int MODE>
static int py_launch_conv(const PyConv& A, hipStream_t stream) {
    const int tiles_x = (A.side + PT_W - 1) / PT_W, tiles_y = (A.side + PT_H - 1) / PT_H;
    // 64 output channels per workgroup halve the staging of the input tile; 32 where that would leave most of the chip without a
    // workgroup (measured at 64, 256 and 1024 tiles: equal from 512 tiles on, 1.5x for 32 channels at 64 tiles: DESIGN 3.6d)
    const long long tiles = (long long)tiles_x * tiles_y * A.batch;
    if (tiles >= PY_MA1_BELOW) py_launch<2, MODE>(A, tiles_x, tiles_y, stream);
    else py_launch<1, MODE>(A, tiles_x, tiles_y, stream);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

static bool py_shapes_ok(int batch, int side, int side_out) {
    return batch >= 1 && side >= 1 && side_out >= 1 && side_out <= side && side <= PY_MAX_SIDE && batch <= 65535 &&
           (long long)batch * side * side < (1ll << 31);
}

}  // namespace eg

using namespace eg;

extern "C" {

size_t eg_pyramid_block_scratch_bytes(int batch, int side, int side_out) {
    if (!py_shapes_ok(batch, side, side_out) || side_out == side) return 0;
    return (size_t)batch * PY_C * side * side * sizeof(float);
}

int eg_pyramid_block_fwd(const float* x, int batch, int side, const float* w3, const float* b3, const float* bn_weight,
                         const float* bn_bias, const float* running_mean, const float* running_var, float eps, int side_out,
                         float* scratch, float* out, eg_stream_t stream) {
    if (!x || !w3 || !running_mean || !running_var || !out)
        return set_error(EG_ERR_ARG, "x, w3, running_mean, running_var and out must not be NULL");
    if (!(eps >= 0.f)) return set_error(EG_ERR_ARG, "eps must be >= 0");
    if (batch < 1) return set_error(EG_ERR_ARG, "batch must be >= 1");
    if (side < 1 || side_out < 1) return set_error(EG_ERR_ARG, "side and side_out must be >= 1");
    if (side_out > side) return set_error(EG_ERR_ARG, "side_out must not exceed side");
    if (side > PY_MAX_SIDE) return set_error(EG_ERR_UNSUPPORTED, "sides above 512 are not covered");
    if (batch > 65535 || (long long)batch * side * side >= (1ll << 31)) return set_error(EG_ERR_UNSUPPORTED, "batch too large for one launch");
    const bool pooled = side_out != side;
    if (pooled && !scratch) return set_error(EG_ERR_ARG, "scratch must be given where side_out != side (eg_pyramid_block_scratch_bytes)");
    if (out == x || (pooled && (scratch == x || scratch == out))) return set_error(EG_ERR_ARG, "out and scratch must not alias an input or each other");
    float* full = pooled ? scratch : out;
    if (side >= PY_MFMA_MIN_SIDE) {
        const PyConv A{x, w3, b3, bn_weight, bn_bias, running_mean, running_var, full, eps, batch, side};
        if (const int rc = py_launch_conv<PY_EVAL>(A, (hipStream_t)stream)) return rc;
    } else if (const int rc = eg_embed_block_fwd(x, batch, PY_C, side, w3, b3, bn_weight, bn_bias, running_mean, running_var, eps, nullptr,
                                                 nullptr, PY_C, full, stream)) {
        return rc;
    }
    if (pooled) return eg_adaptive_max_pool_fwd(full, batch * PY_C, side, side_out, out, stream);
    return EG_OK;
}

// ---- training mode (the pointwise parts, the weight gradient and the workspace are pyramid_train.hip) ----------------------------
static int py_check_train(int batch, int side) {
    if (batch < 1) return set_error(EG_ERR_ARG, "batch must be >= 1");
    if (side < 1) return set_error(EG_ERR_ARG, "side must be >= 1");
    if (side > PY_MAX_SIDE) return set_error(EG_ERR_UNSUPPORTED, "sides above 512 are not covered");
    if (batch > 65535 || (long long)batch * side * side >= (1ll << 31)) return set_error(EG_ERR_UNSUPPORTED, "batch too large for one launch");
    return EG_OK;
}

int eg_pyramid_conv_fwd(const float* x, int batch, int side, const float* w3, const float* b3, float* z, eg_stream_t stream) {
    if (!x || !w3 || !z) return set_error(EG_ERR_ARG, "x, w3 and z must not be NULL");
    if (z == x || z == w3 || (b3 && z == b3)) return set_error(EG_ERR_ARG, "z must not alias an input");
    if (const int rc = py_check_train(batch, side)) return rc;
    if (side < PY_PLAIN_MFMA_MIN_SIDE) return eg_embed_conv_fwd(x, batch, PY_C, side, w3, b3, PY_C, z, stream);
    const PyConv A{x, w3, b3, nullptr, nullptr, nullptr, nullptr, z, 0.f, batch, side};
    return py_launch_conv<PY_PLAIN>(A, (hipStream_t)stream);
}

int eg_pyramid_conv_bwd_data(const float* dz, const float* w3, const float* ds, int batch, int side, float* dx, eg_stream_t stream) {
    if (!dz || !w3 || !dx) return set_error(EG_ERR_ARG, "dz, w3 and dx must not be NULL");
    if (dx == dz || dx == w3 || (ds && dx == ds)) return set_error(EG_ERR_ARG, "dx must not alias an input");
    if (const int rc = py_check_train(batch, side)) return rc;
    if (side < PY_DGRAD_MFMA_MIN_SIDE) {
        // k_conv3x3_deep adds 16 partial chains per output: one matrix chain would give other bits, so these sides keep the two calls
        if (const int rc = eg_conv3x3_bwd_data(dz, w3, batch, PY_C, side, PY_C, side, 0, dx, nullptr, nullptr, stream)) return rc;
        return ds ? eg_embed_res_bwd_input(ds, nullptr, batch, PY_C, PY_C, side, dx, stream) : EG_OK;
    }
    const PyConv A{dz, w3, ds, nullptr, nullptr, nullptr, nullptr, dx, 0.f, batch, side};
    return py_launch_conv<PY_DGRAD>(A, (hipStream_t)stream);
}

}  // extern "C"
