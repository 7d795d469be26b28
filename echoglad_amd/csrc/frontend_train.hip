// The UNet front-end in TRAINING mode: conv3x3 -> ReLU -> BatchNorm2d with batch statistics, its backward, and the
// adaptive max pool with its backward (the pool's forward kernel is frontend.h's, here with indices).  fp32 NCHW; the
// convolution's input is the forward's (x0 nearest-resized, concatenated with an optional x1) and is never materialised.  The two
// convolution kernels of frontend.hip run three times per block: forward with the relu(acc + bias) epilogue, and as the data
// gradient (weights read transposed, taps flipped, plain epilogue).
//
// Every reduction has a fixed order and no chain is longer than 256 terms:
//   BatchNorm statistics   a channel's batch * side^2 values are cut into chunks of 256 * T (T = 32; 128 above 2^29 values); a lane
//                          adds its T values (stride 256), the 256 lanes meet in a fixed LDS tree.  A chunk writes (sum, sum of squared
//                          deviations from ITS mean); whoever needs the channel's mean / variance combines the chunks (lane chains of
//                          <= 256 chunks, the same tree) with the pairwise update M2 = sum M2_i + n_i (mean_i - mean)^2.
//   weight gradient        one workgroup per tile of <= 256 pixels (32 x 8 of one frame above side 16, whole planes of consecutive
//                          frames up to it) and block of output x input channels; a lane owns one (o, c) pair's nine taps and adds the
//                          tile's pixels in order.  The tiles' partials are added by k_sum_slices: 8 lane groups x chains of <= 256
//                          slices (nested once more above 2048 slices), the groups in index order.
//   bias gradient          per-chunk tree sums of dz, then k_sum_slices.
//   resize backward        a source pixel adds its block of destination pixels (<= 16 x 16) in row-major order.
// No atomics; nothing is allocated; nothing waits for the host; every entry point may be captured.
#include "common.h"
#include "frontend.h"

namespace eg {

__host__ __device__ inline int fb_terms(long long n) { return n <= (1ll << 29) ? 32 : 128; }
inline int fb_chunks(long long n) { return (int)((n + (long long)FE_THREADS * fb_terms(n) - 1) / ((long long)FE_THREADS * fb_terms(n))); }
// the number of values in chunk `chunk` of a channel's n, T per lane: 256 T but for the last.  The chunk statistics and their
// combination must agree on it (M2 = sum M2_i + n_i (mean_i - mean)^2)
__device__ inline float fb_chunk_count(long long chunk, long long n, int T) {
    const long long left = n - chunk * FE_THREADS * T;
    return (float)(left < (long long)FE_THREADS * T ? left : (long long)FE_THREADS * T);
}

// the 256 lanes' values added in a fixed tree; every lane gets the sum
__device__ inline float fb_block_sum(float v, float* s) {
    const int t = threadIdx.x;
    __syncthreads();                                  // (s may still be read from the previous call)
    s[t] = v;
    __syncthreads();
#pragma unroll
    for (int w = FE_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) s[t] += s[t + w];
        __syncthreads();
    }
    return s[0];
}

// element e of channel c of an NCHW map with `plane` pixels per plane and C channels
__device__ inline size_t fb_at(long long e, int c, int C, int plane) {
    const long long b = e / plane;
    return ((size_t)b * C + c) * plane + (size_t)(e - b * plane);
}

// ---------------------------------------------------------------------------
// BatchNorm forward
// ---------------------------------------------------------------------------
// grid (chunks, C): part[c][chunk] = (sum, sum of squared deviations from the chunk's mean)
__global__ __launch_bounds__(FE_THREADS) void k_bn_chunk_stats(const float* __restrict__ r, int C, int plane, long long n, int T,
                                                               float2* __restrict__ part) {
    __shared__ float s[FE_THREADS];
    const int c = blockIdx.y, t = threadIdx.x;
    const long long base = (long long)blockIdx.x * FE_THREADS * T;
    const float cnt = fb_chunk_count(blockIdx.x, n, T);
    float sum = 0.f;
    for (int j = 0; j < T; ++j) {
        const long long e = base + (long long)j * FE_THREADS + t;
        if (e < n) sum += r[fb_at(e, c, C, plane)];
    }
    const float total = fb_block_sum(sum, s);
    const float m = total / cnt;
    float sq = 0.f;
    for (int j = 0; j < T; ++j) {
        const long long e = base + (long long)j * FE_THREADS + t;
        if (e < n) {
            const float d = r[fb_at(e, c, C, plane)] - m;
            sq = fmaf(d, d, sq);
        }
    }
    const float m2 = fb_block_sum(sq, s);
    if (t == 0) part[(size_t)c * gridDim.x + blockIdx.x] = make_float2(total, m2);
}

// mean and biased variance of channel c from its chunks, by the whole workgroup (every workgroup that asks gets the same bits)
__device__ inline void fb_channel_stats(const float2* __restrict__ part, int c, int chunks, long long n, int T, float* s, float& mean,
                                        float& var) {
    const int t = threadIdx.x;
    const int per = (chunks + FE_THREADS - 1) / FE_THREADS;             // <= 256: chunks <= 65536
    const float2* p = part + (size_t)c * chunks;
    float sum = 0.f;
    for (int j = 0; j < per; ++j) {
        const int i = t * per + j;
        if (i < chunks) sum += p[i].x;
    }
    mean = fb_block_sum(sum, s) / (float)n;
    float m2 = 0.f;
    for (int j = 0; j < per; ++j) {
        const int i = t * per + j;
        if (i < chunks) {
            const float cnt = fb_chunk_count(i, n, T);
            const float d = p[i].x / cnt - mean;
            m2 += fmaf(cnt * d, d, p[i].y);
        }
    }
    var = fb_block_sum(m2, s) / (float)n;
}

struct FbFwd {
    const float* r;
    const float2* part;
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    float* y;
    float* save_mean;
    float* save_invstd;
    long long n;
    float eps, momentum;
    int C, plane, T;
};

// grid (chunks, C): y = (r - mean) * gamma * invstd + beta; the first chunk's workgroup writes the statistics
__global__ __launch_bounds__(FE_THREADS) void k_bn_train_apply(const FbFwd A) {
    __shared__ float s[FE_THREADS];
    const int c = blockIdx.y, t = threadIdx.x;
    float mean, var;
    fb_channel_stats(A.part, c, gridDim.x, A.n, A.T, s, mean, var);
    const float invstd = 1.f / sqrtf(var + A.eps);
    const float k = (A.gamma ? A.gamma[c] : 1.f) * invstd;
    const float beta = A.beta ? A.beta[c] : 0.f;
    const long long base = (long long)blockIdx.x * FE_THREADS * A.T;
    for (int j = 0; j < A.T; ++j) {
        const long long e = base + (long long)j * FE_THREADS + t;
        if (e < A.n) {
            const size_t at = fb_at(e, c, A.C, A.plane);
            A.y[at] = (A.r[at] - mean) * k + beta;
        }
    }
    if (blockIdx.x == 0 && t == 0) {
        A.save_mean[c] = mean;
        A.save_invstd[c] = invstd;
        if (A.running_mean) A.running_mean[c] = (1.f - A.momentum) * A.running_mean[c] + A.momentum * mean;
        if (A.running_var)
            A.running_var[c] = (1.f - A.momentum) * A.running_var[c] + A.momentum * (var * ((float)A.n / (float)(A.n - 1)));
    }
}

// ---------------------------------------------------------------------------
// ReLU + BatchNorm backward
// ---------------------------------------------------------------------------
// grid (chunks, C): part[c][chunk] = (sum dy, sum dy * xhat)
__global__ __launch_bounds__(FE_THREADS) void k_bn_bwd_chunk_sums(const float* __restrict__ dy, const float* __restrict__ r,
                                                                  const float* __restrict__ save_mean,
                                                                  const float* __restrict__ save_invstd, int C, int plane, long long n,
                                                                  int T, float2* __restrict__ part) {
    __shared__ float s[FE_THREADS];
    const int c = blockIdx.y, t = threadIdx.x;
    const float mean = save_mean[c], invstd = save_invstd[c];
    const long long base = (long long)blockIdx.x * FE_THREADS * T;
    float a = 0.f, b = 0.f;
    for (int j = 0; j < T; ++j) {
        const long long e = base + (long long)j * FE_THREADS + t;
        if (e < n) {
            const size_t at = fb_at(e, c, C, plane);
            const float g = dy[at];
            a += g;
            b = fmaf(g, (r[at] - mean) * invstd, b);
        }
    }
    const float sa = fb_block_sum(a, s);
    const float sb = fb_block_sum(b, s);
    if (t == 0) part[(size_t)c * gridDim.x + blockIdx.x] = make_float2(sa, sb);
}

struct FbBwd {
    const float* dy;
    const float* r;
    const float* save_mean;
    const float* save_invstd;
    const float* gamma;
    const float2* part;
    float* dz;
    float* dz_part;         // [chunks][C]: the chunk's sum of dz (the bias gradient's slices)
    float* dgamma;          // [C] or NULL
    float* dbeta;           // [C] or NULL
    long long n;
    int C, plane, T;
};

// grid (chunks, C): dr = gamma invstd (dy - dbeta / n - xhat dgamma / n), dz = dr [r > 0]
__global__ __launch_bounds__(FE_THREADS) void k_bn_bwd_apply(const FbBwd A) {
    __shared__ float s[FE_THREADS];
    const int c = blockIdx.y, t = threadIdx.x, chunks = gridDim.x;
    const int per = (chunks + FE_THREADS - 1) / FE_THREADS;
    const float2* p = A.part + (size_t)c * chunks;
    float a = 0.f, b = 0.f;
    for (int j = 0; j < per; ++j) {
        const int i = t * per + j;
        if (i < chunks) { a += p[i].x; b += p[i].y; }
    }
    const float dbeta = fb_block_sum(a, s);
    const float dgamma = fb_block_sum(b, s);
    const float mean = A.save_mean[c], invstd = A.save_invstd[c];
    const float k = (A.gamma ? A.gamma[c] : 1.f) * invstd;
    const float mb = dbeta / (float)A.n, mg = dgamma / (float)A.n;
    const long long base = (long long)blockIdx.x * FE_THREADS * A.T;
    float sum = 0.f;
    for (int j = 0; j < A.T; ++j) {
        const long long e = base + (long long)j * FE_THREADS + t;
        if (e < A.n) {
            const size_t at = fb_at(e, c, A.C, A.plane);
            const float rv = A.r[at];
            const float xhat = (rv - mean) * invstd;
            const float dz = rv > 0.f ? k * (A.dy[at] - mb - xhat * mg) : 0.f;
            A.dz[at] = dz;
            sum += dz;
        }
    }
    const float total = fb_block_sum(sum, s);
    if (t == 0) {
        A.dz_part[(size_t)blockIdx.x * A.C + c] = total;
        if (blockIdx.x == 0) {
            if (A.dgamma) A.dgamma[c] = dgamma;
            if (A.dbeta) A.dbeta[c] = dbeta;
        }
    }
}

// ---------------------------------------------------------------------------
// out[q] = sum over slices s of part[s][q], q < Q: a workgroup owns 32 outputs; lane group g (of 8) adds slices [g L, (g + 1) L) in
// chains of <= 256 (a chain of chains above that), lane group 0 adds the eight in index order
// ---------------------------------------------------------------------------
constexpr int FS_OUT = 32, FS_GROUPS = 8;

__global__ __launch_bounds__(FE_THREADS) void k_sum_slices(const float* __restrict__ part, long long S, int Q, float* __restrict__ out) {
    __shared__ float s[FS_GROUPS][FS_OUT];
    const int ql = threadIdx.x % FS_OUT, g = threadIdx.x / FS_OUT;
    const int q = blockIdx.x * FS_OUT + ql;
    const long long L = (S + FS_GROUPS - 1) / FS_GROUPS;
    const long long lo = g * L, hi = lo + L < S ? lo + L : S;
    float outer = 0.f;
    if (q < Q) {
        for (long long s0 = lo; s0 < hi; s0 += 256) {
            const long long s1 = s0 + 256 < hi ? s0 + 256 : hi;
            float inner = 0.f;
            for (long long i = s0; i < s1; ++i) inner += part[(size_t)i * Q + q];
            outer += inner;
        }
    }
    s[g][ql] = outer;
    __syncthreads();
    if (g == 0 && q < Q) {
        float sum = s[0][ql];
#pragma unroll
        for (int k = 1; k < FS_GROUPS; ++k) sum += s[k][ql];
        out[q] = sum;
    }
}

void fs_launch(const float* part, long long S, int Q, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_sum_slices, dim3((unsigned)((Q + FS_OUT - 1) / FS_OUT)), dim3(FE_THREADS), 0, stream, part, S, Q, out);
}

// ---------------------------------------------------------------------------
// resize backward: dx0[b, c, sy, sx] = sum of full[b, c, y, x] over the destination pixels that read (sy, sx)
// ---------------------------------------------------------------------------
constexpr int FR_MAX_RATIO = 16;

__global__ __launch_bounds__(FE_THREADS) void k_resize_bwd(const float* __restrict__ full, long long total, int side0, int side,
                                                           float* __restrict__ dx0) {
    const long long e = (long long)blockIdx.x * FE_THREADS + threadIdx.x;
    if (e >= total) return;
    const int plane0 = side0 * side0;
    const long long pl = e / plane0;
    const int q = (int)(e - pl * plane0);
    const int sy = q / side0, sx = q - sy * side0;
    // destinations d with d * side0 / side == s: ceil(s side / side0) <= d < ceil((s + 1) side / side0)
    const int y_lo = (sy * side + side0 - 1) / side0, x_lo = (sx * side + side0 - 1) / side0;
    int y_hi = ((sy + 1) * side + side0 - 1) / side0, x_hi = ((sx + 1) * side + side0 - 1) / side0;
    y_hi = y_hi < side ? y_hi : side;
    x_hi = x_hi < side ? x_hi : side;
    const float* src = full + (size_t)pl * side * side;
    float sum = 0.f;
    for (int y = y_lo; y < y_hi; ++y)
        for (int x = x_lo; x < x_hi; ++x) sum += src[y * side + x];
    dx0[e] = sum;
}

// ---------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------
constexpr int FW_PX = 256;                     // pixels of a tile
constexpr int FW_POS = 576;                    // positions with the halo: 32 x 8 -> 340; planes of side 4 (16 frames) -> 576
constexpr int FW_XS = FW_POS + 1;              // odd strides: the channels of a wave read distinct banks
constexpr int FW_DS = FW_PX + 1;

struct FwArgs {
    const float* x0;
    const float* x1;
    const float* dz;
    float* out;             // [slices][c_out][c_in][9]
    int c0, c1, c_out, batch, side, side0;
    int tw, th, tiles_x, tiles_per_frame, frames;      // tile extent, tiles of a frame, frames of a tile (1 above side 16)
};

// OB x CB (output, input) channel pairs, 256 / (OB CB) pixel slices per pair
template <int OB, int CB>
__global__ __launch_bounds__(FE_THREADS) void k_conv3x3_wgrad(const FwArgs A) {
    constexpr int PS = FE_THREADS / (OB * CB);
    __shared__ float s_x[CB][FW_XS];
    __shared__ float s_dz[OB][FW_DS];
    __shared__ int s_base[FW_PX];
    const int t = threadIdx.x;
    const int side = A.side, side0 = A.side0, c0 = A.c0, c_in = A.c0 + A.c1, c_out = A.c_out;
    const int plane = side * side, plane0 = side0 * side0;
    const int tw = A.tw, th = A.th, lw = tw + 2, lh = th + 2;
    const int slice = blockIdx.x;
    const int sf = slice / A.tiles_per_frame, tile = slice - sf * A.tiles_per_frame;
    const int b0 = sf * A.frames;
    const int tile_y = tile / A.tiles_x, tile_x = tile - tile_y * A.tiles_x;
    const int x_lo = tile_x * tw, y_lo = tile_y * th;
    const int o0 = blockIdx.y * OB, cb0 = blockIdx.z * CB;
    const int npix = A.frames * tw * th, npos = A.frames * lw * lh;       // <= FW_PX, <= FW_POS (the launcher's choice of frames)

    for (int pos = t; pos < npos; pos += FE_THREADS) {
        const int f = pos / (lw * lh), q = pos - f * (lw * lh);
        const int ly = q / lw, lx = q - ly * lw;
        const int b = b0 + f, y = y_lo + ly - 1, x = x_lo + lx - 1;
        const bool in = b < A.batch && y >= 0 && y < side && x >= 0 && x < side;
        int off0 = 0;
        if (in) off0 = side0 == side ? y * side + x : fe_src(y, side0, side) * side0 + fe_src(x, side0, side);
        for (int ci = 0; ci < CB; ++ci) {
            const int c = cb0 + ci;
            float v = 0.f;
            if (in && c < c_in)
                v = c < c0 ? A.x0[((size_t)b * c0 + c) * plane0 + off0] : A.x1[((size_t)b * A.c1 + c - c0) * plane + y * side + x];
            s_x[ci][pos] = v;
        }
    }
    if (t < npix) {
        const int f = t / (tw * th), q = t - f * (tw * th);
        const int ty = q / tw, tx = q - ty * tw;
        const int b = b0 + f, y = y_lo + ty, x = x_lo + tx;
        const bool in = b < A.batch && y < side && x < side;
        s_base[t] = f * (lw * lh) + ty * lw + tx;
        for (int oi = 0; oi < OB; ++oi) {
            const int o = o0 + oi;
            s_dz[oi][t] = in && o < c_out ? A.dz[((size_t)b * c_out + o) * plane + y * side + x] : 0.f;
        }
    }
    __syncthreads();

    const int ci = t % CB, oi = (t / CB) % OB, ps = t / (CB * OB);
    const int per = (npix + PS - 1) / PS;
    const int p_lo = ps * per, p_hi = p_lo + per < npix ? p_lo + per : npix;
    float acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.f;
    for (int p = p_lo; p < p_hi; ++p) {
        const float d = s_dz[oi][p];
        const float* xs = &s_x[ci][s_base[p]];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc[ky * 3 + kx] = fmaf(d, xs[ky * lw + kx], acc[ky * 3 + kx]);
    }
    if (PS > 1) {                                    // the pixel slices of a pair meet in LDS and are added in slice order
        __syncthreads();
        float* red = &s_x[0][0];                     // PS * OB * CB * 9 = 2304 floats <= CB * FW_XS
#pragma unroll
        for (int k = 0; k < 9; ++k) red[(ps * OB * CB + oi * CB + ci) * 9 + k] = acc[k];
        __syncthreads();
        if (ps == 0) {
            for (int j = 1; j < PS; ++j)
#pragma unroll
                for (int k = 0; k < 9; ++k) acc[k] += red[(j * OB * CB + oi * CB + ci) * 9 + k];
        }
    }
    const int o = o0 + oi, c = cb0 + ci;
    if (ps == 0 && o < c_out && c < c_in) {
        float* dst = A.out + (((size_t)slice * c_out + o) * c_in + c) * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) dst[k] = acc[k];
    }
}

// the tiling of the weight gradient: whole planes of `frames` consecutive frames up to side 16, 32 x 8 tiles of one frame above
struct FwTiling {
    int tw, th, tiles_x, tiles_per_frame, frames;
    long long slices;
};

static FwTiling fw_tiling(int batch, int side) {
    FwTiling g;
    if (side <= FE_DEEP_MAX_SIDE) {
        g.tw = g.th = side;
        g.tiles_x = g.tiles_per_frame = 1;
        const int by_px = FW_PX / (side * side), by_pos = FW_POS / ((side + 2) * (side + 2));
        g.frames = by_px < by_pos ? by_px : by_pos;
        if (g.frames > batch) g.frames = batch;
        g.slices = (batch + g.frames - 1) / g.frames;
    } else {
        g.tw = 32;
        g.th = 8;
        g.tiles_x = (side + 31) / 32;
        g.tiles_per_frame = g.tiles_x * ((side + 7) / 8);
        g.frames = 1;
        g.slices = (long long)batch * g.tiles_per_frame;
    }
    return g;
}

// workspace: [bn: chunks * C float2][dz sums: chunks * C float][weight-gradient slices], each part rounded up to 256 bytes
static size_t round256(size_t v) { return (v + 255) / 256 * 256; }
static size_t ws_bn_bytes(int batch, int c_out, int side) { return round256((size_t)fb_chunks((long long)batch * side * side) * c_out * sizeof(float2)); }
static size_t ws_dz_bytes(int batch, int c_out, int side) { return round256((size_t)fb_chunks((long long)batch * side * side) * c_out * sizeof(float)); }
static size_t ws_wgrad_bytes(int batch, int c_in, int c_out, int side) {
    const FwTiling g = fw_tiling(batch, side);
    return g.slices > 1 ? round256((size_t)g.slices * c_out * c_in * 9 * sizeof(float)) : 0;
}

// ---------------------------------------------------------------------------
// the adaptive max pool's backward in gather form (the forward is frontend.h's k_adaptive_max_pool<true>)
// ---------------------------------------------------------------------------
// one lane per INPUT pixel: the windows that contain it, in row-major order, give their dy where it is their maximum
__global__ __launch_bounds__(FE_THREADS) void k_adaptive_max_pool_bwd(const float* __restrict__ dy, const int* __restrict__ idx,
                                                                      long long total, int side_in, int side_out,
                                                                      float* __restrict__ dx) {
    const long long e = (long long)blockIdx.x * FE_THREADS + threadIdx.x;
    if (e >= total) return;
    const int plane_in = side_in * side_in, plane_out = side_out * side_out;
    const long long pl = e / plane_in;
    const int q = (int)(e - pl * plane_in);
    const int y = q / side_in, x = q - y * side_in;
    // window i covers [floor(i in / out), ceil((i + 1) in / out)): those with y inside are floor(y out / in) .. ceil((y + 1) out / in) - 1
    const int i_lo = (y * side_out) / side_in, j_lo = (x * side_out) / side_in;
    int i_hi = ((y + 1) * side_out + side_in - 1) / side_in, j_hi = ((x + 1) * side_out + side_in - 1) / side_in;
    i_hi = i_hi < side_out ? i_hi : side_out;
    j_hi = j_hi < side_out ? j_hi : side_out;
    const float* g = dy + pl * plane_out;
    const int* ix = idx + pl * plane_out;
    float sum = 0.f;
    for (int i = i_lo; i < i_hi; ++i)
        for (int j = j_lo; j < j_hi; ++j)
            if (ix[i * side_out + j] == q) sum += g[i * side_out + j];
    dx[e] = sum;
}

static int bn_check(int batch, int channels, int side) {
    if (batch < 1 || channels < 1 || side < 1) return set_error(EG_ERR_ARG, "batch, channels and side must be >= 1");
    if (channels > FE_MAX_CH) return set_error(EG_ERR_UNSUPPORTED, "channels above 512 are not covered");
    if (side > FE_MAX_SIDE) return set_error(EG_ERR_UNSUPPORTED, "sides above 512 are not covered");
    if (batch > 65535 || (long long)batch * side * side >= (1ll << 31)) return set_error(EG_ERR_UNSUPPORTED, "batch too large for one launch");
    return EG_OK;
}

}  // namespace eg

using namespace eg;

extern "C" {

size_t eg_frontend_train_workspace_bytes(int batch, int c_in, int c_out, int side) {
    if (batch < 1 || c_in < 1 || c_out < 1 || side < 1 || batch > 65535 || c_in > FE_MAX_CH || c_out > FE_MAX_CH || side > FE_MAX_SIDE)
        return 0;
    return ws_bn_bytes(batch, c_out, side) + ws_dz_bytes(batch, c_out, side) + ws_wgrad_bytes(batch, c_in, c_out, side);
}

int eg_conv3x3_relu_fwd(const float* x0, int c0, int side0, const float* x1, int c1, int batch, int side, const float* weight,
                        const float* bias, int c_out, float* r, eg_stream_t stream) {
    if (!x0 || !weight || !r) return set_error(EG_ERR_ARG, "x0, weight and r must not be NULL");
    if (const int rc = fe_check_x1(x1, c1)) return rc;
    if (r == x0 || r == x1) return set_error(EG_ERR_ARG, "r must not alias an input");
    if (const int rc = fe_check_shapes(batch, c0, c1, c_out, side, side0)) return rc;
    FeConv A;
    A.x0 = x0; A.x1 = x1; A.weight = weight; A.bias = bias; A.out = r;
    A.c0 = c0; A.c1 = c1; A.c_out = c_out; A.batch = batch; A.side = side; A.side0 = side0;
    return fe_launch_conv(A, FE_RELU, (hipStream_t)stream);
}

int eg_bn2d_train_fwd(const float* r, int batch, int channels, int side, const float* gamma, const float* beta, float eps,
                      float momentum, float* running_mean, float* running_var, void* workspace, float* y, float* save_mean,
                      float* save_invstd, eg_stream_t stream) {
    if (!r || !workspace || !y || !save_mean || !save_invstd)
        return set_error(EG_ERR_ARG, "r, workspace, y, save_mean and save_invstd must not be NULL");
    if (y == r) return set_error(EG_ERR_ARG, "y must not alias r (r is kept for the backward)");
    if (const int rc = bn_check(batch, channels, side)) return rc;
    if (!(eps >= 0.f)) return set_error(EG_ERR_ARG, "eps must be >= 0");
    const long long n = (long long)batch * side * side;
    if (n < 2) return set_error(EG_ERR_ARG, "Expected more than 1 value per channel when training");
    const int T = fb_terms(n), chunks = fb_chunks(n);
    float2* part = (float2*)workspace;
    const dim3 grid((unsigned)chunks, (unsigned)channels);
    hipLaunchKernelGGL(k_bn_chunk_stats, grid, dim3(FE_THREADS), 0, (hipStream_t)stream, r, channels, side * side, n, T, part);
    FbFwd A{r, part, gamma, beta, running_mean, running_var, y, save_mean, save_invstd, n, eps, momentum, channels, side * side, T};
    hipLaunchKernelGGL(k_bn_train_apply, grid, dim3(FE_THREADS), 0, (hipStream_t)stream, A);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

int eg_relu_bn2d_bwd(const float* dy, const float* r, const float* save_mean, const float* save_invstd, const float* gamma, int batch,
                     int channels, int side, void* workspace, float* dz, float* dgamma, float* dbeta, float* dbias,
                     eg_stream_t stream) {
    if (!dy || !r || !save_mean || !save_invstd || !workspace || !dz)
        return set_error(EG_ERR_ARG, "dy, r, save_mean, save_invstd, workspace and dz must not be NULL");
    if (dz == dy || dz == r) return set_error(EG_ERR_ARG, "dz must not alias dy or r");
    if (const int rc = bn_check(batch, channels, side)) return rc;
    const long long n = (long long)batch * side * side;
    const int T = fb_terms(n), chunks = fb_chunks(n);
    float2* part = (float2*)workspace;
    float* dz_part = (float*)((char*)workspace + ws_bn_bytes(batch, channels, side));
    const dim3 grid((unsigned)chunks, (unsigned)channels);
    hipLaunchKernelGGL(k_bn_bwd_chunk_sums, grid, dim3(FE_THREADS), 0, (hipStream_t)stream, dy, r, save_mean, save_invstd, channels,
                       side * side, n, T, part);
    FbBwd A{dy, r, save_mean, save_invstd, gamma, part, dz, dz_part, dgamma, dbeta, n, channels, side * side, T};
    hipLaunchKernelGGL(k_bn_bwd_apply, grid, dim3(FE_THREADS), 0, (hipStream_t)stream, A);
    if (dbias) fs_launch(dz_part, chunks, channels, dbias, (hipStream_t)stream);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

int eg_conv3x3_bwd_data(const float* dz, const float* weight, int batch, int c_out, int side, int c0, int side0, int c1, float* dx0,
                        float* dx1, float* full, eg_stream_t stream) {
    if (!dz || !weight) return set_error(EG_ERR_ARG, "dz and weight must not be NULL");
    if (!dx0 && !dx1) return set_error(EG_ERR_ARG, "one of dx0 and dx1 must be given");
    if (dx1 && c1 < 1) return set_error(EG_ERR_ARG, "dx1 without c1");
    if (const int rc = fe_check_shapes(batch, c0, c1, c_out, side, side0)) return rc;
    const bool resized = side0 != side;
    if (dx0 && resized && !full) return set_error(EG_ERR_ARG, "a resized x0 needs the full-resolution scratch [batch, c0, side, side]");
    if (dx0 && resized && (side + side0 - 1) / side0 > FR_MAX_RATIO)
        return set_error(EG_ERR_UNSUPPORTED, "enlargements above 16 x are not covered by the backward");
    // the forward kernels on dz: c_out input channels, c0 + c1 output channels, split at c0
    FeConv A;
    A.x0 = dz; A.weight = weight; A.out = dx0 ? (resized ? full : dx0) : nullptr; A.out1 = dx1; A.split = c0;
    A.c0 = c_out; A.c_out = c0 + c1; A.batch = batch; A.side = A.side0 = side;
    if (const int rc = fe_launch_conv(A, FE_DGRAD, (hipStream_t)stream)) return rc;
    if (dx0 && resized) {
        const long long total = (long long)batch * c0 * side0 * side0;
        hipLaunchKernelGGL(k_resize_bwd, dim3((unsigned)fe_blocks(total)), dim3(FE_THREADS), 0, (hipStream_t)stream, full, total, side0,
                           side, dx0);
        EG_HIP_TRY(hipGetLastError());
    }
    return EG_OK;
}

int eg_conv3x3_bwd_weight(const float* x0, int c0, int side0, const float* x1, int c1, int batch, int side, const float* dz, int c_out,
                          void* workspace, float* dweight, eg_stream_t stream) {
    if (!x0 || !dz || !dweight) return set_error(EG_ERR_ARG, "x0, dz and dweight must not be NULL");
    if (const int rc = fe_check_x1(x1, c1)) return rc;
    if (const int rc = fe_check_shapes(batch, c0, c1, c_out, side, side0)) return rc;
    const int c_in = c0 + c1;
    const FwTiling g = fw_tiling(batch, side);
    if (g.slices > 1 && !workspace) return set_error(EG_ERR_ARG, "workspace must not be NULL");
    float* part = g.slices > 1 ? (float*)((char*)workspace + ws_bn_bytes(batch, c_out, side) + ws_dz_bytes(batch, c_out, side)) : dweight;
    FwArgs A{x0, x1, dz, part, c0, c1, c_out, batch, side, side0, g.tw, g.th, g.tiles_x, g.tiles_per_frame, g.frames};
    if (c_in <= 8 && c_out <= 8)
        hipLaunchKernelGGL((k_conv3x3_wgrad<8, 8>), dim3((unsigned)g.slices, (c_out + 7) / 8, (c_in + 7) / 8), dim3(FE_THREADS), 0,
                           (hipStream_t)stream, A);
    else
        hipLaunchKernelGGL((k_conv3x3_wgrad<16, 16>), dim3((unsigned)g.slices, (c_out + 15) / 16, (c_in + 15) / 16), dim3(FE_THREADS),
                           0, (hipStream_t)stream, A);
    if (g.slices > 1) fs_launch(part, g.slices, c_out * c_in * 9, dweight, (hipStream_t)stream);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

int eg_adaptive_max_pool_idx_fwd(const float* x, int planes, int side_in, int side_out, float* out, int* idx, eg_stream_t stream) {
    if (const int rc = fe_pool_check(x, out, "a required pointer is NULL", planes, side_in, side_out)) return rc;
    if (fe_pool_too_large(planes, side_in)) return set_error(EG_ERR_UNSUPPORTED, "planes * side_in^2 too large for one launch");
    if (!idx) return set_error(EG_ERR_ARG, "idx must not be NULL");
    if (out == x) return set_error(EG_ERR_ARG, "out must not alias x");
    return fe_pool_forward<true>(x, planes, side_in, side_out, out, idx, (hipStream_t)stream);
}

int eg_adaptive_max_pool_bwd(const float* dy, const int* idx, int planes, int side_in, int side_out, float* dx, eg_stream_t stream) {
    if (const int rc = fe_pool_check(dy, dx, "a required pointer is NULL", planes, side_in, side_out)) return rc;
    if (fe_pool_too_large(planes, side_in)) return set_error(EG_ERR_UNSUPPORTED, "planes * side_in^2 too large for one launch");
    if (!idx) return set_error(EG_ERR_ARG, "idx must not be NULL");
    if (dx == dy) return set_error(EG_ERR_ARG, "dx must not alias dy");
    const long long total = (long long)planes * side_in * side_in;
    hipLaunchKernelGGL(k_adaptive_max_pool_bwd, dim3((unsigned)fe_blocks(total)), dim3(FE_THREADS), 0, (hipStream_t)stream, dy, idx,
                       total, side_in, side_out, dx);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

}  // extern "C"
