// The CNN-pyramid block in training mode (reference: CNNResBlock.forward with AdaptiveMaxPool2d): what is not a
// convolution of pyramid_conv.hip.  The order is pool, then ReLU, then dropout, as in the reference:
//     v = y + x,  (m, idx) = AdaptiveMaxPool2d(side_out)(v),  out = relu(m) * keep[b, o]
//   eg_pyramid_act_fwd         ONE launch, a lane per pooled element: the window of v is scanned in row-major order (the first maximum,
//                              a NaN takes over: k_adaptive_max_pool's rule), v is never written.
//   eg_pyramid_act_bwd         k_py_bwd_sums (ds = the pool's backward of g keep [out > 0] in gather form, a lane per input pixel,
//                              windows in row-major order; the chunk's sums for the BatchNorm), k_py_bwd_apply (dz, dgamma, dbeta, the
//                              chunk's sum of dz), k_sum_slices for db3 where it is wanted: embedder.hip's three launches.
//   eg_pyramid_conv_bwd_weight k_pyramid_wgrad: dw3[o][n] (n = c * 9 + tap) as a GEMM on v_mfma_f32_32x32x2_f32, M = 128 (o),
//                              N = 1152 (n), K = the pixels.  A = dz (row = o), B = the haloed x tile (column = n).
// THE ORDER OF SUMMATION of the weight gradient is its contract and a function of (batch, side) alone:
//   * The map of every frame is cut into tiles of 32 x 8 pixels; tiles are numbered frame-major, then tile row, then tile column.
//   * One tile is ONE chain from 0 per output: its pixels in row-major order, MFMA step m of a tile row takes pixels x = 2m (lane half
//     0) and 2m + 1 (half 1); tile rows below the map are not visited, and of a row's 16 steps only the groups of four that hold a
//     pixel of the map (pixels right of the map inside the last group are zero terms).  256 terms at most.
//   * The tiles are dealt to S = ceil(tiles / per) slices of per = ceil(tiles / min(tiles, 64)) consecutive tiles: S <= 64 whatever
//     the batch and the side.  Inside a slice the tile sums are added in tile order in chains of 256 (L1); every 256 tiles L1 is added
//     to L2 and cleared, every 65536 tiles L2 to L3; at the end L2 += L1, L3 += L2, and L3 is the slice.  (per < 2^24: L3 <= 256 terms.)
//   * S > 1: the slices are added by frontend_train.hip's k_sum_slices; S == 1 writes dw3 itself.
// A workgroup (4 waves) owns one slice, 64 output channels and 128 columns n (wave w: columns 32 w .. 32 w + 31, both blocks of 32
// channels: two accumulators).  A tile goes through LDS in two stages of 4 pixel rows: dz [64][4 x 32] at stride 129 (lane i reads
// bank i + p), x as 16 channels of 6 haloed rows at row stride 35 and channel stride 233 = 9 mod 32 (column n reads bank n + const:
// both operands are conflict-free ds_read_b32); the next stage's global loads are issued in front of the current stage's MFMAs.
// Every other reduction here has a fixed order in chains of at most 256 terms, as in embedder.hip (whose chunking this file repeats).
// No atomics, no allocation, nothing waits for the host; capturable.
#include "common.h"
#include "frontend.h"
#include "train_common.h"

namespace eg {

constexpr int PR_C = EG_CHANNELS;
constexpr int PR_MAX_SIDE = 512;
constexpr int PR_THREADS = 256;

__host__ __device__ inline int pr_terms(long long n) { return n <= (1ll << 29) ? 32 : 128; }
inline int pr_chunks(long long n) { return (int)((n + (long long)PR_THREADS * pr_terms(n) - 1) / ((long long)PR_THREADS * pr_terms(n))); }
inline long long pr_blocks(long long total) { return (total + PR_THREADS - 1) / PR_THREADS; }

// the 256 lanes' values added in a fixed tree; every lane gets the sum (embedder.hip's em_block_sum)
__device__ inline float pr_block_sum(float v, float* s) {
    const int t = threadIdx.x;
    __syncthreads();
    s[t] = v;
    __syncthreads();
#pragma unroll
    for (int w = PR_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) s[t] += s[t + w];
        __syncthreads();
    }
    return s[0];
}

// ---------------------------------------------------------------------------
// forward: a lane per pooled element
// ---------------------------------------------------------------------------
struct PrAct {
    const float* y;
    const float* x;
    float* keep;            // [batch * 128]
    int* idx;               // [batch, 128, side_out, side_out]
    float* out;             // [batch, 128, side_out, side_out]
    const unsigned long long* epoch;
    unsigned long long seed;
    long long total;        // batch * 128 * side_out^2
    float p, inv_keep;
    int side, side_out;
};

__global__ __launch_bounds__(PR_THREADS) void k_py_act_fwd(const PrAct A) {
    const long long e = (long long)blockIdx.x * PR_THREADS + threadIdx.x;
    if (e >= A.total) return;
    const int side_in = A.side, side_out = A.side_out, plane_out = side_out * side_out;
    const long long pl = e / plane_out;                  // b * 128 + o: the plane, and the mask's index
    const int r = (int)(e - pl * plane_out);
    const int i = r / side_out, j = r - i * side_out;
    const int y0 = (i * side_in) / side_out, y1 = ((i + 1) * side_in + side_out - 1) / side_out;
    const int x0 = (j * side_in) / side_out, x1 = ((j + 1) * side_in + side_out - 1) / side_out;
    const size_t base = (size_t)pl * side_in * side_in;
    float m = -INFINITY;
    int at = y0 * side_in + x0;
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) {
            const float v = A.y[base + yy * side_in + xx] + A.x[base + yy * side_in + xx];
            if (v > m || v != v) {                       // the first maximum in scan order; a NaN always takes over
                m = v;
                at = yy * side_in + xx;
            }
        }
    const float kp = keep_scale(A.seed + epoch_now(A.epoch), (unsigned long long)pl, A.p, A.inv_keep);
    A.out[e] = fmaxf(m, 0.f) * kp;
    A.idx[e] = at;
    if (r == 0) A.keep[pl] = kp;
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
struct PrBwd {
    const float* dout;      // pooled
    const float* out;       // pooled
    const float* keep;
    const int* idx;         // pooled
    const float* z;
    const float* save_mean;
    const float* save_invstd;
    const float* gamma;     // [128] or NULL (1)
    float* ds;
    float* dz;
    float2* part;           // [128][chunks]: (sum ds, sum ds xhat)
    float* slices;          // [chunks][128]: the chunk's sum of dz
    float* dgamma;
    float* dbeta;
    long long n;            // batch * side^2
    int side, side_out, T;
};

// grid (chunks, 128): ds[b, o, q] = sum over the windows that contain q, in row-major order, of gp where idx == q,
// gp = dout keep [out > 0] (a dropped plane has out == 0); the chunk's sums for the BatchNorm
__global__ __launch_bounds__(PR_THREADS) void k_py_bwd_sums(const PrBwd A) {
    __shared__ float s[PR_THREADS];
    const int o = blockIdx.y, t = threadIdx.x, side_in = A.side, side_out = A.side_out;
    const int plane = side_in * side_in, plane_out = side_out * side_out;
    const float mean = A.save_mean[o], invstd = A.save_invstd[o];
    const long long base = (long long)blockIdx.x * PR_THREADS * A.T;
    float a = 0.f, b = 0.f;
    for (int j = 0; j < A.T; ++j) {
        const long long e = base + (long long)j * PR_THREADS + t;
        if (e < A.n) {
            const long long f = e / plane;
            const int q = (int)(e - f * plane);
            const int y = q / side_in, x = q - y * side_in;
            const int i_lo = (y * side_out) / side_in, j_lo = (x * side_out) / side_in;
            int i_hi = ((y + 1) * side_out + side_in - 1) / side_in, j_hi = ((x + 1) * side_out + side_in - 1) / side_in;
            i_hi = i_hi < side_out ? i_hi : side_out;
            j_hi = j_hi < side_out ? j_hi : side_out;
            const size_t pl = (size_t)f * PR_C + o;
            const float kp = A.keep[pl];
            const float* g = A.dout + pl * plane_out;
            const float* po = A.out + pl * plane_out;
            const int* ix = A.idx + pl * plane_out;
            float d = 0.f;
            for (int wi = i_lo; wi < i_hi; ++wi)
                for (int wj = j_lo; wj < j_hi; ++wj) {
                    const int w = wi * side_out + wj;
                    if (ix[w] == q) d += po[w] > 0.f ? g[w] * kp : 0.f;
                }
            const size_t at = pl * plane + q;
            A.ds[at] = d;
            a += d;
            b = fmaf(d, (A.z[at] - mean) * invstd, b);
        }
    }
    const float sa = pr_block_sum(a, s);
    const float sb = pr_block_sum(b, s);
    if (t == 0) A.part[(size_t)o * gridDim.x + blockIdx.x] = make_float2(sa, sb);
}

// grid (chunks, 128): dz = gamma invstd (ds - dbeta / n - xhat dgamma / n); the first chunk's workgroup writes dgamma and dbeta
__global__ __launch_bounds__(PR_THREADS) void k_py_bwd_apply(const PrBwd A) {
    __shared__ float s[PR_THREADS];
    const int o = blockIdx.y, t = threadIdx.x, chunks = gridDim.x, plane = A.side * A.side;
    const int per = (chunks + PR_THREADS - 1) / PR_THREADS;              // <= 256: chunks <= 65536
    const float2* p = A.part + (size_t)o * chunks;
    float a = 0.f, b = 0.f;
    for (int j = 0; j < per; ++j) {
        const int i = t * per + j;
        if (i < chunks) { a += p[i].x; b += p[i].y; }
    }
    const float dbeta = pr_block_sum(a, s);
    const float dgamma = pr_block_sum(b, s);
    const float mean = A.save_mean[o], invstd = A.save_invstd[o];
    const float k = (A.gamma ? A.gamma[o] : 1.f) * invstd;
    const float mb = dbeta / (float)A.n, mg = dgamma / (float)A.n;
    const long long base = (long long)blockIdx.x * PR_THREADS * A.T;
    float sum = 0.f;
    for (int j = 0; j < A.T; ++j) {
        const long long e = base + (long long)j * PR_THREADS + t;
        if (e < A.n) {
            const long long f = e / plane;
            const size_t at = ((size_t)f * PR_C + o) * plane + (size_t)(e - f * plane);
            const float xhat = (A.z[at] - mean) * invstd;
            const float dz = k * (A.ds[at] - mb - xhat * mg);
            A.dz[at] = dz;
            sum += dz;
        }
    }
    const float total = pr_block_sum(sum, s);
    if (t == 0) {
        A.slices[(size_t)blockIdx.x * PR_C + o] = total;
        if (blockIdx.x == 0) {
            if (A.dgamma) A.dgamma[o] = dgamma;
            if (A.dbeta) A.dbeta[o] = dbeta;
        }
    }
}

// ---------------------------------------------------------------------------
// the weight gradient on the matrix unit (the contract is at the top of the file)
// ---------------------------------------------------------------------------
constexpr int PW_MAX_SLICES = 64;
constexpr int PW_N = PR_C * 9;                           // 1152 columns n = c * 9 + tap
constexpr int PW_TW = 32, PW_TH = 8;                     // pixel tile: one inner chain
constexpr int PW_SH = 4;                                 // tile rows of an LDS stage
constexpr int PW_OB = 64;                                // output channels of a workgroup
constexpr int PW_NB = 128;                               // columns of a workgroup (32 per wave)
constexpr int PW_CH = 16;                                // input channels staged: 128 consecutive columns touch at most 16
constexpr int PW_DS = PW_SH * PW_TW + 1;                 // 129: LDS stride of a dz row
constexpr int PW_LW = PW_TW + 2, PW_LH = PW_SH + 2;      // 34 x 6 haloed positions of a stage
constexpr int PW_POS = PW_LW * PW_LH;                    // 204 <= 256: a thread stages one position of every channel
constexpr int PW_XR = PW_LW + 1;                         // 35: row stride of the x image (3 dy + dx: nine taps on nine banks)
constexpr int PW_XC = 233;                               // channel stride, 9 mod 32, >= 6 * 35
constexpr int PW_DZ_PER = PW_OB * PW_SH * PW_TW / PR_THREADS;       // dz values a thread stages: 32
static_assert(PW_POS <= PR_THREADS && PW_XC >= PW_LH * PW_XR && PW_XC % 32 == 9, "x image of the weight gradient");

typedef float pw_f32x16 __attribute__((ext_vector_type(16)));

struct PwArgs {
    const float* x;         // [batch, 128, side, side]
    const float* dz;        // [batch, 128, side, side]
    float* part;            // [slices][128][1152], or dw3 itself where there is one slice
    int side, tiles_x, tiles_per_frame;
    int tiles, per;         // all tiles; tiles of a slice
};

struct PwSlicing {
    int tiles_x, tiles_per_frame, tiles, per, slices;
};

static PwSlicing pw_slicing(int batch, int side) {
    PwSlicing g;
    g.tiles_x = (side + PW_TW - 1) / PW_TW;
    g.tiles_per_frame = g.tiles_x * ((side + PW_TH - 1) / PW_TH);
    const long long tiles = (long long)batch * g.tiles_per_frame;       // < 2^31 / 8 + ...: batch side^2 < 2^31 and side <= 512
    g.tiles = (int)tiles;
    const int want = g.tiles < PW_MAX_SLICES ? g.tiles : PW_MAX_SLICES;
    g.per = (g.tiles + want - 1) / want;
    g.slices = (g.tiles + g.per - 1) / g.per;
    return g;
}

// grid (slices, 2 channel halves, 9 column groups)
__global__ __launch_bounds__(PR_THREADS) void k_pyramid_wgrad(const PwArgs A) {
    __shared__ float s_dz[PW_OB * PW_DS];
    __shared__ float s_x[PW_CH * PW_XC];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int side = A.side, plane = side * side;
    const int o0 = blockIdx.y * PW_OB;
    const int n_lo = blockIdx.z * PW_NB;
    const int c_lo = n_lo / 9;                            // the first channel staged
    const int t_lo = blockIdx.x * A.per;
    const int t_hi = t_lo + A.per < A.tiles ? t_lo + A.per : A.tiles;
    const int stages = (t_hi - t_lo) * (PW_TH / PW_SH);

    // this lane's column of B: n = (c, tap) -> its offset inside the x image for the pixel at stage position (0, 0)
    const int n = n_lo + wave * 32 + col;
    const int cl = n / 9 - c_lo, tap = n - (n / 9) * 9;
    const float* b_lane = s_x + cl * PW_XC + (tap / 3) * PW_XR + tap % 3 + half;
    const float* a_lane = s_dz + col * PW_DS + half;

    // what this thread stages: dz values (o = t / 128 + 2 j, row (t / 32) % 4, pixel t % 32) and x position t of 16 channels
    const int d_px = t & 31, d_row = (t >> 5) & 3, d_o = t >> 7;
    const int x_ly = t / PW_LW, x_lx = t - x_ly * PW_LW;
    float rdz[PW_DZ_PER], rx[PW_CH];

    auto fetch = [&](int st) {                            // global -> registers; stage st of this slice
        const int tile = t_lo + st / (PW_TH / PW_SH), h = st % (PW_TH / PW_SH);
        const int b = tile / A.tiles_per_frame, tr = tile - b * A.tiles_per_frame;
        const int tile_y = tr / A.tiles_x, tile_x = tr - tile_y * A.tiles_x;
        const int x_lo = tile_x * PW_TW, y_lo = tile_y * PW_TH + h * PW_SH;
        {
            const int y = y_lo + d_row, x = x_lo + d_px;
            const bool in = y < side && x < side;
            const float* src = A.dz + ((size_t)b * PR_C + o0 + d_o) * plane + (in ? y * side + x : 0);
#pragma unroll
            for (int j = 0; j < PW_DZ_PER; ++j) rdz[j] = in ? src[(size_t)(2 * j) * plane] : 0.f;
        }
        {
            const int y = y_lo + x_ly - 1, x = x_lo + x_lx - 1;
            const bool in = t < PW_POS && y >= 0 && y < side && x >= 0 && x < side;
            const float* src = A.x + (size_t)b * PR_C * plane + (in ? y * side + x : 0);
#pragma unroll
            for (int ci = 0; ci < PW_CH; ++ci) rx[ci] = in && c_lo + ci < PR_C ? src[(size_t)(c_lo + ci) * plane] : 0.f;
        }
    };

    pw_f32x16 acc[2], l1[2], l2[2], l3[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[a][j] = l1[a][j] = l2[a][j] = l3[a][j] = 0.f;

    if (stages > 0) fetch(0);
    for (int st = 0; st < stages; ++st) {
        // the rows and the MFMA steps of this stage that lie inside the map (uniform over the workgroup)
        const int tile = t_lo + st / (PW_TH / PW_SH), h = st % (PW_TH / PW_SH);
        const int tr = tile % A.tiles_per_frame;
        const int tile_y = tr / A.tiles_x, tile_x = tr - tile_y * A.tiles_x;
        const int y_lo = tile_y * PW_TH + h * PW_SH;
        const int rows = side - y_lo < PW_SH ? (side - y_lo > 0 ? side - y_lo : 0) : PW_SH;
        const int cols = side - tile_x * PW_TW < PW_TW ? side - tile_x * PW_TW : PW_TW;
        if (rows > 0) {
#pragma unroll
            for (int j = 0; j < PW_DZ_PER; ++j) s_dz[(d_o + 2 * j) * PW_DS + d_row * PW_TW + d_px] = rdz[j];
            if (t < PW_POS)
#pragma unroll
                for (int ci = 0; ci < PW_CH; ++ci) s_x[ci * PW_XC + x_ly * PW_XR + x_lx] = rx[ci];
            __syncthreads();
        }
        if (st + 1 < stages) fetch(st + 1);
        // steps in groups of four; the groups that hold a pixel of the map (a full tile: all four)
        const int groups = (cols + 7) / 8;
        for (int r = 0; r < rows; ++r) {
            for (int q = 0; q < groups; ++q) {
                const float* ar = a_lane + r * PW_TW + 8 * q;
                const float* br = b_lane + r * PW_XR + 8 * q;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const float bv = br[2 * m];
                    const float a0 = ar[2 * m], a1 = ar[32 * PW_DS + 2 * m];
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc[1], 0, 0, 0);
                }
            }
        }
        if (rows > 0) __syncthreads();
        if (h == PW_TH / PW_SH - 1) {                     // the tile is done: fold its chain
            const int i = tile - t_lo + 1;                // tiles of the slice finished
#pragma unroll
            for (int a = 0; a < 2; ++a) {
#pragma unroll
                for (int j = 0; j < 16; ++j) { l1[a][j] += acc[a][j]; acc[a][j] = 0.f; }
            }
            if ((i & 255) == 0) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int j = 0; j < 16; ++j) { l2[a][j] += l1[a][j]; l1[a][j] = 0.f; }
            }
            if ((i & 65535) == 0) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int j = 0; j < 16; ++j) { l3[a][j] += l2[a][j]; l2[a][j] = 0.f; }
            }
        }
    }

    // C/D: col = lane & 31 = column n, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) = output channel inside the block of 32
    float* dst = A.part + (size_t)blockIdx.x * PR_C * PW_N + n;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int oc = o0 + a * 32 + (j & 3) + 8 * (j >> 2) + 4 * half;
            dst[(size_t)oc * PW_N] = l3[a][j] + (l2[a][j] + l1[a][j]);
        }
}

static size_t pr_round256(size_t v) { return (v + 255) / 256 * 256; }
static size_t pr_part_bytes(int batch, int side) { return pr_round256((size_t)pr_chunks((long long)batch * side * side) * PR_C * sizeof(float2)); }
static size_t pr_dz_bytes(int batch, int side) { return pr_round256((size_t)pr_chunks((long long)batch * side * side) * PR_C * sizeof(float)); }
static size_t pr_wgrad_bytes(int batch, int side) {
    // min(tiles, 64) slices are reserved (the rounding of `per` may leave the last few unused): from 64 tiles on the same bytes
    const PwSlicing g = pw_slicing(batch, side);
    const int reserve = g.tiles < PW_MAX_SLICES ? g.tiles : PW_MAX_SLICES;
    return reserve > 1 ? (size_t)reserve * PR_C * PW_N * sizeof(float) : 0;
}

static bool pr_shapes_ok(int batch, int side) {
    return batch >= 1 && side >= 1 && side <= PR_MAX_SIDE && batch <= 65535 && (long long)batch * side * side < (1ll << 31);
}

static int pr_check_shapes(int batch, int side) {
    if (batch < 1) return set_error(EG_ERR_ARG, "batch must be >= 1");
    if (side < 1) return set_error(EG_ERR_ARG, "side must be >= 1");
    if (side > PR_MAX_SIDE) return set_error(EG_ERR_UNSUPPORTED, "sides above 512 are not covered");
    if (batch > 65535 || (long long)batch * side * side >= (1ll << 31)) return set_error(EG_ERR_UNSUPPORTED, "batch too large for one launch");
    return EG_OK;
}

static int pr_check_pool(int side, int side_out) {
    if (side_out < 1) return set_error(EG_ERR_ARG, "side_out must be >= 1");
    if (side_out > side) return set_error(EG_ERR_ARG, "side_out must not exceed side");
    return EG_OK;
}

}  // namespace eg

using namespace eg;

extern "C" {

// [BatchNorm sums: chunks * 128 float2][dz sums: chunks * 128 float][weight-gradient slices: <= 64 * 128 * 1152 float]; the head is
// what eg_bn2d_train_fwd takes at 128 channels, so the block's forward brings the same buffer
size_t eg_pyramid_train_workspace_bytes(int batch, int side, int side_out) {
    if (!pr_shapes_ok(batch, side) || side_out < 1 || side_out > side) return 0;
    return pr_part_bytes(batch, side) + pr_dz_bytes(batch, side) + pr_wgrad_bytes(batch, side);
}

int eg_pyramid_act_fwd(const float* y, const float* x, int batch, int side, int side_out, float p, uint64_t seed, float* keep, int* idx,
                       float* out, eg_stream_t stream) {
    if (!y || !x || !keep || !idx || !out) return set_error(EG_ERR_ARG, "y, x, keep, idx and out must not be NULL");
    if (out == x || out == y || (void*)idx == (void*)x || (void*)idx == (void*)y || (void*)idx == (void*)out || keep == x || keep == y ||
        keep == out || (void*)keep == (void*)idx)
        return set_error(EG_ERR_ARG, "keep, idx and out must not alias an input or each other");
    if (!(p >= 0.f && p < 1.f)) return set_error(EG_ERR_ARG, "dropout p must be in [0, 1)");
    if (const int rc = pr_check_shapes(batch, side)) return rc;
    if (const int rc = pr_check_pool(side, side_out)) return rc;
    if (const int rc = eg_epoch_required(p)) return rc;
    const long long total = (long long)batch * PR_C * side_out * side_out;
    const PrAct A{y, x, keep, idx, out, eg_epoch_ptr(), (unsigned long long)seed, total, p, p > 0.f ? 1.0f / (1.0f - p) : 1.0f, side, side_out};
    hipLaunchKernelGGL(k_py_act_fwd, dim3((unsigned)pr_blocks(total)), dim3(PR_THREADS), 0, (hipStream_t)stream, A);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

int eg_pyramid_act_bwd(const float* dout, const float* out, const float* keep, const int* idx, const float* z, const float* save_mean,
                       const float* save_invstd, const float* gamma, int batch, int side, int side_out, void* workspace, float* ds,
                       float* dz, float* dgamma, float* dbeta, float* db3, eg_stream_t stream) {
    if (!dout || !out || !keep || !idx || !z || !save_mean || !save_invstd || !workspace || !ds || !dz)
        return set_error(EG_ERR_ARG, "dout, out, keep, idx, z, save_mean, save_invstd, workspace, ds and dz must not be NULL");
    if (ds == dout || ds == out || ds == z || (void*)ds == (void*)idx || dz == dout || dz == out || dz == z || (void*)dz == (void*)idx ||
        dz == ds)
        return set_error(EG_ERR_ARG, "ds and dz must not alias an input or each other");
    if (const int rc = pr_check_shapes(batch, side)) return rc;
    if (const int rc = pr_check_pool(side, side_out)) return rc;
    const long long n = (long long)batch * side * side;
    if (n < 2) return set_error(EG_ERR_ARG, "Expected more than 1 value per channel when training");
    const int T = pr_terms(n), chunks = pr_chunks(n);
    float2* part = (float2*)workspace;
    float* slices = (float*)((char*)workspace + pr_part_bytes(batch, side));
    const PrBwd A{dout, out, keep, idx, z, save_mean, save_invstd, gamma, ds, dz, part, slices, dgamma, dbeta, n, side, side_out, T};
    const dim3 grid((unsigned)chunks, (unsigned)PR_C);
    hipLaunchKernelGGL(k_py_bwd_sums, grid, dim3(PR_THREADS), 0, (hipStream_t)stream, A);
    hipLaunchKernelGGL(k_py_bwd_apply, grid, dim3(PR_THREADS), 0, (hipStream_t)stream, A);
    if (db3) fs_launch(slices, chunks, PR_C, db3, (hipStream_t)stream);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

int eg_pyramid_conv_bwd_weight(const float* x, const float* dz, int batch, int side, void* workspace, float* dw3, eg_stream_t stream) {
    if (!x || !dz || !dw3) return set_error(EG_ERR_ARG, "x, dz and dw3 must not be NULL");
    if (dw3 == x || dw3 == dz) return set_error(EG_ERR_ARG, "dw3 must not alias an input");
    if (const int rc = pr_check_shapes(batch, side)) return rc;
    const PwSlicing g = pw_slicing(batch, side);
    if (g.slices > 1 && !workspace) return set_error(EG_ERR_ARG, "workspace must not be NULL");
    float* part = g.slices > 1 ? (float*)((char*)workspace + pr_part_bytes(batch, side) + pr_dz_bytes(batch, side)) : dw3;
    const PwArgs A{x, dz, part, side, g.tiles_x, g.tiles_per_frame, g.tiles, g.per};
    hipLaunchKernelGGL(k_pyramid_wgrad, dim3((unsigned)g.slices, PR_C / PW_OB, PW_N / PW_NB), dim3(PR_THREADS), 0, (hipStream_t)stream, A);
    if (g.slices > 1) fs_launch(part, g.slices, PR_C * PW_N, dw3, (hipStream_t)stream);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

}  // extern "C"
