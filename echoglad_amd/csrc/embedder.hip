// The CNN embedder's residual block (reference: CNNResBlock, src/core/models.py:71-152), the first module of every step:
//     z = conv3x3(x, W3, zero padding 1) + b3,  y = BatchNorm2d(z)  (BEFORE the ReLU),  r = W1 x + b1 (1 x 1) or r = x,
//     out = Dropout2d(relu(y + r))                         (the reference's MaxPool2d(1) is the identity)
// fp32 NCHW, square maps; weights are read in torch's own layouts, in place, every call.
//   eval      k_embed_conv_tile<., true>: ONE launch.  The shape of frontend.hip's k_conv3x3_tile: a workgroup owns a 32 x 8 pixel tile
//             and OCB output channels of one frame, the input tile with its halo goes through LDS 8 channels at a time, weights are
//             wave-uniform and come through the scalar cache.  The residual is taken from the centre tap of the staged tile, so x is
//             read once.  One kernel serves every side (sides up to 16 only occur in tests).
//   training  forward: k_embed_conv_tile<., false> (z), eg_bn2d_train_fwd of frontend_train.hip on z (2 launches), k_embed_act_fwd
//             (residual, ReLU, plane mask): 4 launches.  Backward: k_embed_bwd_sums, k_embed_bwd_apply, k_embed_sum_slices here (3), then
//             eg_conv3x3_bwd_weight (<= 2), eg_conv3x3_bwd_data (1) and k_embed_res_bwd_input (1) where x asks for a gradient.
// Every reduction has a fixed order in chains of at most 256 terms, as in frontend_train.hip (whose chunking this file repeats: a
// channel's batch * side^2 values in chunks of 256 * T, T = 32, 128 above 2^29 values; 256 lanes meet in a fixed LDS tree; the chunks
// are combined in lane chains of <= 256 and the same tree).  No atomics, no allocation, nothing waits for the host; capturable.
#include "common.h"
#include "train_common.h"

namespace eg {

constexpr int EM_MAX_SIDE = 512;
constexpr int EM_MAX_CH = 128;
constexpr int EM_THREADS = 256;

__host__ __device__ inline int em_terms(long long n) { return n <= (1ll << 29) ? 32 : 128; }
inline int em_chunks(long long n) { return (int)((n + (long long)EM_THREADS * em_terms(n) - 1) / ((long long)EM_THREADS * em_terms(n))); }
inline long long em_blocks(long long total) { return (total + EM_THREADS - 1) / EM_THREADS; }

// the 256 lanes' values added in a fixed tree; every lane gets the sum
__device__ inline float em_block_sum(float v, float* s) {
    const int t = threadIdx.x;
    __syncthreads();                                  // (s may still be read from the previous call)
    s[t] = v;
    __syncthreads();
#pragma unroll
    for (int w = EM_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) s[t] += s[t + w];
        __syncthreads();
    }
    return s[0];
}

// element e (of batch * plane) of channel c of an NCHW map with C channels
__device__ inline size_t em_at(long long e, int c, int C, int plane) {
    const long long b = e / plane;
    return ((size_t)b * C + c) * plane + (size_t)(e - b * plane);
}

// ---------------------------------------------------------------------------
// the convolution: LDS tile with a halo; EVAL: the whole block's epilogue, otherwise z = acc + b3
// ---------------------------------------------------------------------------
struct EmConv {
    const float* x;         // [batch, c_in, side, side]
    const float* w3;        // [c_out, c_in, 3, 3]
    const float* b3;        // [c_out] or NULL
    const float* w1;        // [c_out, c_in] or NULL (identity residual, c_in == c_out); EVAL
    const float* b1;        // [c_out] or NULL; EVAL
    const float* gamma;     // [c_out] or NULL (1); EVAL
    const float* beta;      // [c_out] or NULL (0); EVAL
    const float* mean;      // [c_out]; EVAL
    const float* var;       // [c_out]; EVAL
    float* out;             // [batch, c_out, side, side]
    float eps;
    int c_in, c_out, batch, side;
};

constexpr int ET_W = 32, ET_H = 8;                       // pixel tile of a workgroup: a half-wave reads one contiguous LDS row
constexpr int ET_LW = ET_W + 2, ET_LH = ET_H + 2;
constexpr int ET_POS = ET_LW * ET_LH;                    // 340 positions with the halo
constexpr int ET_PER = (ET_POS + EM_THREADS - 1) / EM_THREADS;      // positions a thread stages: 2
constexpr int ET_CIB = 8;                                // input channels per LDS stage

template <int OCB, bool EVAL>
__global__ __launch_bounds__(EM_THREADS) void k_embed_conv_tile(const EmConv A, int tiles_x) {
    __shared__ float s_in[ET_CIB][ET_POS];
    const int t = threadIdx.x;
    const int tx = t % ET_W, ty = t / ET_W;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x_lo = tile_x * ET_W, y_lo = tile_y * ET_H;
    const int o0 = blockIdx.y * OCB;
    const int b = blockIdx.z;
    const int side = A.side, c_in = A.c_in, c_out = A.c_out;
    const int plane = side * side;
    const float* xb = A.x + (size_t)b * c_in * plane;

    // the positions of the haloed tile this thread stages: their offsets inside a plane, -1 in the zero padding
    int off[ET_PER];
#pragma unroll
    for (int j = 0; j < ET_PER; ++j) {
        const int pos = t + j * EM_THREADS;
        const int ly = pos / ET_LW, lx = pos - ly * ET_LW;
        const int y = y_lo + ly - 1, x = x_lo + lx - 1;
        off[j] = pos < ET_POS && y >= 0 && y < side && x >= 0 && x < side ? y * side + x : -1;
    }

    float acc[OCB], res[OCB];
#pragma unroll
    for (int o = 0; o < OCB; ++o) {
        acc[o] = 0.f;
        const int oc = o0 + o < c_out ? o0 + o : c_out - 1;
        res[o] = EVAL && A.w1 && A.b1 ? A.b1[oc] : 0.f;
    }

    for (int cb = 0; cb < c_in; cb += ET_CIB) {
        const int nci = c_in - cb < ET_CIB ? c_in - cb : ET_CIB;
#pragma unroll
        for (int j = 0; j < ET_PER; ++j) {
            const int pos = t + j * EM_THREADS;
            if (pos < ET_POS)
                for (int ci = 0; ci < nci; ++ci) s_in[ci][pos] = off[j] >= 0 ? xb[(size_t)(cb + ci) * plane + off[j]] : 0.f;
        }
        __syncthreads();
        for (int ci = 0; ci < nci; ++ci) {
            const int c = cb + ci;
            float v[9];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) v[dy * 3 + dx] = s_in[ci][(ty + dy) * ET_LW + tx + dx];
#pragma unroll
            for (int o = 0; o < OCB; ++o) {
                const int oc = o0 + o < c_out ? o0 + o : c_out - 1;                // wave-uniform: scalar loads
                const float* w = A.w3 + ((size_t)oc * c_in + c) * 9;
#pragma unroll
                for (int k = 0; k < 9; ++k) acc[o] = fmaf(v[k], w[k], acc[o]);
                if (EVAL) {                                                        // the residual: the centre tap, channel ascending
                    if (A.w1) res[o] = fmaf(v[4], A.w1[(size_t)oc * c_in + c], res[o]);
                    else if (c == oc) res[o] = v[4];
                }
            }
        }
        __syncthreads();
    }

    const int y = y_lo + ty, x = x_lo + tx;
    if (y < side && x < side) {
#pragma unroll
        for (int o = 0; o < OCB; ++o) {
            const int oc = o0 + o;
            if (oc < c_out) {
                const float z = acc[o] + (A.b3 ? A.b3[oc] : 0.f);
                float v = z;
                if (EVAL) {
                    const float k = (A.gamma ? A.gamma[oc] : 1.f) / sqrtf(A.var[oc] + A.eps);
                    v = fmaxf((z - A.mean[oc]) * k + (A.beta ? A.beta[oc] : 0.f) + res[o], 0.f);
                }
                A.out[((size_t)b * c_out + oc) * plane + y * side + x] = v;
            }
        }
    }
}

template <bool EVAL>
static int em_launch_conv(const EmConv& A, hipStream_t stream) {
    const int tiles_x = (A.side + ET_W - 1) / ET_W, tiles_y = (A.side + ET_H - 1) / ET_H;
    // 8 output channels per lane halve the LDS reads per multiply-add; 4 where that would leave most of the chip without a tile
    const bool wide = A.c_out >= 8 && (long long)tiles_x * tiles_y * ((A.c_out + 7) / 8) * A.batch >= 512;
    if (wide)
        hipLaunchKernelGGL((k_embed_conv_tile<8, EVAL>), dim3(tiles_x * tiles_y, (A.c_out + 7) / 8, A.batch), dim3(EM_THREADS), 0, stream,
                           A, tiles_x);
    else
        hipLaunchKernelGGL((k_embed_conv_tile<4, EVAL>), dim3(tiles_x * tiles_y, (A.c_out + 3) / 4, A.batch), dim3(EM_THREADS), 0, stream,
                           A, tiles_x);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

// ---------------------------------------------------------------------------
// training forward: out = relu(y + r) keep[b, o]; grid (pixel blocks of batch * plane, c_out): the 1 x 1 weights are wave-uniform
// ---------------------------------------------------------------------------
struct EmAct {
    const float* y;
    const float* x;
    const float* w1;        // [c_out, c_in] or NULL (identity)
    const float* b1;        // [c_out] or NULL
    float* keep;            // [batch * c_out]
    float* out;
    const unsigned long long* epoch;
    unsigned long long seed;
    long long total;        // batch * plane
    float p, inv_keep;
    int c_in, c_out, plane;
};

__global__ __launch_bounds__(EM_THREADS) void k_embed_act_fwd(const EmAct A) {
    const long long e = (long long)blockIdx.x * EM_THREADS + threadIdx.x;
    if (e >= A.total) return;
    const int o = blockIdx.y, plane = A.plane, c_in = A.c_in;
    const long long b = e / plane;
    const int q = (int)(e - b * plane);
    float r;
    if (A.w1) {
        r = A.b1 ? A.b1[o] : 0.f;
        const float* xp = A.x + (size_t)b * c_in * plane + q;
        for (int c = 0; c < c_in; ++c) r = fmaf(xp[(size_t)c * plane], A.w1[(size_t)o * c_in + c], r);
    } else {
        r = A.x[((size_t)b * c_in + o) * plane + q];
    }
    const unsigned long long idx = (unsigned long long)b * A.c_out + o;
    const float kp = keep_scale(A.seed + epoch_now(A.epoch), idx, A.p, A.inv_keep);
    A.out[((size_t)b * A.c_out + o) * plane + q] = fmaxf(A.y[((size_t)b * A.c_out + o) * plane + q] + r, 0.f) * kp;
    if (q == 0) A.keep[idx] = kp;
}

// ---------------------------------------------------------------------------
// training backward
// ---------------------------------------------------------------------------
struct EmBwd {
    const float* dout;
    const float* out;
    const float* keep;
    const float* x;
    const float* z;
    const float* save_mean;
    const float* save_invstd;
    const float* gamma;     // [c_out] or NULL (1)
    float* ds;
    float* dz;
    float2* part;           // [c_out][chunks]: (sum ds, sum ds xhat)
    float* slices;          // [chunks][Q]: the chunk's sum of dz per channel, then of ds x per (o, c)
    float* dgamma;
    float* dbeta;
    float* db1;
    long long n;
    int c_in, c_out, plane, T, Q, want_dw1;
};

// grid (chunks, c_out): ds = dout keep [out > 0] (a dropped plane has out == 0), the chunk's sums for the BatchNorm and for dW1
__global__ __launch_bounds__(EM_THREADS) void k_embed_bwd_sums(const EmBwd A) {
    __shared__ float s[EM_THREADS];
    const int o = blockIdx.y, t = threadIdx.x, plane = A.plane, c_out = A.c_out;
    const float mean = A.save_mean[o], invstd = A.save_invstd[o];
    const long long base = (long long)blockIdx.x * EM_THREADS * A.T;
    float a = 0.f, b = 0.f;
    for (int j = 0; j < A.T; ++j) {
        const long long e = base + (long long)j * EM_THREADS + t;
        if (e < A.n) {
            const long long f = e / plane;
            const size_t at = ((size_t)f * c_out + o) * plane + (size_t)(e - f * plane);
            const float d = A.out[at] > 0.f ? A.dout[at] * A.keep[f * c_out + o] : 0.f;
            A.ds[at] = d;
            a += d;
            b = fmaf(d, (A.z[at] - mean) * invstd, b);
        }
    }
    const float sa = em_block_sum(a, s);
    const float sb = em_block_sum(b, s);
    if (t == 0) A.part[(size_t)o * gridDim.x + blockIdx.x] = make_float2(sa, sb);
    if (A.want_dw1) {
        for (int c = 0; c < A.c_in; ++c) {
            float w = 0.f;
            for (int j = 0; j < A.T; ++j) {
                const long long e = base + (long long)j * EM_THREADS + t;
                if (e < A.n) w = fmaf(A.ds[em_at(e, o, c_out, plane)], A.x[em_at(e, c, A.c_in, plane)], w);   // this lane's own stores
            }
            const float sw = em_block_sum(w, s);
            if (t == 0) A.slices[(size_t)blockIdx.x * A.Q + c_out + o * A.c_in + c] = sw;
        }
    }
}

// grid (chunks, c_out): dz = gamma invstd (ds - dbeta / n - xhat dgamma / n); the first chunk's workgroup writes dgamma, dbeta, db1
__global__ __launch_bounds__(EM_THREADS) void k_embed_bwd_apply(const EmBwd A) {
    __shared__ float s[EM_THREADS];
    const int o = blockIdx.y, t = threadIdx.x, chunks = gridDim.x;
    const int per = (chunks + EM_THREADS - 1) / EM_THREADS;              // <= 256: chunks <= 65536
    const float2* p = A.part + (size_t)o * chunks;
    float a = 0.f, b = 0.f;
    for (int j = 0; j < per; ++j) {
        const int i = t * per + j;
        if (i < chunks) { a += p[i].x; b += p[i].y; }
    }
    const float dbeta = em_block_sum(a, s);
    const float dgamma = em_block_sum(b, s);
    const float mean = A.save_mean[o], invstd = A.save_invstd[o];
    const float k = (A.gamma ? A.gamma[o] : 1.f) * invstd;
    const float mb = dbeta / (float)A.n, mg = dgamma / (float)A.n;
    const long long base = (long long)blockIdx.x * EM_THREADS * A.T;
    float sum = 0.f;
    for (int j = 0; j < A.T; ++j) {
        const long long e = base + (long long)j * EM_THREADS + t;
        if (e < A.n) {
            const size_t at = em_at(e, o, A.c_out, A.plane);
            const float xhat = (A.z[at] - mean) * invstd;
            const float dz = k * (A.ds[at] - mb - xhat * mg);
            A.dz[at] = dz;
            sum += dz;
        }
    }
    const float total = em_block_sum(sum, s);
    if (t == 0) {
        A.slices[(size_t)blockIdx.x * A.Q + o] = total;
        if (blockIdx.x == 0) {
            if (A.dgamma) A.dgamma[o] = dgamma;
            if (A.dbeta) A.dbeta[o] = dbeta;
            if (A.db1) A.db1[o] = dbeta;               // db1 = sum ds = dbeta
        }
    }
}

// sum over slices i of part[i][q] for q in [q_lo, q_hi): columns < split go to out0[q], the rest to out1[q - split] (either may be
// NULL).  A workgroup owns 32 columns; lane group g (of 8) adds slices [g L, (g + 1) L) in chains of <= 256 (a chain of chains above
// that), lane group 0 adds the eight in index order: frontend_train.hip's k_sum_slices with two destinations
constexpr int ES_OUT = 32, ES_GROUPS = 8;

__global__ __launch_bounds__(EM_THREADS) void k_embed_sum_slices(const float* __restrict__ part, long long S, int Q, int q_lo, int q_hi,
                                                                 int split, float* __restrict__ out0, float* __restrict__ out1) {
    __shared__ float s[ES_GROUPS][ES_OUT];
    const int ql = threadIdx.x % ES_OUT, g = threadIdx.x / ES_OUT;
    const int q = q_lo + blockIdx.x * ES_OUT + ql;
    const long long L = (S + ES_GROUPS - 1) / ES_GROUPS;
    const long long lo = g * L, hi = lo + L < S ? lo + L : S;
    float outer = 0.f;
    if (q < q_hi) {
        for (long long s0 = lo; s0 < hi; s0 += 256) {
            const long long s1 = s0 + 256 < hi ? s0 + 256 : hi;
            float inner = 0.f;
            for (long long i = s0; i < s1; ++i) inner += part[(size_t)i * Q + q];
            outer += inner;
        }
    }
    s[g][ql] = outer;
    __syncthreads();
    if (g == 0 && q < q_hi) {
        float sum = s[0][ql];
#pragma unroll
        for (int k = 1; k < ES_GROUPS; ++k) sum += s[k][ql];
        if (q < split) { if (out0) out0[q] = sum; }
        else if (out1) out1[q - split] = sum;
    }
}

// grid (pixel blocks of batch * plane, c_in): dx[b, c] += sum over o (ascending) of W1[o][c] ds[b, o], or ds[b, c] (identity)
__global__ __launch_bounds__(EM_THREADS) void k_embed_res_bwd_input(const float* __restrict__ ds, const float* __restrict__ w1, long long total,
                                                                    int c_in, int c_out, int plane, float* __restrict__ dx) {
    const long long e = (long long)blockIdx.x * EM_THREADS + threadIdx.x;
    if (e >= total) return;
    const int c = blockIdx.y;
    const long long b = e / plane;
    const int q = (int)(e - b * plane);
    float acc;
    if (w1) {
        acc = 0.f;
        const float* dp = ds + (size_t)b * c_out * plane + q;
        for (int o = 0; o < c_out; ++o) acc = fmaf(dp[(size_t)o * plane], w1[(size_t)o * c_in + c], acc);
    } else {
        acc = ds[((size_t)b * c_out + c) * plane + q];
    }
    dx[((size_t)b * c_in + c) * plane + q] += acc;
}

static int em_check_shapes(int batch, int c_in, int c_out, int side) {
    if (batch < 1) return set_error(EG_ERR_ARG, "batch must be >= 1");
    if (c_in < 1 || c_out < 1) return set_error(EG_ERR_ARG, "c_in and c_out must be >= 1");
    if (side < 1) return set_error(EG_ERR_ARG, "side must be >= 1");
    if (c_in > EM_MAX_CH || c_out > EM_MAX_CH) return set_error(EG_ERR_UNSUPPORTED, "embedder channels above 128 are not covered");
    if (side > EM_MAX_SIDE) return set_error(EG_ERR_UNSUPPORTED, "sides above 512 are not covered");
    if (batch > 65535 || (long long)batch * side * side >= (1ll << 31)) return set_error(EG_ERR_UNSUPPORTED, "batch too large for one launch");
    return EG_OK;
}

// the residual's weights: W1 is needed exactly where the channel counts differ (it may be given where they agree); b1 only with W1
static int em_check_residual(const float* w1, const float* b1, int c_in, int c_out) {
    if (!w1 && c_in != c_out) return set_error(EG_ERR_ARG, "w1 must be given where c_in != c_out (there is no identity residual)");
    if (b1 && !w1) return set_error(EG_ERR_ARG, "b1 without w1");
    return EG_OK;
}

static size_t em_round256(size_t v) { return (v + 255) / 256 * 256; }
static size_t em_part_bytes(int batch, int c_out, int side) { return em_round256((size_t)em_chunks((long long)batch * side * side) * c_out * sizeof(float2)); }
static size_t em_slice_bytes(int batch, int c_in, int c_out, int side) {
    return em_round256((size_t)em_chunks((long long)batch * side * side) * c_out * (1 + c_in) * sizeof(float));
}

}  // namespace eg

using namespace eg;

extern "C" {

size_t eg_embed_workspace_bytes(int batch, int c_in, int c_out, int side) {
    if (batch < 1 || c_in < 1 || c_out < 1 || side < 1 || batch > 65535 || c_in > EM_MAX_CH || c_out > EM_MAX_CH || side > EM_MAX_SIDE ||
        (long long)batch * side * side >= (1ll << 31))
        return 0;
    return em_part_bytes(batch, c_out, side) + em_slice_bytes(batch, c_in, c_out, side);
}

int eg_embed_block_fwd(const float* x, int batch, int c_in, int side, const float* w3, const float* b3, const float* bn_weight,
                       const float* bn_bias, const float* bn_mean, const float* bn_var, float bn_eps, const float* w1, const float* b1,
                       int c_out, float* out, eg_stream_t stream) {
    if (!x || !w3 || !bn_mean || !bn_var || !out) return set_error(EG_ERR_ARG, "x, w3, bn_mean, bn_var and out must not be NULL");
    if (!(bn_eps >= 0.f)) return set_error(EG_ERR_ARG, "bn_eps must be >= 0");
    if (out == x) return set_error(EG_ERR_ARG, "out must not alias an input");
    if (const int rc = em_check_shapes(batch, c_in, c_out, side)) return rc;
    if (const int rc = em_check_residual(w1, b1, c_in, c_out)) return rc;
    const EmConv A{x, w3, b3, w1, b1, bn_weight, bn_bias, bn_mean, bn_var, out, bn_eps, c_in, c_out, batch, side};
    return em_launch_conv<true>(A, (hipStream_t)stream);
}

int eg_embed_conv_fwd(const float* x, int batch, int c_in, int side, const float* w3, const float* b3, int c_out, float* z,
                      eg_stream_t stream) {
    if (!x || !w3 || !z) return set_error(EG_ERR_ARG, "x, w3 and z must not be NULL");
    if (z == x) return set_error(EG_ERR_ARG, "z must not alias an input");
    if (const int rc = em_check_shapes(batch, c_in, c_out, side)) return rc;
    const EmConv A{x, w3, b3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, z, 0.f, c_in, c_out, batch, side};
    return em_launch_conv<false>(A, (hipStream_t)stream);
}

int eg_embed_act_fwd(const float* y, const float* x, int batch, int c_in, int side, const float* w1, const float* b1, int c_out, float p,
                     uint64_t seed, float* keep, float* out, eg_stream_t stream) {
    if (!y || !x || !keep || !out) return set_error(EG_ERR_ARG, "y, x, keep and out must not be NULL");
    if (out == x || out == y) return set_error(EG_ERR_ARG, "out must not alias an input");
    if (!(p >= 0.f && p < 1.f)) return set_error(EG_ERR_ARG, "dropout p must be in [0, 1)");
    if (const int rc = em_check_shapes(batch, c_in, c_out, side)) return rc;
    if (const int rc = em_check_residual(w1, b1, c_in, c_out)) return rc;
    if (const int rc = eg_epoch_required(p)) return rc;
    const long long total = (long long)batch * side * side;
    const EmAct A{y, x, w1, b1, keep, out, eg_epoch_ptr(), (unsigned long long)seed, total, p, p > 0.f ? 1.0f / (1.0f - p) : 1.0f,
                  c_in, c_out, side * side};
    hipLaunchKernelGGL(k_embed_act_fwd, dim3((unsigned)em_blocks(total), (unsigned)c_out), dim3(EM_THREADS), 0, (hipStream_t)stream, A);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

int eg_embed_act_bwd(const float* dout, const float* out, const float* keep, const float* x, const float* z, const float* save_mean,
                     const float* save_invstd, const float* gamma, int batch, int c_in, int c_out, int side, void* workspace, float* ds,
                     float* dz, float* dgamma, float* dbeta, float* db3, float* db1, float* dw1, eg_stream_t stream) {
    if (!dout || !out || !keep || !x || !z || !save_mean || !save_invstd || !workspace || !ds || !dz)
        return set_error(EG_ERR_ARG, "dout, out, keep, x, z, save_mean, save_invstd, workspace, ds and dz must not be NULL");
    if (ds == dout || ds == out || ds == x || ds == z || dz == dout || dz == out || dz == x || dz == z || dz == ds)
        return set_error(EG_ERR_ARG, "ds and dz must not alias an input or each other");
    if (const int rc = em_check_shapes(batch, c_in, c_out, side)) return rc;
    const long long n = (long long)batch * side * side;
    const int T = em_terms(n), chunks = em_chunks(n), Q = c_out * (1 + c_in);
    float2* part = (float2*)workspace;
    float* slices = (float*)((char*)workspace + em_part_bytes(batch, c_out, side));
    const EmBwd A{dout, out, keep, x, z, save_mean, save_invstd, gamma, ds, dz, part, slices, dgamma, dbeta, db1, n,
                  c_in, c_out, side * side, T, Q, dw1 ? 1 : 0};
    const dim3 grid((unsigned)chunks, (unsigned)c_out);
    hipLaunchKernelGGL(k_embed_bwd_sums, grid, dim3(EM_THREADS), 0, (hipStream_t)stream, A);
    hipLaunchKernelGGL(k_embed_bwd_apply, grid, dim3(EM_THREADS), 0, (hipStream_t)stream, A);
    if (db3 || dw1) {
        const int q_lo = db3 ? 0 : c_out, q_hi = dw1 ? Q : c_out;
        hipLaunchKernelGGL(k_embed_sum_slices, dim3((unsigned)((q_hi - q_lo + ES_OUT - 1) / ES_OUT)), dim3(EM_THREADS), 0,
                           (hipStream_t)stream, slices, (long long)chunks, Q, q_lo, q_hi, c_out, db3, dw1);
    }
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

int eg_embed_res_bwd_input(const float* ds, const float* w1, int batch, int c_in, int c_out, int side, float* dx, eg_stream_t stream) {
    if (!ds || !dx) return set_error(EG_ERR_ARG, "ds and dx must not be NULL");
    if (dx == ds) return set_error(EG_ERR_ARG, "dx must not alias ds");
    if (const int rc = em_check_shapes(batch, c_in, c_out, side)) return rc;
    if (const int rc = em_check_residual(w1, nullptr, c_in, c_out)) return rc;
    const long long total = (long long)batch * side * side;
    hipLaunchKernelGGL(k_embed_res_bwd_input, dim3((unsigned)em_blocks(total), (unsigned)c_in), dim3(EM_THREADS), 0, (hipStream_t)stream,
                       ds, w1, total, c_in, c_out, side * side, dx);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

}  // extern "C"
