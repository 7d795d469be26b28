// The UNet tail and the 4 classifier heads in one gfx950 kernel: the no-GNN baselines' whole path behind the decoder.
// Replaces reference src/core/models.py:759-799 / :802-838 behind create_node_pixels' decoder: `F.relu(self.linears[i](f))` of
// every level (:707-710), the permute / cat into node rows (:726-756), h[node_type == 0] and the 4 x nn.Sequential + torch.cat.
// Composed from eg_conv1x1_relu_pack_levels and eg_classifier_fwd that is two launches with the node-major [B * N, 128] rows
// (36.9 MB per 224 x 224 frame) written and read back in between.  With no GNN layer between tail and heads a row never has to
// leave the workgroup: a tile of 64 positions of one (frame, level) goes from decoder-map channels to four logits here.
//
//   tail   the [C_l -> 128] product of k_conv1x1_relu_pack (pack.hip) in ITS order of summation -- accumulator from 0, input
//          channels ascending, one FMA each, bias added after the sum, then ReLU -- on plain FMAs from LDS (118 MFLOP per frame:
//          not matrix-unit work), 16 threads more per position than there; the result goes into the heads' LDS tile.
//   heads  the body of k_classifier (classifier.hip), instruction for instruction.
// Both stages are row-independent and keep their orders, so the logits are bit-identical to the two launches'.  The rows the
// node-type filter drops (connection rows in front of the levels, coordinate rows behind them) are never computed: no row_lo.
#include "tile.h"

namespace eg {

constexpr int PK_MAX_LEVELS = 16;          // as pack.hip
constexpr int TH_THREADS = 512;
constexpr int TH_CC = 32;                  // input channels per pass through LDS (CP_CC of pack.hip: the chunking changes no order)

struct TailHeadsArgs {
    const float* feat[PK_MAX_LEVELS];      // [batch, cin_l, side_l, side_l]
    const float* w[PK_MAX_LEVELS];         // [128, cin_l]
    const float* bias[PK_MAX_LEVELS];      // [128] or NULL
    int cin[PK_MAX_LEVELS];
    int side[PK_MAX_LEVELS];
    int row0[PK_MAX_LEVELS];               // first logits row of the level inside a frame
    int tile0[PK_MAX_LEVELS + 1];          // prefix sum of 64-position tiles per level
    int n_levels, batch, n_rows, sigmoid;  // n_rows: logits rows per frame (sum of side_l^2)
};

__global__ __launch_bounds__(TH_THREADS, 4) void k_conv1x1_relu_heads(const TailHeadsArgs a, const float* __restrict__ w1,
                                                                      const float* __restrict__ s1, const float* __restrict__ t1,
                                                                      const float* __restrict__ w2, const float* __restrict__ s2,
                                                                      const float* __restrict__ t2, const float* __restrict__ w3,
                                                                      const float* __restrict__ b3, float* __restrict__ logits) {
    __shared__ __attribute__((aligned(16))) float s_a[TILE * LDA + 4];
    __shared__ __attribute__((aligned(16))) float s_out[TILE * 4];
    __shared__ __attribute__((aligned(16))) float s_f[TH_CC][TILE];
    __shared__ __attribute__((aligned(16))) float s_w[TH_CC][C + 4];
    __shared__ __attribute__((aligned(16))) float s_bn[2 * C + 3 * 64];      // s1, t1 | s2, t2, w3

    const int tid = threadIdx.x;
    const int lane_k = tid & 63;
    const int wave = wave_id();

    // ---- the heads' weight slices, in registers for the lifetime of the workgroup (k_classifier) ----
    float wreg[32];
    load_w_slice16(w1, wave, lane_k, 0, wreg);
    // The BatchNorm vectors and the last Linear's weights wait in LDS (k_classifier holds these 20 values per lane in registers;
    // beside the tail's accumulators and addresses that spilled): read back per tile, first use behind the tail's barriers.
    if (tid < C) { s_bn[tid] = s1[tid]; s_bn[C + tid] = t1[tid]; }
    else if (tid < C + 64) { const int i = tid - C; s_bn[2 * C + i] = s2[i]; s_bn[2 * C + 64 + i] = t2[i]; s_bn[2 * C + 128 + i] = w3[i]; }
    const int ch_d = 16 * wave + 4 * (lane_k >> 4);
    const int head = wave & 3, rhalf = wave >> 2;
    float w2a[8];
    {
        const f32x4* p = reinterpret_cast<const f32x4*>(w2 + (size_t)(head * 16 + (lane_k & 15)) * 32 + 8 * (lane_k >> 4));
        const f32x4 q0 = p[0], q1 = p[1];
        w2a[0] = q0.x; w2a[1] = q0.y; w2a[2] = q0.z; w2a[3] = q0.w; w2a[4] = q1.x; w2a[5] = q1.y; w2a[6] = q1.z; w2a[7] = q1.w;
    }
    const int o4h = head * 16 + 4 * (lane_k >> 4);
    const float b3v = b3[head];

    const int tiles_per_frame = a.tile0[a.n_levels];

    TileWalk walk(WALK_MOD8, tiles_per_frame * a.batch, nullptr, reinterpret_cast<int*>(&s_a[TILE * LDA]));
    int tile;
    while (walk.next(tile)) {
        int lane = lane_k;
        asm volatile("" : "+v"(lane));
        // tail: thread (o4 = tid & 31, ps = tid >> 5) holds output channels 4 o4 .. 4 o4 + 3 of positions ps, ps + 16, ps + 32, ps + 48
        // (derived per tile from the opaque lane: hoisted out of the walk, the tail's addresses cost the registers the heads need)
        const int o4 = lane & 31, ps = 2 * wave + (lane >> 5);
        const int frame = tile / tiles_per_frame, t = tile - frame * tiles_per_frame;
        int l = 0;
        for (int k = 1; k < a.n_levels; ++k) l += t >= a.tile0[k] ? 1 : 0;
        const int P = a.side[l] * a.side[l], cin = a.cin[l];
        const int pos0 = (t - a.tile0[l]) * TILE;
        const int npos = min(TILE, P - pos0);
        const float* __restrict__ src = a.feat[l] + (size_t)frame * cin * P + pos0;
        const float* __restrict__ wl = a.w[l];
        const bool vec = (P & 3) == 0;                                    // channel planes 16-B aligned: 16-B loads
        f32x4 acc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < cin; c0 += TH_CC) {
            const int cc = min(TH_CC, cin - c0);
            if (vec) {                                                    // 16 lanes x 16 B per channel plane run, 32 planes at once
                const int p4 = lane & 15, c = 4 * wave + (lane >> 4);
                if (c < cc) {
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    if (4 * p4 < npos) v = *reinterpret_cast<const f32x4*>(src + (size_t)(c0 + c) * P + 4 * p4);
                    *reinterpret_cast<f32x4*>(&s_f[c][4 * p4]) = v;
                }
            } else {
                for (int i = tid; i < cc * TILE; i += TH_THREADS) {
                    const int c = i >> 6, pp = i & 63;
                    s_f[c][pp] = pp < npos ? src[(size_t)(c0 + c) * P + pp] : 0.f;
                }
            }
            if (o4 < cc) {                                                // W[o][c0 + c] -> s_w[c][o]: 32 lanes = one row's pass
#pragma unroll
                for (int k = 0; k < C / 16; ++k) s_w[o4][ps + 16 * k] = wl[(size_t)(ps + 16 * k) * cin + c0 + o4];
            }
            __syncthreads();
#pragma unroll 4
            for (int c = 0; c < cc; ++c) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(&s_w[c][4 * o4]);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] += w * s_f[c][ps + 16 * k];
            }
            __syncthreads();
        }
        {   // bias after the sum, ReLU, into the heads' A tile: a half-wave writes one 512-B row (rows past npos: finite, unused)
            const float* __restrict__ bl = a.bias[l];
            const f32x4 bv = bl ? *reinterpret_cast<const f32x4*>(bl + 4 * o4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                f32x4 v = acc[k] + bv;
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                *reinterpret_cast<f32x4*>(&s_a[(ps + 16 * k) * LDA + 4 * o4]) = v;
            }
        }
        __syncthreads();
        // ---- heads: k_classifier from here on ----
        f32x4v hacc[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) hacc[b] = f32x4v{0.f, 0.f, 0.f, 0.f};
        mfma16_pair<false>(s_a, 0, lane, wreg, hacc[0], hacc[1]);
        if (npos > 32) mfma16_pair<false>(s_a, 32, lane, wreg, hacc[2], hacc[3]);
        __syncthreads();
        {   // hidden layer 1 (BN + ReLU) back into the tile: row j, channels 16w + 4q .. +3
            const int j = lane & 15, q4 = lane >> 4;
            const f32x4 s1v = *reinterpret_cast<const f32x4*>(&s_bn[ch_d]);
            const f32x4 t1v = *reinterpret_cast<const f32x4*>(&s_bn[C + ch_d]);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                f32x4v hv;
                hv.x = fmaxf(hacc[b].x * s1v.x + t1v.x, 0.f);
                hv.y = fmaxf(hacc[b].y * s1v.y + t1v.y, 0.f);
                hv.z = fmaxf(hacc[b].z * s1v.z + t1v.z, 0.f);
                hv.w = fmaxf(hacc[b].w * s1v.w + t1v.w, 0.f);
                *reinterpret_cast<f32x4v*>(&s_a[(16 * b + j) * LDA + 16 * wave + 4 * q4]) = hv;
            }
        }
        __syncthreads();
        // Linear(32,16) + BN + ReLU + Linear(16,1) for (head, 32-row half): K = 32 on the MFMA
        const f32x4 s2v = *reinterpret_cast<const f32x4*>(&s_bn[2 * C + o4h]);
        const f32x4 t2v = *reinterpret_cast<const f32x4*>(&s_bn[2 * C + 64 + o4h]);
        const f32x4 w3v = *reinterpret_cast<const f32x4*>(&s_bn[2 * C + 128 + o4h]);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const int row0 = 32 * rhalf + 16 * rb;
            const int j = lane & 15, kq = lane >> 4;
            const f32x4* hp = reinterpret_cast<const f32x4*>(&s_a[(row0 + j) * LDA + 32 * head + 8 * kq]);
            const f32x4 b0 = hp[0], b1 = hp[1];
            f32x4v z = {0.f, 0.f, 0.f, 0.f};
            z = __builtin_amdgcn_mfma_f32_16x16x4f32(w2a[0], b0.x, z, 0, 0, 0);
            z = __builtin_amdgcn_mfma_f32_16x16x4f32(w2a[1], b0.y, z, 0, 0, 0);
            z = __builtin_amdgcn_mfma_f32_16x16x4f32(w2a[2], b0.z, z, 0, 0, 0);
            z = __builtin_amdgcn_mfma_f32_16x16x4f32(w2a[3], b0.w, z, 0, 0, 0);
            z = __builtin_amdgcn_mfma_f32_16x16x4f32(w2a[4], b1.x, z, 0, 0, 0);
            z = __builtin_amdgcn_mfma_f32_16x16x4f32(w2a[5], b1.y, z, 0, 0, 0);
            z = __builtin_amdgcn_mfma_f32_16x16x4f32(w2a[6], b1.z, z, 0, 0, 0);
            z = __builtin_amdgcn_mfma_f32_16x16x4f32(w2a[7], b1.w, z, 0, 0, 0);
            float y = w3v.x * fmaxf(z.x * s2v.x + t2v.x, 0.f) + w3v.y * fmaxf(z.y * s2v.y + t2v.y, 0.f) +
                      w3v.z * fmaxf(z.z * s2v.z + t2v.z, 0.f) + w3v.w * fmaxf(z.w * s2v.w + t2v.w, 0.f);
            y += __shfl_xor(y, 16);
            y += __shfl_xor(y, 32);
            y += b3v;
            if (a.sigmoid) y = 1.0f / (1.0f + __expf(-y));
            if (kq == 0) s_out[(row0 + j) * 4 + head] = y;
        }
        __syncthreads();
        if (tid < npos)
            *reinterpret_cast<f32x4*>(logits + ((size_t)frame * a.n_rows + a.row0[l] + pos0 + tid) * 4) =
                *reinterpret_cast<const f32x4*>(&s_out[tid * 4]);
    }
}

static inline bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace eg

using namespace eg;

extern "C" int eg_conv1x1_relu_heads_fwd(const float* const* level_feats, const float* const* level_weights,
                                         const float* const* level_biases, const int* level_channels, const int* level_side,
                                         int n_levels, int batch, const float* w1, const float* s1, const float* t1, const float* w2,
                                         const float* s2, const float* t2, const float* w3, const float* b3, int sigmoid, float* logits,
                                         eg_stream_t stream) {
    if (!level_feats || !level_weights || !level_channels || !level_side || !w1 || !s1 || !t1 || !w2 || !s2 || !t2 || !w3 || !b3 || !logits)
        return set_error(EG_ERR_ARG, "NULL argument");
    if (misaligned16(logits)) return set_error(EG_ERR_ARG, "logits must be 16-byte aligned");
    if (n_levels < 1 || n_levels > PK_MAX_LEVELS || batch < 1) return set_error(EG_ERR_ARG, "bad argument");
    TailHeadsArgs a{};
    a.n_levels = n_levels; a.batch = batch; a.sigmoid = sigmoid;
    int64_t row = 0, tiles = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (!level_feats[l] || !level_weights[l] || level_side[l] < 1 || level_channels[l] < 1)
            return set_error(EG_ERR_ARG, "NULL level map / weight or bad side / channel count");
        const int64_t P = (int64_t)level_side[l] * level_side[l];
        if (((P & 3) == 0 && misaligned16(level_feats[l])) || (level_biases && level_biases[l] && misaligned16(level_biases[l])))
            return set_error(EG_ERR_ARG, "level features with side * side % 4 == 0 and every bias must be 16-byte aligned");
        if (P >= (1ll << 31) || (row + P) * (int64_t)batch >= (1ll << 31)) return set_error(EG_ERR_ARG, "batch * rows exceeds int32");
        a.feat[l] = level_feats[l]; a.w[l] = level_weights[l]; a.bias[l] = level_biases ? level_biases[l] : nullptr;
        a.cin[l] = level_channels[l]; a.side[l] = level_side[l]; a.row0[l] = (int)row; a.tile0[l] = (int)tiles;
        row += P;
        tiles += (P + TILE - 1) / TILE;
    }
    a.n_rows = (int)row;
    a.tile0[n_levels] = (int)tiles;
    long long n_tiles = (long long)tiles * batch;                 // (< 2^31: no level has more tiles than rows)
    long long g = n_tiles < 512 ? n_tiles : 512;                  // 2 resident 8-wave workgroups per CU
    g = (g + 7) / 8 * 8;
    hipLaunchKernelGGL(k_conv1x1_relu_heads, dim3((unsigned)g), dim3(TH_THREADS), 0, (hipStream_t)stream, a, w1, s1, t1, w2, s2, t2,
                       w3, b3, logits);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}
