// Backward of the UNet tail, relu(conv1x1) fused into the node packing (k_conv1x1_relu_pack of pack.hip), for gfx950: no atomics,
// a fixed order of summation, nothing but launches on the caller's stream (capturable).
//
//   dz[b,pos,o] = d_nodes[row,o] where nodes[row,o] > 0, else 0      (the mask is the forward's own output: relu(s) > 0 <=> s > 0)
//   dF[b,c,pos] = sum_o W[o,c] dz[b,pos,o]                            one 128-term FMA chain, o ascending
//   dW[o,c]     = sum_{b,pos} dz[b,pos,o] f[b,c,pos]                  db[o] = sum_{b,pos} dz[b,pos,o]
//
// Products launch (k_tail_bwd): the forward's tiling, 64 consecutive positions of one (frame, level), 256 threads, input channels in
// passes of CP_CC = 32.  A workgroup owns one (level, slice, channel pass) and walks the tiles [slice * tps, (slice + 1) * tps) of
// the level's batch * ceil(P / 64) tiles, numbered frame-major, in ascending order.  Per tile it stages the masked dz tile (64 node
// rows of 512 B from d_nodes and from nodes, one row per half-wave: the forward's store pattern reversed) and the feature chunk in
// LDS -- both loaded into registers one tile ahead -- writes the dF chunk and adds the tile to its 128 x <= 32 block of dW, held in registers: positions ascending inside a tile,
// tiles ascending.  The pass-0 workgroup does the same for db.  After its last tile it stores the block into the workspace.
// Reduce launch (k_tail_bwd_reduce): dW_l and db_l from the slices; 16 runs of consecutive slices are summed in ascending order by
// 16 threads per element, then the 16 sums in ascending order.  The kernel boundary makes the partials visible.
//
// The plan: cap(c) = clamp(4096 / c, 16, 1024) slices at most for a level of c channels; tps = ceil(tiles / cap) tiles per slice,
// slices = ceil(tiles / tps) (the last slice may be short).  A function of (sides, channels, batch) alone, so the same inputs give
// the same bits on every run and every device.  At batch 1 the frame-sized default level (224 x 224, 4 channels: 784 tiles) gets
// 784 one-tile workgroups; d_nodes and nodes are read once for it (one channel pass).
// Workspace: level l owns S_l * 128 * (c_l + 1) floats, S_l = min(cap(c_l), tiles_l): [slices][128][c_l] partial dW, then at
// S_l * 128 * c_l [slices][128] partial db.  At most 2.62 MB per level up to 256 channels (1024 * 128 * 5 floats at c = 4) and
// 8 KiB * (c + 1) above, whatever the batch: 19.9 MB for the default dims (512 .. 4 channels).
#include <algorithm>

#include "common.h"

namespace eg {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TB_MAX_LEVELS = 16;          // PK_MAX_LEVELS of pack.hip
constexpr int TB_THREADS = 256;
constexpr int TB_POS = 64;                 // PK_POS
constexpr int TB_CC = 32;                  // CP_CC
constexpr int TB_LD = C + 4;               // row stride of the dz tile and of the transposed weights: 16-B rows, conflict-free b128 columns
constexpr int TB_RGROUPS = 16;             // the reduce launch: runs of slices per element

struct TailBwdArgs {
    const float* feat[TB_MAX_LEVELS];      // [batch, cin_l, side_l, side_l]; read where dW is wanted
    const float* w[TB_MAX_LEVELS];         // [128, cin_l]; read where dF is wanted
    float* dfeat[TB_MAX_LEVELS];           // NULL: not wanted
    float* part_w[TB_MAX_LEVELS];          // [slices][128][cin_l] in the workspace, NULL: dW not wanted
    float* part_b[TB_MAX_LEVELS];          // [slices][128], NULL: db not wanted
    int cin[TB_MAX_LEVELS];
    int side[TB_MAX_LEVELS];
    int row0[TB_MAX_LEVELS];               // first row of the level inside a frame
    int tpf[TB_MAX_LEVELS];                // tiles per frame
    int tiles[TB_MAX_LEVELS];              // batch * tpf
    int tps[TB_MAX_LEVELS];                // tiles per slice
    int passes[TB_MAX_LEVELS];             // channel passes that have work
    int blk0[TB_MAX_LEVELS + 1];           // prefix sum of slices * passes over the levels that want something
    int n_levels, n_rows;
};

// One channel pass over one tile whose dz and features are staged.  CCT = 4, 8 or 32 covers the pass's cc <= CCT channels (rows cc ..
// CCT - 1 of s_f and s_w are zero): dF thread (pos = tid & 63, wave wv) takes channels wv + 4 j, j < CCT / 4; dW thread
// (o = tid & 127, half h) takes channels h + 2 j, j < CCT / 2, so that 4 channels already keep every wave busy.
template <int CCT>
__device__ __forceinline__ void tile_products(const float (*s_dz)[TB_LD], const float (*s_f)[TB_POS], const float (*s_w)[TB_LD],
                                              int tid, int cc, int npos, float* __restrict__ df, int64_t P, bool want_part,
                                              float* acc, float& accb) {
    if (df) {
        constexpr int NJ = CCT / 4;
        const int pos = tid & 63, wv = tid >> 6;
        float a[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) a[j] = 0.f;
#pragma unroll 4
        for (int o4 = 0; o4 < C / 4; ++o4) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(&s_dz[pos][4 * o4]);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const f32x4 wq = *reinterpret_cast<const f32x4*>(&s_w[wv + 4 * j][4 * o4]);
                a[j] = fmaf(wq.x, d.x, a[j]); a[j] = fmaf(wq.y, d.y, a[j]); a[j] = fmaf(wq.z, d.z, a[j]); a[j] = fmaf(wq.w, d.w, a[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = wv + 4 * j;
            if (c < cc && pos < npos) df[(int64_t)c * P + pos] = a[j];
        }
    }
    if (want_part) {
        constexpr int NJ = CCT / 2;
        const int o = tid & 127, h = tid >> 7;
        const int n4 = (npos + 3) >> 2;                          // rows npos .. 63 of s_dz and columns npos .. 63 of s_f are zero
        for (int q = 0; q < n4; ++q) {
            const float d0 = s_dz[4 * q][o], d1 = s_dz[4 * q + 1][o], d2 = s_dz[4 * q + 2][o], d3 = s_dz[4 * q + 3][o];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const f32x4 f = *reinterpret_cast<const f32x4*>(&s_f[h + 2 * j][4 * q]);
                acc[j] = fmaf(d0, f.x, acc[j]); acc[j] = fmaf(d1, f.y, acc[j]); acc[j] = fmaf(d2, f.z, acc[j]); acc[j] = fmaf(d3, f.w, acc[j]);
            }
            accb += d0; accb += d1; accb += d2; accb += d3;
        }
    }
}

__global__ __launch_bounds__(TB_THREADS, 2) void k_tail_bwd(const TailBwdArgs a, const float* __restrict__ d_nodes,
                                                         const float* __restrict__ nodes) {
    __shared__ __attribute__((aligned(16))) float s_dz[TB_POS][TB_LD];
    __shared__ __attribute__((aligned(16))) float s_f[TB_CC][TB_POS];
    __shared__ __attribute__((aligned(16))) float s_w[TB_CC][TB_LD];
    int l = 0;
    for (int k = 1; k < a.n_levels; ++k) l += (int)blockIdx.x >= a.blk0[k] ? 1 : 0;
    const int idx = (int)blockIdx.x - a.blk0[l];
    const int passes = a.passes[l];
    const int slice = idx / passes, pass = idx - slice * passes;
    const int cin = a.cin[l], tpf = a.tpf[l];
    const int64_t P = (int64_t)a.side[l] * a.side[l];
    const int c0 = pass * TB_CC;
    const int cc = min(TB_CC, cin - c0);
    const int cct = cc <= 4 ? 4 : cc <= 8 ? 8 : TB_CC;
    const int tid = threadIdx.x;
    const float* __restrict__ fl = a.feat[l];
    const float* __restrict__ wl = a.w[l];
    float* __restrict__ dfl = a.dfeat[l];
    float* __restrict__ pw = a.part_w[l];
    float* __restrict__ pb = pass == 0 ? a.part_b[l] : nullptr;
    const bool want_part = pw != nullptr || pb != nullptr;
    const bool stage_f = pw != nullptr;
    const bool vec = (P & 3) == 0;

    if (dfl) {                                                        // W[o][c0 + c] -> s_w[c][o], rows cc .. cct - 1 zero
        for (int i = tid; i < C * cct; i += TB_THREADS) {
            const int o = i / cct, c = i - o * cct;
            s_w[c][o] = c < cc ? wl[(size_t)o * cin + c0 + c] : 0.f;
        }
    }
    if (!stage_f) {                                                   // db alone: the products run on zero features
        for (int i = tid; i < cct * TB_POS; i += TB_THREADS) s_f[i >> 6][i & 63] = 0.f;
    }
    float acc[TB_CC / 2], accb = 0.f;
#pragma unroll
    for (int j = 0; j < TB_CC / 2; ++j) acc[j] = 0.f;

    const int t_lo = slice * a.tps[l], t_hi = min(t_lo + a.tps[l], a.tiles[l]);
    const int q4 = tid & 31, r0 = tid >> 5;                           // node side: a half-wave = one 512-B row
    const int p4 = tid & 15, cr = tid >> 4;                           // feature side, 16-B route: 16 lanes x 16 B per channel plane run
    // the loads of a tile -- 8 rows of d_nodes and of nodes per half-wave, <= 8 feature values per thread -- go to registers and
    // are issued one tile ahead, behind the barrier that hands the current tile to the products: their latency runs under them
    f32x4 g[8], y[8];
    float fr[8];
    auto issue = [&](int T) {
        const int b = T / tpf, pos0 = (T - b * tpf) * TB_POS;
        const int npos = (int)min((int64_t)TB_POS, P - pos0);
        const size_t row = ((size_t)b * a.n_rows + a.row0[l] + pos0) * C + 4 * q4;
#pragma unroll
        for (int k = 0; k < 8; ++k) {                                 // every load is unconditional (rows, channels and positions
            const int r = min(r0 + 8 * k, npos - 1);                  // clamped into the tile): nothing waits for it before the
            g[k] = *reinterpret_cast<const f32x4*>(d_nodes + row + (size_t)r * C);      // products; what lies outside is zeroed when
            y[k] = *reinterpret_cast<const f32x4*>(nodes + row + (size_t)r * C);        // the registers go to LDS
        }
        if (stage_f) {                                                // features [cct][64]
            const float* __restrict__ src = fl + ((size_t)b * cin + c0) * P + pos0;
            if (vec) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int c = min(cr + 16 * k, cc - 1), pp = 4 * p4 < npos ? 4 * p4 : 0;
                    const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)c * P + pp);
                    fr[4 * k] = v.x; fr[4 * k + 1] = v.y; fr[4 * k + 2] = v.z; fr[4 * k + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int i = tid + TB_THREADS * k, c = min(i >> 6, cc - 1), pp = min(i & 63, npos - 1);
                    fr[k] = src[(size_t)c * P + pp];
                }
            }
        }
    };
    issue(t_lo);
    for (int T = t_lo; T < t_hi; ++T) {
        const int b = T / tpf, pos0 = (T - b * tpf) * TB_POS;
        const int npos = (int)min((int64_t)TB_POS, P - pos0);
        if (stage_f) {                                                // zero beyond cc and npos
            if (vec) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int c = cr + 16 * k;
                    const bool in = c < cc && 4 * p4 < npos;
                    if (c < cct)
                        *reinterpret_cast<f32x4*>(&s_f[c][4 * p4]) =
                            in ? f32x4{fr[4 * k], fr[4 * k + 1], fr[4 * k + 2], fr[4 * k + 3]} : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int i = tid + TB_THREADS * k, c = i >> 6, pp = i & 63;
                    if (c < cct) s_f[c][pp] = (c < cc && pp < npos) ? fr[k] : 0.f;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool in = r0 + 8 * k < npos;
            f32x4 v;
            v.x = in && y[k].x > 0.f ? g[k].x : 0.f; v.y = in && y[k].y > 0.f ? g[k].y : 0.f;
            v.z = in && y[k].z > 0.f ? g[k].z : 0.f; v.w = in && y[k].w > 0.f ? g[k].w : 0.f;
            *reinterpret_cast<f32x4*>(&s_dz[r0 + 8 * k][4 * q4]) = v;
        }
        __syncthreads();
        if (T + 1 < t_hi) issue(T + 1);
        float* df = dfl ? dfl + ((size_t)b * cin + c0) * P + pos0 : nullptr;
        if (cct == 4) tile_products<4>(s_dz, s_f, s_w, tid, cc, npos, df, P, want_part, acc, accb);
        else if (cct == 8) tile_products<8>(s_dz, s_f, s_w, tid, cc, npos, df, P, want_part, acc, accb);
        else tile_products<TB_CC>(s_dz, s_f, s_w, tid, cc, npos, df, P, want_part, acc, accb);
        __syncthreads();
    }
    const int o = tid & 127, h = tid >> 7;
    if (pw) {
        float* dst = pw + ((size_t)slice * C + o) * cin + c0;
#pragma unroll
        for (int j = 0; j < TB_CC / 2; ++j) {
            const int c = h + 2 * j;
            if (c < cc) dst[c] = acc[j];
        }
    }
    if (pb && h == 0) pb[(size_t)slice * C + o] = accb;
}

// dst[e] = sum over the n slices of src[s * stride + e]: thread (e = tid & 15, run = tid >> 4) sums the slices
// [run * q, (run + 1) * q), q = ceil(n / 16), in ascending order; run 0 then adds the 16 sums in ascending order.
struct TailReduceArgs {
    const float* src[2 * TB_MAX_LEVELS];
    float* dst[2 * TB_MAX_LEVELS];
    int count[2 * TB_MAX_LEVELS];          // elements, = the stride between slices
    int n[2 * TB_MAX_LEVELS];              // slices
    int blk0[2 * TB_MAX_LEVELS + 1];       // prefix sum of ceil(count / 16)
    int n_seg;
};

__global__ __launch_bounds__(TB_THREADS) void k_tail_bwd_reduce(const TailReduceArgs a) {
    __shared__ float s[TB_RGROUPS][17];
    int g = 0;
    for (int k = 1; k < a.n_seg; ++k) g += (int)blockIdx.x >= a.blk0[k] ? 1 : 0;
    const int tid = threadIdx.x, el = tid & 15, run = tid >> 4;
    const int e = ((int)blockIdx.x - a.blk0[g]) * 16 + el;
    const int count = a.count[g], n = a.n[g];
    const int q = (n + TB_RGROUPS - 1) / TB_RGROUPS;
    const int s_lo = min(run * q, n), s_hi = min(s_lo + q, n);
    float sum = 0.f;
    if (e < count) {
        const float* __restrict__ p = a.src[g] + (size_t)s_lo * count + e;
#pragma unroll 8
        for (int k = s_lo; k < s_hi; ++k, p += count) sum += *p;
    }
    s[run][el] = sum;
    __syncthreads();
    if (run == 0 && e < count) {
        float t = s[0][el];
#pragma unroll
        for (int k = 1; k < TB_RGROUPS; ++k) t += s[k][el];
        a.dst[g][e] = t;
    }
}

static inline bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

// ---- the plan: host arithmetic only --------------------------------------------------------------------------------------------
struct TailLevelPlan { int tpf, tiles, tps, slices, ws_slices; };

static inline int tail_bwd_cap(int channels) { return std::max(16, std::min(1024, 4096 / channels)); }

static bool tail_plan(const int* level_channels, const int* level_side, int n_levels, int batch, TailLevelPlan* plan) {
    if (!level_channels || !level_side || n_levels < 1 || n_levels > TB_MAX_LEVELS || batch < 1) return false;
    int64_t rows = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int c = level_channels[l], side = level_side[l];
        if (c < 1 || side < 1 || side > 46340) return false;
        const int64_t P = (int64_t)side * side;
        rows += P;
        if (rows * batch >= (1ll << 31)) return false;
        TailLevelPlan& p = plan[l];
        p.tpf = (int)((P + TB_POS - 1) / TB_POS);
        p.tiles = p.tpf * batch;
        const int cap = tail_bwd_cap(c);
        p.tps = (p.tiles + cap - 1) / cap;
        p.slices = (p.tiles + p.tps - 1) / p.tps;
        p.ws_slices = std::min(cap, p.tiles);
    }
    return true;
}

}  // namespace eg

using namespace eg;

extern "C" {

size_t eg_conv1x1_relu_pack_bwd_workspace_bytes(const int* level_channels, const int* level_side, int n_levels, int batch) {
    TailLevelPlan plan[TB_MAX_LEVELS];
    if (!tail_plan(level_channels, level_side, n_levels, batch, plan)) return 0;
    size_t floats = 0;
    for (int l = 0; l < n_levels; ++l) floats += (size_t)plan[l].ws_slices * C * ((size_t)level_channels[l] + 1);
    return floats * sizeof(float);
}

int eg_conv1x1_relu_pack_bwd_plan(const int* level_channels, const int* level_side, int n_levels, int batch, int* level_slices,
                                  int* level_tiles_per_slice) {
    TailLevelPlan plan[TB_MAX_LEVELS];
    if (!level_slices || !level_tiles_per_slice) return set_error(EG_ERR_ARG, "NULL argument");
    if (!tail_plan(level_channels, level_side, n_levels, batch, plan)) return set_error(EG_ERR_ARG, "shapes out of range");
    for (int l = 0; l < n_levels; ++l) { level_slices[l] = plan[l].slices; level_tiles_per_slice[l] = plan[l].tps; }
    return EG_OK;
}

int eg_conv1x1_relu_pack_bwd(const float* d_nodes, const float* nodes, const float* const* level_feats, const float* const* level_weights,
                             const int* level_channels, const int* level_side, int n_levels, int batch, int64_t n_rows,
                             int64_t row_offset, void* workspace, float* const* d_feats, float* const* d_weights,
                             float* const* d_biases, eg_stream_t stream) {
    if (!d_nodes || !nodes || !level_channels || !level_side) return set_error(EG_ERR_ARG, "NULL argument");
    if (n_levels < 1 || n_levels > TB_MAX_LEVELS || batch < 1 || n_rows < 1 || row_offset < 0) return set_error(EG_ERR_ARG, "bad argument");
    if (n_rows * (int64_t)batch >= (1ll << 31)) return set_error(EG_ERR_ARG, "batch * rows exceeds int32");
    if (misaligned16(d_nodes) || misaligned16(nodes)) return set_error(EG_ERR_ARG, "d_nodes and nodes must be 16-byte aligned");
    for (int l = 0; l < n_levels; ++l)
        if (level_side[l] < 1 || level_channels[l] < 1) return set_error(EG_ERR_ARG, "bad side / channel count");
    int64_t used = row_offset;
    for (int l = 0; l < n_levels; ++l) {
        used += (int64_t)level_side[l] * level_side[l];
        if (used > n_rows) return set_error(EG_ERR_ARG, "levels do not fit the frame's rows");
    }
    TailLevelPlan plan[TB_MAX_LEVELS];
    if (!tail_plan(level_channels, level_side, n_levels, batch, plan)) return set_error(EG_ERR_ARG, "shapes out of range");

    TailBwdArgs a{};
    TailReduceArgs r{};
    a.n_levels = n_levels; a.n_rows = (int)n_rows;
    int64_t row = row_offset;
    int blocks = 0, rblocks = 0;
    size_t ws_floats = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int c = level_channels[l];
        const int64_t P = (int64_t)level_side[l] * level_side[l];
        float* df = d_feats ? d_feats[l] : nullptr;
        float* dw = d_weights ? d_weights[l] : nullptr;
        float* db = d_biases ? d_biases[l] : nullptr;
        if (df && (!level_weights || !level_weights[l])) return set_error(EG_ERR_ARG, "a level's dF needs its weight");
        if (dw && (!level_feats || !level_feats[l])) return set_error(EG_ERR_ARG, "a level's dW needs its features");
        if ((P & 3) == 0 && ((level_feats && level_feats[l] && misaligned16(level_feats[l])) || (df && misaligned16(df))))
            return set_error(EG_ERR_ARG, "level features and dF with side * side % 4 == 0 must be 16-byte aligned");
        if ((dw || db) && !workspace) return set_error(EG_ERR_ARG, "dW / db need the workspace");
        const TailLevelPlan& p = plan[l];
        a.feat[l] = dw ? level_feats[l] : nullptr; a.w[l] = df ? level_weights[l] : nullptr; a.dfeat[l] = df;
        a.cin[l] = c; a.side[l] = level_side[l]; a.row0[l] = (int)row;
        a.tpf[l] = p.tpf; a.tiles[l] = p.tiles; a.tps[l] = p.tps;
        float* base = (float*)workspace + ws_floats;
        a.part_w[l] = dw ? base : nullptr;
        a.part_b[l] = db ? base + (size_t)p.ws_slices * C * c : nullptr;
        a.passes[l] = (df || dw) ? (c + TB_CC - 1) / TB_CC : (db ? 1 : 0);
        a.blk0[l] = blocks;
        blocks += p.slices * a.passes[l];
        if (dw) {
            r.src[r.n_seg] = a.part_w[l]; r.dst[r.n_seg] = dw; r.count[r.n_seg] = C * c; r.n[r.n_seg] = p.slices;
            r.blk0[r.n_seg++] = rblocks;
            rblocks += (C * c + 15) / 16;
        }
        if (db) {
            r.src[r.n_seg] = a.part_b[l]; r.dst[r.n_seg] = db; r.count[r.n_seg] = C; r.n[r.n_seg] = p.slices;
            r.blk0[r.n_seg++] = rblocks;
            rblocks += C / 16;
        }
        ws_floats += (size_t)p.ws_slices * C * ((size_t)c + 1);
        row += P;
    }
    a.blk0[n_levels] = blocks;
    r.blk0[r.n_seg] = rblocks;
    if (blocks == 0) return EG_OK;                                    // nothing is wanted: nothing is launched
    hipLaunchKernelGGL(k_tail_bwd, dim3((unsigned)blocks), dim3(TB_THREADS), 0, (hipStream_t)stream, a, d_nodes, nodes);
    EG_HIP_TRY(hipGetLastError());
    if (rblocks) {
        hipLaunchKernelGGL(k_tail_bwd_reduce, dim3((unsigned)rblocks), dim3(TB_THREADS), 0, (hipStream_t)stream, r);
        EG_HIP_TRY(hipGetLastError());
    }
    return EG_OK;
}

}  // extern "C"
