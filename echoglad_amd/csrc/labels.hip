// Dense node labels from landmark coordinates: the reference's create_node_labels (src/core/datasets.py:1586-1612) on the
// device.  A frame's labels y [n_rows, 4] and valid_labels [n_rows, 4] (1.15 MB each at 224/7) carry eight integers and four
// flags; the host path builds them with numpy per landmark and level and pushes them through a pageable copy every step.  Here
// the batch brings coords [batch, 4, 2] (h, w) and valid4 [batch, 4] and ONE launch writes both dense tensors.
//
// Rules (include/echoglad_hip.h, eg_node_labels): level l of side p occupies rows start[l] .. + p * p of a frame, row-major
// (i, j); channel c of row start[l] + i * p + j is 1 iff (i, j) == (bin(h), bin(w)) of landmark c, where
//     aux levels (all but the last)   bin(v) = v * p / F  for 0 <= v < F,   p - 1  for -F <= v < 0
//     the last level (side == F)      bin(v) = v          for 0 <= v < F,   v + F  for -F <= v < 0
// (numpy's digitize against linspace(0, F, p + 1), and its wrap-around of a negative index).  A landmark with h or w outside
// [-F, F) has no 1 on any level.  Rows outside every level are 0.
//
// A workgroup owns NL_ROWS consecutive rows of one frame.  Its first wave computes the 4 * n_levels target rows of the frame
// once and keeps those that fall into the workgroup's rows (relative to its first row) in LDS; a workgroup without one -- all but
// a handful -- stores zeros without looking at LDS again.  Every element is written once, by one 16-byte store per row and
// tensor; no fill pass, no atomics, no allocation, no synchronisation with the host.
#include "common.h"

namespace eg {

typedef float nl_f32x4 __attribute__((ext_vector_type(4)));

constexpr int NL_THREADS = 256;
constexpr int NL_UNROLL = 4;                            // rows per lane
constexpr int NL_ROWS = NL_THREADS * NL_UNROLL;         // rows per workgroup
constexpr int NL_MAX_LEVELS = 16;

struct NlLevels {
    int start[NL_MAX_LEVELS];
    int side[NL_MAX_LEVELS];
    int n_levels;
    int frame;
};

// the bin of one coordinate on a level of side p (last: the main grid), or -1 outside [-F, F)
__device__ inline int nl_bin(int v, int p, int F, bool last) {
    if (v >= F || v < -F) return -1;
    if (v < 0) return last ? v + F : p - 1;
    return last ? v : (int)(((long long)v * p) / F);
}

__global__ __launch_bounds__(NL_THREADS) void k_node_labels(const int* __restrict__ coords, const float* __restrict__ valid4,
                                                            long long n_rows, unsigned blocks_per_frame, const NlLevels L,
                                                            nl_f32x4* __restrict__ labels, nl_f32x4* __restrict__ valid) {
    __shared__ int s_tgt[4 * NL_MAX_LEVELS];           // target rows inside this workgroup's rows, relative to r0; -1: none
    const int t = threadIdx.x;
    const unsigned b = blockIdx.x / blocks_per_frame;
    const long long r0 = (long long)(blockIdx.x - b * blocks_per_frame) * NL_ROWS;
    const long long left = n_rows - r0;
    const int cnt = left < NL_ROWS ? (int)left : NL_ROWS;       // rows of this workgroup (>= 1 by the grid's size)
    const int n_tgt = 4 * L.n_levels;
    int hit = 0;
    if (t < n_tgt) {
        const int l = t >> 2, c = t & 3;
        int start = 0, side = 1;
#pragma unroll
        for (int k = 0; k < NL_MAX_LEVELS; ++k)                  // (a select chain: no dynamic index into the kernel argument)
            if (k == l) { start = L.start[k]; side = L.side[k]; }
        const bool last = l == L.n_levels - 1;
        const int* hw = coords + ((size_t)b * 4 + c) * 2;
        const int bh = nl_bin(hw[0], side, L.frame, last), bw = nl_bin(hw[1], side, L.frame, last);
        int rel = -1;
        if (bh >= 0 && bw >= 0) {
            const long long d = (long long)start + (long long)bh * side + bw - r0;
            if (d >= 0 && d < cnt) { rel = (int)d; hit = 1; }
        }
        s_tgt[t] = rel;
    }
    const int any = __syncthreads_or(hit);
    nl_f32x4 vv = {1.f, 1.f, 1.f, 1.f};
    if (valid4) {
        const float* v = valid4 + (size_t)b * 4;
        vv = nl_f32x4{v[0], v[1], v[2], v[3]};
    }
    const long long base = (long long)b * n_rows + r0;
#pragma unroll
    for (int u = 0; u < NL_UNROLL; ++u) {
        const int r = u * NL_THREADS + t;
        if (r >= cnt) break;
        nl_f32x4 y = {0.f, 0.f, 0.f, 0.f};
        if (any) {
            for (int k = 0; k < n_tgt; k += 4) {                 // one level: channels 0 .. 3
                y.x = s_tgt[k + 0] == r ? 1.f : y.x;
                y.y = s_tgt[k + 1] == r ? 1.f : y.y;
                y.z = s_tgt[k + 2] == r ? 1.f : y.z;
                y.w = s_tgt[k + 3] == r ? 1.f : y.w;
            }
        }
        labels[base + r] = y;
        if (valid) valid[base + r] = vv;
    }
}

}  // namespace eg

using namespace eg;

extern "C" {

int eg_node_labels(const int* coords, const float* valid4, int batch, int64_t n_rows, const int* level_start, const int* level_side,
                   int n_levels, int frame_size, float* labels, float* valid, eg_stream_t stream) {
    if (batch < 1) return set_error(EG_ERR_ARG, "batch must be >= 1");
    if (n_levels < 1 || n_levels > NL_MAX_LEVELS) return set_error(EG_ERR_ARG, "n_levels must be in 1 .. 16");
    if (!level_start || !level_side) return set_error(EG_ERR_ARG, "level_start and level_side must not be NULL");
    if (n_rows < 1 || frame_size < 1) return set_error(EG_ERR_ARG, "n_rows and frame_size must be >= 1");
    NlLevels L{};
    L.n_levels = n_levels;
    L.frame = frame_size;
    for (int l = 0; l < n_levels; ++l) {
        const long long sz = (long long)level_side[l] * level_side[l];
        if (level_side[l] < 1 || level_start[l] < 0 || level_start[l] + sz > n_rows)
            return set_error(EG_ERR_ARG, "level " + std::to_string(l) + " does not fit in n_rows");
        L.start[l] = level_start[l];
        L.side[l] = level_side[l];
    }
    if (level_side[n_levels - 1] != frame_size)
        return set_error(EG_ERR_ARG, "the last level is the main grid: its side must equal frame_size");
    if (!coords || !labels) return set_error(EG_ERR_ARG, "coords and labels must not be NULL");
    if (((uintptr_t)labels | (uintptr_t)valid) % 16 || (uintptr_t)coords % 4 || (uintptr_t)valid4 % 4)
        return set_error(EG_ERR_ARG, "labels / valid must be 16-byte aligned, coords / valid4 4-byte aligned");
    const long long blocks_per_frame = (n_rows + NL_ROWS - 1) / NL_ROWS;
    if (blocks_per_frame * batch >= (1ll << 31)) return set_error(EG_ERR_ARG, "batch * n_rows too large for one launch");
    hipLaunchKernelGGL(k_node_labels, dim3((unsigned)(blocks_per_frame * batch)), dim3(NL_THREADS), 0, (hipStream_t)stream, coords,
                       valid4, (long long)n_rows, (unsigned)blocks_per_frame, L, (nl_f32x4*)labels, (nl_f32x4*)valid);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

}  // extern "C"
