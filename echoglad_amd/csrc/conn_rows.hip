// Connection-node features: the first n_conn rows of every frame of the node array [batch * n_rows, 128] are column means over
// row ranges of the SAME array (a level's packed rows), taken in place right behind the packing launch (gfx950).
// Replaces `map.mean(dim=(2, 3))` per level + an indexed assignment into a clone of the node array (reference
// src/core/models.py:524-533, :737-752): nothing is read but the node rows themselves, nothing is written but the n_conn rows.
//
// THE ORDER OF SUMMATION is a function of a source's row count alone (eg_conn_rows_plan):
//   rows_per_chunk = max(128, ceil(rows / 512)),  chunks = ceil(rows / rows_per_chunk)  (<= 512; the last chunk may be short).
//   Chunk k holds rows [k * rpc, min(rows, (k + 1) * rpc)) of the source.  One workgroup sums it: row lane h = 0 .. 7 (a half-wave,
//   one 512-B row per access) adds rows h, h + 8, h + 16, .. of the chunk, ascending, to 0; the 8 lane sums are then added
//   ascending, ((s0 + s1) + s2) + .. + s7.  A source of ONE chunk is divided by (float)rows there and stored.  Otherwise the chunk
//   sums go to the workspace and a second launch adds them ascending, (p0 + p1) + p2 + .., and divides.
//   Longest chain of additions: d(rows) = (ceil(min(rows, rpc) / 8) - 1) + 7 + (chunks - 1).
// No atomics, no flags, no fences between workgroups: the kernel boundary is the only ordering.  A frame's bits do not depend on
// the batch, the grid, the device or the other sources of the call.  Equal sources are summed once and stored to every row that
// names them.
//
// THE BACKWARD, in place on d_nodes: for every distinct source range, t = sum over the connection rows j that name it, j ascending,
// of d_nodes[b, j, c] * inv_j with inv_j = 1.0f / (float)rows_j taken ON THE HOST in fp32; the first product starts the sum, every
// further one is a rounded multiply followed by a rounded add (no fused multiply-add); then d_nodes[b, base + i, c] += t, one
// rounded add per element.  One launch.  The connection rows are only read.
#include "common.h"

namespace eg {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CR_MAX = 16;                // connection rows per frame
constexpr int CR_THREADS = 256;
constexpr int CR_LANES = CR_THREADS / 32; // row lanes: half-waves, one 512-B row each
constexpr int CR_MIN_RPC = 128;
constexpr int CR_MAX_CHUNKS = 512;

struct ConnRowsArgs {
    long long base[CR_MAX];               // distinct sources: first row inside a frame, rows
    long long rows[CR_MAX];
    long long ws0[CR_MAX];                // first partial row of the source inside a frame's workspace slice (-1: one chunk, none)
    int chunk0[CR_MAX + 1];               // prefix sum of the sources' chunks
    int rpc[CR_MAX];
    int multi[CR_MAX];                    // the sources of more than one chunk
    unsigned targets[CR_MAX];             // bit j: connection row j names this source
    float inv[CR_MAX];                    // per connection row: 1.0f / rows (backward)
    int n_src, n_multi, n_conn;
    long long n_rows, ws_rows;            // rows per frame of the node array / of the workspace
};

static void plan(long long rows, int& chunks, int& rpc) {
    const long long r = (rows + CR_MAX_CHUNKS - 1) / CR_MAX_CHUNKS;
    rpc = (int)(r > CR_MIN_RPC ? r : CR_MIN_RPC);
    chunks = (int)((rows + rpc - 1) / rpc);
}

__device__ __forceinline__ void store_targets(const ConnRowsArgs& a, int u, long long frame_row0, int q, f32x4 tot, float* nodes) {
    const float n = (float)a.rows[u];
    tot.x = tot.x / n; tot.y = tot.y / n; tot.z = tot.z / n; tot.w = tot.w / n;
    const unsigned mask = a.targets[u];
    for (int j = 0; j < a.n_conn; ++j)
        if (mask >> j & 1u) *reinterpret_cast<f32x4*>(nodes + (size_t)(frame_row0 + j) * C + 4 * q) = tot;
}

// workgroup = (frame, source, chunk)
__global__ __launch_bounds__(CR_THREADS) void k_conn_rows_sum(const ConnRowsArgs a, float* nodes, float* ws) {
    __shared__ f32x4 s[CR_LANES][32];
    const int per_frame = a.chunk0[a.n_src];
    const int b = blockIdx.x / per_frame, t = blockIdx.x - b * per_frame;
    int u = 0;
    for (int k = 1; k < a.n_src; ++k) u += t >= a.chunk0[k] ? 1 : 0;
    const int k = t - a.chunk0[u];
    const int rpc = a.rpc[u];
    const long long r0 = (long long)k * rpc, left = a.rows[u] - r0;
    const int m = (int)(left < rpc ? left : rpc);
    const int tid = threadIdx.x, h = tid >> 5, q = tid & 31;
    const long long frame_row0 = (long long)b * a.n_rows;
    const float* src = nodes + (size_t)(frame_row0 + a.base[u] + r0) * C + 4 * q;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int r = h; r < m; r += CR_LANES) acc += *reinterpret_cast<const f32x4*>(src + (size_t)r * C);
    s[h][q] = acc;
    __syncthreads();
    if (h == 0) {
        f32x4 tot = s[0][q];
#pragma unroll
        for (int i = 1; i < CR_LANES; ++i) tot += s[i][q];
        if (a.ws0[u] < 0) store_targets(a, u, frame_row0, q, tot, nodes);
        else *reinterpret_cast<f32x4*>(ws + (size_t)((long long)b * a.ws_rows + a.ws0[u] + k) * C + 4 * q) = tot;
    }
}

// workgroup = (frame, source of more than one chunk); the lower half-wave adds the chunk sums ascending
__global__ __launch_bounds__(64) void k_conn_rows_finish(const ConnRowsArgs a, float* nodes, const float* ws) {
    const int b = blockIdx.x / a.n_multi, u = a.multi[blockIdx.x - b * a.n_multi];
    const int q = threadIdx.x;
    if (q >= 32) return;
    const int chunks = a.chunk0[u + 1] - a.chunk0[u];
    const float* p = ws + (size_t)((long long)b * a.ws_rows + a.ws0[u]) * C + 4 * q;
    f32x4 tot = *reinterpret_cast<const f32x4*>(p);
#pragma unroll 8
    for (int k = 1; k < chunks; ++k) tot += *reinterpret_cast<const f32x4*>(p + (size_t)k * C);
    store_targets(a, u, (long long)b * a.n_rows, q, tot, nodes);
}

// workgroup = (frame, source, chunk): the same cut as the forward, the rows of a chunk spread over the 8 row lanes
__global__ __launch_bounds__(CR_THREADS) void k_conn_rows_bwd(const ConnRowsArgs a, float* d_nodes) {
    const int per_frame = a.chunk0[a.n_src];
    const int b = blockIdx.x / per_frame, t = blockIdx.x - b * per_frame;
    int u = 0;
    for (int k = 1; k < a.n_src; ++k) u += t >= a.chunk0[k] ? 1 : 0;
    const int k = t - a.chunk0[u];
    const int rpc = a.rpc[u];
    const long long r0 = (long long)k * rpc, left = a.rows[u] - r0;
    const int m = (int)(left < rpc ? left : rpc);
    const int tid = threadIdx.x, h = tid >> 5, q = tid & 31;
    const long long frame_row0 = (long long)b * a.n_rows;
    const unsigned mask = a.targets[u];
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    bool first = true;
    for (int j = 0; j < a.n_conn; ++j) {
        if (!(mask >> j & 1u)) continue;
        const f32x4 v = *reinterpret_cast<const f32x4*>(d_nodes + (size_t)(frame_row0 + j) * C + 4 * q);
        const float w = a.inv[j];
        const f32x4 pr = {__fmul_rn(v.x, w), __fmul_rn(v.y, w), __fmul_rn(v.z, w), __fmul_rn(v.w, w)};
        g = first ? pr : f32x4{__fadd_rn(g.x, pr.x), __fadd_rn(g.y, pr.y), __fadd_rn(g.z, pr.z), __fadd_rn(g.w, pr.w)};
        first = false;
    }
    float* dst = d_nodes + (size_t)(frame_row0 + a.base[u] + r0) * C + 4 * q;
#pragma unroll 4
    for (int r = h; r < m; r += CR_LANES) {
        f32x4 v = *reinterpret_cast<f32x4*>(dst + (size_t)r * C);
        v = f32x4{__fadd_rn(v.x, g.x), __fadd_rn(v.y, g.y), __fadd_rn(v.z, g.z), __fadd_rn(v.w, g.w)};
        *reinterpret_cast<f32x4*>(dst + (size_t)r * C) = v;
    }
}

// the level table, checked and folded into distinct sources; every refusal comes before any launch
static int fill_conn_rows(const void* nodes, int batch, int64_t n_rows, int n_conn, const int64_t* src_base, const int64_t* src_rows,
                          ConnRowsArgs& a) {
    if (!nodes || !src_base || !src_rows) return set_error(EG_ERR_ARG, "NULL argument");
    if (((uintptr_t)nodes & 15) != 0) return set_error(EG_ERR_ARG, "the node array must be 16-byte aligned");
    if (n_conn < 1 || batch < 1 || n_rows < 1) return set_error(EG_ERR_ARG, "bad argument: n_conn, batch and n_rows are at least 1");
    if (n_conn > CR_MAX) return set_error(EG_ERR_UNSUPPORTED, "at most 16 connection rows per frame");
    if (n_rows * (int64_t)batch >= (1ll << 31)) return set_error(EG_ERR_UNSUPPORTED, "batch * rows exceeds int32");
    a.n_conn = n_conn; a.n_rows = n_rows; a.n_src = 0; a.n_multi = 0; a.ws_rows = 0;
    int chunks_total = 0;
    for (int j = 0; j < n_conn; ++j) {
        const int64_t base = src_base[j], rows = src_rows[j];
        if (rows < 1) return set_error(EG_ERR_ARG, "a source range needs at least one row");
        if (base < n_conn) return set_error(EG_ERR_ARG, "a source range touches the connection rows");
        if (base > n_rows - rows) return set_error(EG_ERR_ARG, "a source range ends past the frame's rows");
        a.inv[j] = 1.0f / (float)rows;
        int u = 0;
        for (; u < a.n_src; ++u) {
            if (a.base[u] == base && a.rows[u] == rows) break;
            if (base < a.base[u] + a.rows[u] && a.base[u] < base + rows)
                return set_error(EG_ERR_ARG, "source ranges must be equal or disjoint");
        }
        if (u == a.n_src) {
            int chunks, rpc;
            plan(rows, chunks, rpc);
            a.base[u] = base; a.rows[u] = rows; a.rpc[u] = rpc; a.targets[u] = 0; a.chunk0[u] = chunks_total;
            a.ws0[u] = -1;
            if (chunks > 1) { a.ws0[u] = a.ws_rows; a.ws_rows += chunks; a.multi[a.n_multi++] = u; }
            chunks_total += chunks;
            ++a.n_src;
        }
        a.targets[u] |= 1u << j;
    }
    a.chunk0[a.n_src] = chunks_total;
    return EG_OK;
}

}  // namespace eg

using namespace eg;

extern "C" {

int eg_conn_rows_plan(int64_t rows, int* chunks, int* rows_per_chunk) {
    if (!chunks || !rows_per_chunk || rows < 1 || rows >= (1ll << 31)) return set_error(EG_ERR_ARG, "bad argument");
    plan(rows, *chunks, *rows_per_chunk);
    return EG_OK;
}

size_t eg_conn_rows_workspace_bytes(const int64_t* src_base, const int64_t* src_rows, int n_conn, int batch, int64_t n_rows) {
    ConnRowsArgs a{};
    alignas(16) static const float probe[4] = {0.f, 0.f, 0.f, 0.f};       // (stands in for the node array: only the table is looked at)
    if (fill_conn_rows(probe, batch, n_rows, n_conn, src_base, src_rows, a) != EG_OK) return 0;
    return (size_t)batch * (size_t)a.ws_rows * C * sizeof(float);
}

int eg_conn_rows_fwd(float* nodes, int batch, int64_t n_rows, int n_conn, const int64_t* src_base, const int64_t* src_rows,
                     void* workspace, eg_stream_t stream) {
    ConnRowsArgs a{};
    int rc = fill_conn_rows(nodes, batch, n_rows, n_conn, src_base, src_rows, a);
    if (rc != EG_OK) return rc;
    if (a.n_multi > 0 && (!workspace || ((uintptr_t)workspace & 15) != 0))
        return set_error(EG_ERR_ARG, "a source of more than one chunk needs the workspace (16-byte aligned)");
    hipLaunchKernelGGL(k_conn_rows_sum, dim3((unsigned)((int64_t)batch * a.chunk0[a.n_src])), dim3(CR_THREADS), 0, (hipStream_t)stream,
                       a, nodes, (float*)workspace);
    EG_HIP_TRY(hipGetLastError());
    if (a.n_multi > 0) {
        hipLaunchKernelGGL(k_conn_rows_finish, dim3((unsigned)(batch * a.n_multi)), dim3(64), 0, (hipStream_t)stream, a, nodes,
                           (const float*)workspace);
        EG_HIP_TRY(hipGetLastError());
    }
    return EG_OK;
}

int eg_conn_rows_bwd(float* d_nodes, int batch, int64_t n_rows, int n_conn, const int64_t* src_base, const int64_t* src_rows,
                     eg_stream_t stream) {
    ConnRowsArgs a{};
    int rc = fill_conn_rows(d_nodes, batch, n_rows, n_conn, src_base, src_rows, a);
    if (rc != EG_OK) return rc;
    hipLaunchKernelGGL(k_conn_rows_bwd, dim3((unsigned)((int64_t)batch * a.chunk0[a.n_src])), dim3(CR_THREADS), 0, (hipStream_t)stream,
                       a, d_nodes);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

}  // extern "C"
