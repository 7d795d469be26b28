// Graph handles of the gfx950 hot-path library: closed-form topology, generic CSR, edge digest.
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <memory>
#include <vector>

#include "topo_tables.h"
#include <cstring>

namespace eg {

static thread_local std::string g_last_error;

int set_error(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define EG_NO_STREAM_YET ((void*)(intptr_t)-1)          // eg_graph::only_stream before the handle's first launch

static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

Knobs read_knobs() {
    Knobs k;
    // Two RUN-TIME knobs are left here, each selecting a fallback that has to exist anyway (include/echoglad_hip.h lists every run-time
    // variable).  What rounds 2 - 5 tuned through the environment is a compile-time constant now (-D to experiment): the winners
    // are the defaults and nobody lands on a losing route by accident.
    k.layer_impl = env_int("EG_LAYER_IMPL", -1);
    k.csr_tiles = env_int("EG_CSR_TILES", 2);
    k.layer_split = env_int("EG_LAYER_SPLIT", 1);
#ifndef EG_WALK_MODE
#define EG_WALK_MODE 0
#endif
#ifndef EG_STAGGER
#define EG_STAGGER 0
#endif
#ifndef EG_GRID
#define EG_GRID 512
#endif
#ifndef EG_PS_GRID
#define EG_PS_GRID 256
#endif
#ifndef EG_RING_GUARD
#define EG_RING_GUARD 1
#endif
#ifndef EG_QUEUE_SELF_RESET
#define EG_QUEUE_SELF_RESET 1
#endif
    k.walk_mode = EG_WALK_MODE;
    k.stagger = EG_STAGGER;
    k.grid_cap = EG_GRID;
    k.ps_grid = EG_PS_GRID;
    k.ring_guard = EG_RING_GUARD;
    k.queue_self_reset = EG_QUEUE_SELF_RESET != 0;
    // the static tile walk of the train forward labels chunks with blockIdx % 8 (a grid below 8 would leave chunks without
    // an owner) and its statistics partials fill at most 2048 slabs of the workspace
    if (k.ps_grid < 8) k.ps_grid = 8;
    if (k.ps_grid > 2048) k.ps_grid = 2048;
    if (k.grid_cap < 8) k.grid_cap = 8;
    if (k.grid_cap > 2048) k.grid_cap = 2048;
    return k;
}

const Knobs& process_knobs() {
    static const Knobs k = read_knobs();      // thread-safe one-time initialisation
    return k;
}

constexpr size_t QUEUE_RING_BYTES = sizeof(int) * ((size_t)QUEUE_SLOTS * QUEUE_SLICE_INTS + QUEUE_TAIL_INTS);

}  // namespace eg

// ---- the tile-queue ring of a handle (common.h) ---------------------------------------------------------------------------
// Every launch takes the next slice.  Slice s was last used by launch k - 64; if that launch ran on the same stream it is
// ordered in front of this one, and if it ran on another stream its event (or, for launches from the time when the handle had
// seen a single stream and recorded none, a query of that whole stream) tells whether it has finished.  A slice whose last
// user is still in flight on another stream is NOT handed out: the call fails with EG_ERR_UNSUPPORTED (the caller serialises,
// or uses a handle per stream).  Launches recorded into a HIP graph (stream capture) carry no event: a captured launch keeps its
// slice for every replay, which is ordered with later eager launches only on the replaying stream itself (header note).
int eg_graph::acquire_queue_slice(hipStream_t stream, int** slice, int* slot) const {
    const unsigned s = launch_seq.fetch_add(1u, std::memory_order_relaxed) % (unsigned)eg::QUEUE_SLOTS;
    // a handle that has only ever launched on ONE stream needs no events (its launches are ordered); the moment a second stream
    // shows up every launch records one.  Slices last used before that moment carry none: their stream is queried as a whole.
    // (the first launch publishes its stream with ONE compare-and-swap from the "none yet" sentinel, and any_launch only afterwards:
    //  a second thread can no longer see any_launch set while only_stream still reads as the legacy default stream)
    {
        void* none = EG_NO_STREAM_YET;
        only_stream.compare_exchange_strong(none, (void*)stream, std::memory_order_acq_rel);
        any_launch.store(1, std::memory_order_release);
    }
    // A capturing stream queries nothing (a query of another stream is not a capturable call, and the answer would describe the
    // moment of the capture, not of a replay): a captured launch is ordered with the handle's other users by the CALLER (header).
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    if (any_launch.load(std::memory_order_acquire) && !multi_stream.load(std::memory_order_acquire) &&
        only_stream.load(std::memory_order_acquire) != (void*)stream) {
        // A second stream shows up.  The launches so far carry no events.  If their stream is idle NOW they are all done and their
        // slices are simply free; otherwise ONE event recorded on it now lies behind all of them.  (Querying that stream as a
        // whole at every later reuse, as before, answers "not ready" for the legacy default stream whenever torch has parked a
        // cross-stream wait on it: a train step warmed up on a side stream after eager steps on the default stream was refused.)
        hipStream_t old = (hipStream_t)only_stream.load(std::memory_order_acquire);
        if (cap == hipStreamCaptureStatusNone) {
            if (hipStreamQuery(old) == hipSuccess) {
                for (int i = 0; i < eg::QUEUE_SLOTS; ++i) {
                    unsigned char two = 2;
                    slot_used[i].compare_exchange_strong(two, 0, std::memory_order_acq_rel);
                }
            } else {
                (void)hipGetLastError();
                if (era_event && hipEventRecord(era_event, old) == hipSuccess) era_recorded.store(1, std::memory_order_release);
                else (void)hipGetLastError();
            }
        }
        multi_stream.store(1, std::memory_order_release);
    }
    const unsigned char used = slot_used[s].load(std::memory_order_acquire);
    if (cap == hipStreamCaptureStatusNone && used && slot_stream[s].load(std::memory_order_acquire) != (void*)stream) {
        const hipError_t q = used == 1 ? hipEventQuery(slot_event[s])
                             : (era_recorded.load(std::memory_order_acquire) ? hipEventQuery(era_event)
                                                                             : hipStreamQuery((hipStream_t)slot_stream[s].load(std::memory_order_acquire)));
        if (q == hipErrorNotReady) {
            (void)hipGetLastError();
            return eg::set_error(EG_ERR_UNSUPPORTED, "more than 64 launches of this graph handle are in flight on different streams: "
                                                     "the tile-queue slice of the launch 64 calls ago is still in use");
        }
        if (q != hipSuccess) { (void)hipGetLastError(); }      // (a destroyed stream, an event never recorded: nothing in flight)
    }
    *slice = walk_counters + (size_t)s * eg::QUEUE_SLICE_INTS;
    *slot = (int)s;
    return EG_OK;
}

void eg_graph::commit_queue_slice(int slot, hipStream_t stream) const {
    if (slot < 0 || slot >= eg::QUEUE_SLOTS) return;
    if (!knobs.ring_guard) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    if (cs != hipStreamCaptureStatusNone) { slot_used[slot].store(0, std::memory_order_release); return; }
    slot_stream[slot].store((void*)stream, std::memory_order_release);
    if (!multi_stream.load(std::memory_order_acquire)) { slot_used[slot].store(2, std::memory_order_release); return; }
    if (hipEventRecord(slot_event[slot], stream) != hipSuccess) { (void)hipGetLastError(); slot_used[slot].store(2, std::memory_order_release); return; }
    slot_used[slot].store(1, std::memory_order_release);
}

namespace eg {

// queue ring of a fresh handle (still to be zeroed) and the events that guard it
static hipError_t alloc_queue_ring(eg_graph* g) {
    const hipError_t e = hipMalloc((void**)&g->walk_counters, QUEUE_RING_BYTES);
    if (e != hipSuccess) return e;
    for (int i = 0; i < QUEUE_SLOTS; ++i)
        if (hipEventCreateWithFlags(&g->slot_event[i], hipEventDisableTiming) != hipSuccess) return hipErrorOutOfMemory;
    if (hipEventCreateWithFlags(&g->era_event, hipEventDisableTiming) != hipSuccess) return hipErrorOutOfMemory;
    return hipSuccess;
}

// A handle under construction: whatever it has acquired when an error return drops it goes with it (~eg_graph).
static std::unique_ptr<eg_graph> new_handle(int kind, int64_t n_nodes) {
    std::unique_ptr<eg_graph> g(new eg_graph{});
    g->only_stream.store(EG_NO_STREAM_YET, std::memory_order_relaxed);
    g->kind = kind;
    g->knobs = read_knobs();
    g->n_nodes = n_nodes;
    return g;
}

// device copy of a host table; an empty table still gets `min_elems` elements
template <class T>
static hipError_t upload(T** dev, const std::vector<T>& v, size_t min_elems = 0) {
    const hipError_t e = hipMalloc((void**)dev, sizeof(T) * (v.size() > min_elems ? v.size() : min_elems));
    return (e != hipSuccess || v.empty()) ? e : hipMemcpy(*dev, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
}

// ---------------------------------------------------------------- CSR build
// transposed = 0: rows are targets (A_hat);  1: rows are sources (A_hat^T, the backward's adjacency of a directed graph)
__global__ void k_edge_keys(const int64_t* __restrict__ ei, int64_t n_edges, int n_nodes, int transposed, int* __restrict__ keys,
                            int* __restrict__ vals, int* __restrict__ counts) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    const int64_t src = ei[e], dst = ei[n_edges + e];
    const bool drop = (src == dst) || src < 0 || dst < 0 || src >= n_nodes || dst >= n_nodes;
    const int64_t row = transposed ? src : dst, col = transposed ? dst : src;
    keys[e] = drop ? n_nodes : (int)row;          // dropped edges sort behind every real row
    vals[e] = (int)col;
    if (!drop) atomicAdd(&counts[row], 1);        // integer: order-independent
}

__global__ void k_dis_from_counts(const int* __restrict__ counts, int n, float* __restrict__ dis) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dis[i] = 1.0f / sqrtf((float)(counts[i] + 1));
}

// ---------------------------------------------------------------- edge digest
__device__ inline unsigned long long mix64(unsigned long long r, unsigned long long c) {
    unsigned long long h = r * 0x9E3779B97F4A7C15ull + c * 0xC2B2AE3D27D4EB4Full + 0x165667B19E3779F9ull;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return h;
}

__global__ void k_edge_hash(const int64_t* __restrict__ ei, int64_t n_edges, unsigned long long* __restrict__ out) {
    unsigned long long acc = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += (int64_t)gridDim.x * blockDim.x)
        acc += mix64((unsigned long long)ei[e], (unsigned long long)ei[n_edges + e]);
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) atomicAdd(&out[1], acc);
    if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = (unsigned long long)n_edges;
}

// out[0] = sum mix64(src, dst), out[1] = sum mix64(dst, src) over the edges a CSR keeps: equal <=> (up to a 2^-64 collision)
// the edge multiset equals its own transpose <=> A_hat is symmetric
__global__ void k_edge_sym(const int64_t* __restrict__ ei, int64_t n_edges, int64_t n_nodes, unsigned long long* __restrict__ out) {
    unsigned long long a = 0, b = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t src = ei[e], dst = ei[n_edges + e];
        if (src == dst || src < 0 || dst < 0 || src >= n_nodes || dst >= n_nodes) continue;
        a += mix64((unsigned long long)src, (unsigned long long)dst);
        b += mix64((unsigned long long)dst, (unsigned long long)src);
    }
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&out[0], a); atomicAdd(&out[1], b); }
}

// ---- CSR regrouped into tiles of 64 nodes that are close in the graph ------------------------------------------------------
// The layer kernel aggregates a tile of 64 rows per workgroup.  With 64 CONSECUTIVE node ids per tile almost every source row
// of an edge lies outside the tile and is loaded once per edge (2.8x the bytes of the implicit stencil at configs[1]); if the
// tile is a breadth-first ball of the graph most sources are the tile's own rows, which the kernel loads once into LDS.
// Greedy graph growing: a tile is filled breadth-first from a seed (taken from the frontier the previous tile left behind, so
// that consecutive tiles are neighbours too); what the queue still holds when the tile is full becomes that frontier.
// order[s] = node of tile slot s (tile = s / 64); `cluster` = false: identity order (consecutive rows).
static void csr_tile_order(int n, const std::vector<int>& rowptr, const std::vector<int>& colidx, bool cluster, std::vector<int>& order) {
    order.clear();
    order.reserve((size_t)n);
    if (!cluster) {
        for (int i = 0; i < n; ++i) order.push_back(i);
        return;
    }
    std::vector<unsigned char> seen((size_t)n, 0);      // 1: placed or in the current queue
    std::vector<int> frontier, q;
    size_t fhead = 0;
    int next_seed = 0;
    while ((int)order.size() < n) {
        int filled = 0;
        q.clear();
        size_t qhead = 0;
        while (filled < TILE && (int)order.size() < n) {
            if (qhead == q.size()) {                      // (the component is exhausted, or the tile starts): a new seed
                int seed = -1;
                while (fhead < frontier.size()) {
                    const int c = frontier[fhead++];
                    if (!seen[c]) { seed = c; break; }
                }
                if (seed < 0) {
                    while (seen[next_seed]) ++next_seed;
                    seed = next_seed;
                }
                seen[seed] = 1;
                q.push_back(seed);
            }
            const int u = q[qhead++];
            order.push_back(u);
            ++filled;
            for (int e = rowptr[u]; e < rowptr[u + 1]; ++e) {
                const int v = colidx[e];
                if (!seen[v]) { seen[v] = 1; q.push_back(v); }
            }
        }
        // queued but not placed: the next tiles' seeds, nearest first
        if (fhead > (1u << 20) && fhead * 2 > frontier.size()) { frontier.erase(frontier.begin(), frontier.begin() + (long)fhead); fhead = 0; }
        for (size_t k = qhead; k < q.size(); ++k) { seen[q[k]] = 0; frontier.push_back(q[k]); }
    }
}

// builds g->t_* from the handle's device CSR (host round trip: a set-up call); mode 1: consecutive rows, 2: clustered
static int csr_tiles(eg_graph* g, int mode, hipStream_t stream) {
    const int n = (int)g->n_nodes;
    const size_t nnz = (size_t)g->nnz;
    std::vector<int> rowptr((size_t)n + 1), colidx(nnz ? nnz : 1);
    std::vector<float> dis((size_t)n);
    EG_HIP_TRY(hipMemcpyAsync(rowptr.data(), g->rowptr, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost, stream));
    if (nnz) EG_HIP_TRY(hipMemcpyAsync(colidx.data(), g->colidx, sizeof(int) * nnz, hipMemcpyDeviceToHost, stream));
    EG_HIP_TRY(hipMemcpyAsync(dis.data(), g->dis, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, stream));
    EG_HIP_TRY(hipStreamSynchronize(stream));
    std::vector<int> order;
    csr_tile_order(n, rowptr, colidx, mode >= 2, order);
    const int n_tiles = (n + TILE - 1) / TILE;
    const size_t slots = (size_t)n_tiles * TILE;
    std::vector<int> slot_of((size_t)n), t_rows(slots, -1), t_rowptr(slots + 1, 0), t_code(nnz ? nnz : 1), t_tgt(nnz ? nnz : 1);
    std::vector<float> t_w(nnz ? nnz : 1), t_dis(slots, 0.f);
    for (int s = 0; s < n; ++s) slot_of[(size_t)order[(size_t)s]] = s;
    size_t o = 0;
    for (size_t s = 0; s < slots; ++s) {
        t_rowptr[s] = (int)o;
        if (s >= (size_t)n) continue;
        const int u = order[s];
        t_rows[s] = u;
        t_dis[s] = dis[(size_t)u] * dis[(size_t)u];
        for (int e = rowptr[(size_t)u]; e < rowptr[(size_t)u + 1]; ++e) {      // (edge order kept: the sum of a row has the old order)
            const int v = colidx[(size_t)e];
            const int sv = slot_of[(size_t)v];
            t_code[o] = (sv / TILE == (int)(s / TILE)) ? -(sv % TILE + 1) : v;
            t_w[o] = dis[(size_t)v] * dis[(size_t)u];
            t_tgt[o] = (int)(s & 7);
            ++o;
        }
    }
    t_rowptr[slots] = (int)o;
    EG_HIP_TRY(upload(&g->t_rows, t_rows));
    EG_HIP_TRY(upload(&g->t_rowptr, t_rowptr));
    EG_HIP_TRY(upload(&g->t_code, t_code));
    EG_HIP_TRY(upload(&g->t_tgt, t_tgt));
    EG_HIP_TRY(upload(&g->t_w, t_w));
    EG_HIP_TRY(upload(&g->t_dis, t_dis));
    g->n_ctiles = n_tiles;
    return EG_OK;
}

// the temporaries of one CSR build, freed on every way out of csr_fill
struct CsrScratch {
    int *keys = nullptr, *vals = nullptr, *keys_out = nullptr, *counts = nullptr;
    unsigned long long* sym = nullptr;
    void* tmp = nullptr;
    ~CsrScratch() {
        for (void* p : {(void*)keys, (void*)vals, (void*)keys_out, (void*)counts, (void*)sym, tmp})
            if (p) (void)hipFree(p);
    }
};

// rowptr / colidx / dis / nnz / symmetric of a fresh CSR handle from the edge list (csr_build)
static int csr_fill(eg_graph* g, const int64_t* ei, int n, int m, hipStream_t stream, const eg_graph* base) {
    const int64_t n_nodes = n, n_edges = m;
    CsrScratch s;
    size_t tmp_bytes = 0, tmp2 = 0;
    const size_t mm = (size_t)(m > 0 ? m : 1);
    EG_HIP_TRY(hipMalloc((void**)&s.keys, sizeof(int) * mm));
    EG_HIP_TRY(hipMalloc((void**)&s.vals, sizeof(int) * mm));
    EG_HIP_TRY(hipMalloc((void**)&s.keys_out, sizeof(int) * mm));
    EG_HIP_TRY(hipMalloc((void**)&s.counts, sizeof(int) * ((size_t)n + 1)));
    EG_HIP_TRY(hipMalloc((void**)&g->colidx, sizeof(int) * mm));
    EG_HIP_TRY(hipMalloc((void**)&g->rowptr, sizeof(int) * ((size_t)n + 1)));
    EG_HIP_TRY(hipMalloc((void**)&g->dis, sizeof(float) * (size_t)n));
    EG_HIP_TRY(alloc_queue_ring(g));
    EG_HIP_TRY(hipMemsetAsync(g->walk_counters, 0, QUEUE_RING_BYTES, stream));
    EG_HIP_TRY(hipMemsetAsync(s.counts, 0, sizeof(int) * ((size_t)n + 1), stream));
    int end_bit = 1;                             // key bits of the stable LSD radix sort by target: neighbours keep their edge_index order
    while ((1ll << end_bit) <= n_nodes && end_bit < 32) ++end_bit;
    if (m > 0) {
        hipLaunchKernelGGL(k_edge_keys, dim3((m + 255) / 256), dim3(256), 0, stream, ei, n_edges, n, base ? 1 : 0, s.keys, s.vals, s.counts);
        EG_HIP_TRY(hipGetLastError());
        EG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, s.keys, s.keys_out, s.vals, g->colidx, m, 0, end_bit, stream));
    }
    EG_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp2, s.counts, g->rowptr, n + 1, stream));
    if (tmp2 > tmp_bytes) tmp_bytes = tmp2;
    EG_HIP_TRY(hipMalloc(&s.tmp, tmp_bytes ? tmp_bytes : 16));
    if (m > 0) {
        size_t tb = tmp_bytes;
        EG_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(s.tmp, tb, s.keys, s.keys_out, s.vals, g->colidx, m, 0, end_bit, stream));
    }
    {
        size_t tb = tmp_bytes;
        EG_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(s.tmp, tb, s.counts, g->rowptr, n + 1, stream));
    }
    unsigned long long sym_host[2] = {0, 0};
    if (base) {
        EG_HIP_TRY(hipMemcpyAsync(g->dis, base->dis, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, stream));
    } else {
        hipLaunchKernelGGL(k_dis_from_counts, dim3((n + 255) / 256), dim3(256), 0, stream, s.counts, n, g->dis);
        EG_HIP_TRY(hipGetLastError());
        EG_HIP_TRY(hipMalloc((void**)&s.sym, 2 * sizeof(unsigned long long)));
        EG_HIP_TRY(hipMemsetAsync(s.sym, 0, 2 * sizeof(unsigned long long), stream));
        if (m > 0) {
            int blocks = (m + 255) / 256;
            hipLaunchKernelGGL(k_edge_sym, dim3(blocks > 2048 ? 2048 : blocks), dim3(256), 0, stream, ei, n_edges, n_nodes, s.sym);
            EG_HIP_TRY(hipGetLastError());
        }
        EG_HIP_TRY(hipMemcpyAsync(sym_host, s.sym, sizeof(sym_host), hipMemcpyDeviceToHost, stream));
    }
    int nnz = 0;
    EG_HIP_TRY(hipMemcpyAsync(&nnz, g->rowptr + n, sizeof(int), hipMemcpyDeviceToHost, stream));
    EG_HIP_TRY(hipStreamSynchronize(stream));
    g->nnz = nnz;
    g->symmetric = base ? base->symmetric : (sym_host[0] == sym_host[1]);
    return EG_OK;
}

// base == NULL: rows = targets, (deg+1)^-1/2 from the in-degrees.  base != NULL: rows = sources (the transposed adjacency
// of the same edge_index), normalisation copied from base.
static int csr_build(const int64_t* ei, int64_t n_nodes, int64_t n_edges, hipStream_t stream, const eg_graph* base, eg_graph** out) {
    if (!out) return set_error(EG_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (n_nodes <= 0 || n_nodes >= (1ll << 31) - 1 || n_edges < 0 || n_edges >= (1ll << 31) - 1)
        return set_error(EG_ERR_ARG, "n_nodes / n_edges out of int32 range");
    if (n_edges > 0 && !ei) return set_error(EG_ERR_ARG, "edge_index is NULL");
    std::unique_ptr<eg_graph> g = new_handle(GRAPH_CSR, n_nodes);
    int rc = csr_fill(g.get(), ei, (int)n_nodes, (int)n_edges, stream, base);
    if (rc == EG_OK && g->knobs.csr_tiles > 0) rc = csr_tiles(g.get(), g->knobs.csr_tiles, stream);
    if (rc != EG_OK) return rc;
    *out = g.release();
    return EG_OK;
}

// allocate and copy what build_topo_tables made for the handle
static hipError_t upload_topo(eg_graph* g, const TopoTables& tt) {
    hipError_t e = upload(&g->dis, tt.dis);
    if (e == hipSuccess) e = alloc_queue_ring(g);
    if (e == hipSuccess) e = hipMemset(g->walk_counters, 0, QUEUE_RING_BYTES);
    if (e == hipSuccess) e = hipMalloc((void**)&g->topo_dev, sizeof(Topo));
    if (e == hipSuccess) e = hipMemcpy(g->topo_dev, &g->topo, sizeof(Topo), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = upload(&g->tiles_dev, tt.tiles);
    if (e == hipSuccess) e = upload(&g->segs_dev, tt.segs);
    if (e == hipSuccess) e = upload(&g->pats_dev, tt.pats);
    if (e == hipSuccess) e = upload(&g->patsq_dev, tt.patsq);
    if (g->n_conn > 0) {
        const size_t per_frame = (size_t)(g->conn_chunks + 2 * g->n_conn) * C;
        if (e == hipSuccess) e = upload(&g->conn_table, tt.conn_table, 4);
        if (e == hipSuccess) e = hipMalloc((void**)&g->conn_scratch, sizeof(float) * per_frame * g->conn_cap * QUEUE_SLOTS);
    }
    if (g->hybrid) {
        if (e == hipSuccess) e = upload(&g->rowptr, tt.h_rowptr);
        if (e == hipSuccess) e = upload(&g->colidx, tt.h_colidx, 1);
    }
    return e;
}

}  // namespace eg

// The one owner of a handle's device resources: every way out of a create call that does not hand the handle over, and
// eg_graph_destroy, end here.
eg_graph::~eg_graph() {
    for (void* p : {(void*)dis, (void*)topo_dev, (void*)tiles_dev, (void*)segs_dev, (void*)pats_dev, (void*)patsq_dev, (void*)walk_counters,
                    (void*)rowptr, (void*)colidx, (void*)conn_table, (void*)conn_scratch, (void*)t_rows, (void*)t_rowptr, (void*)t_code,
                    (void*)t_tgt, (void*)t_w, (void*)t_dis})
        if (p) (void)hipFree(p);
    for (float* p : conn_retired) (void)hipFree(p);
    for (hipEvent_t ev : slot_event)
        if (ev) (void)hipEventDestroy(ev);
    if (era_event) (void)hipEventDestroy(era_event);
}

// ---- eg_debug_layer_timing_*: events around layer-kernel launches while armed (bench.py's in-step kernel durations) ----
namespace {
constexpr int TIMING_MAX = 256;
std::atomic<int> g_timing_armed{0};        // launches still to be timed
std::atomic<int> g_timing_count{0};
hipEvent_t g_timing_ev[2 * TIMING_MAX];
int g_timing_kind[TIMING_MAX];
bool g_timing_have_events = false;
}  // namespace

eg::LaunchTimer::LaunchTimer(int kind, hipStream_t s) : idx(-1), stream(s) {
    if (g_timing_armed.load(std::memory_order_relaxed) <= 0) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); return; }
    if (cs != hipStreamCaptureStatusNone) return;
    if (g_timing_armed.fetch_sub(1, std::memory_order_relaxed) <= 0) return;
    const int i = g_timing_count.fetch_add(1, std::memory_order_relaxed);
    if (i >= TIMING_MAX) return;
    g_timing_kind[i] = kind;
    if (hipEventRecord(g_timing_ev[2 * i], s) == hipSuccess) idx = i;
}
eg::LaunchTimer::~LaunchTimer() {
    if (idx >= 0) (void)hipEventRecord(g_timing_ev[2 * idx + 1], stream);
}

using namespace eg;

extern "C" {

int eg_version(void) { return EG_ABI_VERSION; }

int eg_debug_layer_timing_begin(int max_launches) {
    if (max_launches < 1 || max_launches > TIMING_MAX) return eg::set_error(EG_ERR_ARG, "max_launches must be in [1, 256]");
    if (!g_timing_have_events) {
        for (int i = 0; i < 2 * TIMING_MAX; ++i) EG_HIP_TRY(hipEventCreate(&g_timing_ev[i]));
        g_timing_have_events = true;
    }
    g_timing_count.store(0, std::memory_order_relaxed);
    g_timing_armed.store(max_launches, std::memory_order_relaxed);
    return EG_OK;
}

int eg_debug_layer_timing_end(float* ms, int* kinds, int cap) {
    g_timing_armed.store(0, std::memory_order_relaxed);
    int n = g_timing_count.load(std::memory_order_relaxed);
    if (n > TIMING_MAX) n = TIMING_MAX;
    if (!ms || !kinds || cap < n) return eg::set_error(EG_ERR_ARG, "ms / kinds too small");
    for (int i = 0; i < n; ++i) {
        EG_HIP_TRY(hipEventSynchronize(g_timing_ev[2 * i + 1]));
        EG_HIP_TRY(hipEventElapsedTime(&ms[i], g_timing_ev[2 * i], g_timing_ev[2 * i + 1]));
        kinds[i] = g_timing_kind[i];
    }
    g_timing_count.store(0, std::memory_order_relaxed);
    return n;
}

const char* eg_last_error(void) { return g_last_error.c_str(); }

int eg_topo_create(int frame, int naux, int main_only, int coord_nodes, int conn_nodes, int diag_main, int diag_aux,
                   eg_graph** out) {
    if (!out) return set_error(EG_ERR_ARG, "out is NULL");
    *out = nullptr;
    Topo T;
    int rc = build_topo(frame, naux, main_only, coord_nodes, conn_nodes, diag_main, diag_aux, T);
    if (rc != EG_OK) return rc;
    TopoTables tt;
    rc = build_topo_tables(T, tt);
    if (rc != EG_OK) return rc;
    std::unique_ptr<eg_graph> g = new_handle(GRAPH_TOPO, T.n_nodes);
    g->topo = T;
    g->n_tiles = (int)tt.tiles.size();
    g->n_pats = tt.n_pats;
    g->kid_rows = tt.kid_rows;
    g->flat = tt.flat;
    if (T.n_conn > 0) {
        g->n_conn = T.n_conn;
        g->conn_chunks = tt.conn_chunks;
        g->conn_cap = 8;                                   // frames the scratch holds at first (it grows: conn.hip)
    }
    if (tt.hybrid) {
        g->hybrid = 1;
        g->nnz = (int64_t)tt.h_colidx.size();
        g->symmetric = 1;
    }
    const hipError_t e = upload_topo(g.get(), tt);
    if (e != hipSuccess) return set_error(EG_ERR_HIP, std::string("eg_topo_create: ") + hipGetErrorString(e));
    *out = g.release();
    return EG_OK;
}

int eg_csr_create(const int64_t* ei, int64_t n_nodes, int64_t n_edges, eg_stream_t stream, eg_graph** out) {
    return csr_build(ei, n_nodes, n_edges, (hipStream_t)stream, nullptr, out);
}

int eg_csr_create_transposed(const eg_graph* base, const int64_t* ei, int64_t n_edges, eg_stream_t stream, eg_graph** out) {
    if (!base || base->kind != GRAPH_CSR) return set_error(EG_ERR_ARG, "base must be a CSR handle");
    return csr_build(ei, base->n_nodes, n_edges, (hipStream_t)stream, base, out);
}

int eg_graph_is_symmetric(const eg_graph* g) { return g && (g->kind == GRAPH_TOPO || g->symmetric); }

}  // extern "C"

extern "C" {

int eg_graph_destroy(eg_graph* g) {
    delete g;
    return EG_OK;
}

int64_t eg_graph_num_nodes(const eg_graph* g) { return g ? g->n_nodes : -1; }

int eg_graph_is_structured(const eg_graph* g) { return g && g->kind == GRAPH_TOPO; }

int64_t eg_graph_kidsum_rows(const eg_graph* g) { return (g && g->kind == GRAPH_TOPO) ? g->kid_rows : 0; }

int64_t eg_graph_num_tiles(const eg_graph* g) { return g ? (g->kind == GRAPH_TOPO ? g->n_tiles : (g->n_nodes + TILE - 1) / TILE) : -1; }

int eg_graph_deg_inv_sqrt(const eg_graph* g, float* out_dev, eg_stream_t stream) {
    if (!g || !out_dev) return set_error(EG_ERR_ARG, "NULL argument");
    EG_HIP_TRY(hipMemcpyAsync(out_dev, g->dis, sizeof(float) * g->n_nodes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return EG_OK;
}

int eg_debug_phase_cycles(eg_graph* g, uint64_t* out_host, int reset) {
    if (!g || !out_host) return set_error(EG_ERR_ARG, "NULL argument");
    EG_HIP_TRY(hipDeviceSynchronize());
    int* const tail = g->walk_counters + (size_t)QUEUE_SLOTS * QUEUE_SLICE_INTS;
    EG_HIP_TRY(hipMemcpy(out_host, tail, 11 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) EG_HIP_TRY(hipMemset(tail, 0, 16 * sizeof(uint64_t)));
    return EG_OK;
}

int eg_edge_hash(const int64_t* ei, int64_t n_edges, uint64_t* out_dev, eg_stream_t stream_) {
    if (!out_dev || (n_edges > 0 && !ei) || n_edges < 0) return set_error(EG_ERR_ARG, "bad argument");
    hipStream_t stream = (hipStream_t)stream_;
    EG_HIP_TRY(hipMemsetAsync(out_dev, 0, 2 * sizeof(uint64_t), stream));
    int blocks = (int)((n_edges + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_edge_hash, dim3(blocks), dim3(256), 0, stream, ei, n_edges, (unsigned long long*)out_dev);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

}  // extern "C"
