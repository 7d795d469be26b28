// Per-channel confusion counts of a binary classifier over the valid rows: the numbers behind the reference's
// BalancedBinaryAccuracyEvaluator (src/core/evaluators.py:85-143), which moves logits, labels and valid to the host on every
// step and runs sklearn there.  One launch per update, integer arithmetic only (exact, independent of order, bit-reproducible).
//
// Per channel c, over the rows with valid > 0 (y != 0 is a positive label; a prediction is positive iff pred > 0.5, strict,
// on whatever the model returned -- NaN compares false, as numpy's does):
//     TP = #(y != 0, pred > 0.5)   FN = #(y != 0, !(pred > 0.5))   FP = #(y == 0, pred > 0.5)   TN = #(y == 0, !(pred > 0.5))
// Every wave counts four masks per channel with 64-bit ballots (valid, valid & pos, valid & predicted, valid & pos & predicted),
// a workgroup sums its waves in LDS and leaves one partial; the last workgroup out (a self-resetting ticket, train_common.h's
// eg_ticket_ptr slot 3) sums the partials in a fixed order, appends the record history[*counter] (when *counter < capacity) and advances *counter.  No memset node, no host
// synchronisation: a captured launch appends one record per replay.
#include "train_common.h"

namespace eg {

constexpr int CC_THREADS = 512;                    // 8 waves
constexpr int CC_WAVES = CC_THREADS / 64;
constexpr int CC_UNROLL = 4;                       // rows per lane per sweep: every load of a sweep is issued before its first compare
#ifndef CC_MAX_BLOCKS
#define CC_MAX_BLOCKS 512                          // two workgroups per CU at most
#endif
constexpr int CC_MAX_CHANNELS = 8;

struct CountArgs {
    const float* pred;
    const float* y;
    const float* valid;
    long long rows;
    unsigned long long* partial;                   // [gridDim.x][channels * 4]
    long long* history;                            // [capacity][channels][4]: TP, FN, FP, TN
    long long capacity;
    long long* counter;
    unsigned* ticket;
};

// row r of a [rows, NC] array; VEC (NC == 4, 16-B aligned): one 16-byte load
template <int NC, bool VEC>
__device__ inline void load_row(const float* __restrict__ p, long long r, float (&v)[NC]) {
    if constexpr (VEC) {
        const f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + r);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = __builtin_nontemporal_load(p + r * NC + c);
    }
}

template <int NC, bool VEC>
__global__ __launch_bounds__(CC_THREADS) void k_confusion_counts(const CountArgs a) {
    constexpr int NV = NC * 4;
    static_assert(NV <= 64, "the partials of a workgroup are written by wave 0");
    __shared__ unsigned long long s_wave[CC_WAVES][NV];
    __shared__ unsigned long long s_red[CC_THREADS];
    __shared__ long long s_rec;
    __shared__ unsigned s_last;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const long long rows = a.rows;
    const long long span = 64ll * CC_UNROLL;
    const long long step = (long long)gridDim.x * CC_WAVES * span;
    // cnt[c][0] valid, [1] valid & positive label, [2] valid & positive prediction, [3] all three (wave-uniform)
    unsigned long long cnt[NC][4] = {};
    for (long long base = ((long long)blockIdx.x * CC_WAVES + wave) * span; base < rows; base += step) {
        float pv[CC_UNROLL][NC], yv[CC_UNROLL][NC], vv[CC_UNROLL][NC];
#pragma unroll
        for (int u = 0; u < CC_UNROLL; ++u) {
            const long long r = base + u * 64 + lane, rr = r < rows ? r : rows - 1;
            load_row<NC, VEC>(a.pred, rr, pv[u]);
            load_row<NC, VEC>(a.y, rr, yv[u]);
            load_row<NC, VEC>(a.valid, rr, vv[u]);
        }
#pragma unroll
        for (int u = 0; u < CC_UNROLL; ++u) {
            const bool in = base + u * 64 + lane < rows;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const unsigned long long mv = __ballot(in && vv[u][c] > 0.f);
                const unsigned long long mp = mv & __ballot(yv[u][c] != 0.f);
                const unsigned long long mq = mv & __ballot(pv[u][c] > 0.5f);
                cnt[c][0] += __popcll(mv);
                cnt[c][1] += __popcll(mp);
                cnt[c][2] += __popcll(mq);
                cnt[c][3] += __popcll(mp & mq);
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) s_wave[wave][c * 4 + k] = cnt[c][k];
    }
    __syncthreads();
    // Hand-off to the last workgroup out without a fence: the partials are agent-scope (write-through) stores of wave 0, the ticket
    // is drawn by lane 0 of the same wave once they have completed, and the last workgroup reads them with agent-scope loads.
    // (last_workgroup_out's device-scope release in every workgroup costs ~14 us per 256 workgroups in this kernel, measured: more
    // than the whole batch-8 pass.)
    if (wave == 0) {
        if (t < NV) {
            unsigned long long s = 0;
#pragma unroll
            for (int w = 0; w < CC_WAVES; ++w) s += s_wave[w][t];
            __hip_atomic_store(a.partial + (size_t)blockIdx.x * NV + t, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (t == 0) s_last = atomicInc(a.ticket, gridDim.x - 1) == gridDim.x - 1 ? 1u : 0u;   // wraps to 0: no reset
    }
    __syncthreads();
    if (!s_last) return;

    // the last workgroup out: thread t sums column t % NV of the partials of workgroups t / NV, + S, + 2S, ... (fixed order)
    constexpr int S = CC_THREADS / NV;
    if (t == 0) s_rec = *a.counter;
    if (t < S * NV) {
        constexpr int PER = (CC_MAX_BLOCKS + S - 1) / S;       // all loads in flight before the first add
        const int j = t % NV;
        unsigned long long v[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const unsigned b = t / NV + k * S;
            v[k] = b < gridDim.x ? __hip_atomic_load(a.partial + (size_t)b * NV + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        }
        unsigned long long s = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) s += v[k];
        s_red[t] = s;
    }
    __syncthreads();
    if (t < NV) {
        unsigned long long s = 0;
        for (int k = 0; k < S; ++k) s += s_red[k * NV + t];
        s_wave[0][t] = s;
    }
    __syncthreads();
    const long long rec = s_rec;
    if (t < NV && rec < a.capacity) {
        const int c = t >> 2, k = t & 3;
        const long long v = (long long)s_wave[0][c * 4 + 0], p = (long long)s_wave[0][c * 4 + 1];
        const long long q = (long long)s_wave[0][c * 4 + 2], tp = (long long)s_wave[0][c * 4 + 3];
        const long long out = k == 0 ? tp : k == 1 ? p - tp : k == 2 ? q - tp : v - p - q + tp;
        a.history[rec * NV + t] = out;
    }
    if (t == 0) *a.counter = rec + 1;              // past capacity too: the host refuses a history that overflowed
}

template <int NC>
static void launch_counts(const CountArgs& a, bool vec, unsigned blocks, hipStream_t s) {
    if constexpr (NC == 4) {
        if (vec) {
            hipLaunchKernelGGL((k_confusion_counts<4, true>), dim3(blocks), dim3(CC_THREADS), 0, s, a);
            return;
        }
    }
    hipLaunchKernelGGL((k_confusion_counts<NC, false>), dim3(blocks), dim3(CC_THREADS), 0, s, a);
}

}  // namespace eg

using namespace eg;

extern "C" {

int eg_confusion_counts(const float* pred, const float* y, const float* valid, int64_t rows, int channels, void* workspace,
                        size_t workspace_bytes, int64_t* history, int64_t capacity, int64_t* counter, eg_stream_t stream) {
    if (!pred || !y || !valid || !workspace || !history || !counter) return set_error(EG_ERR_ARG, "NULL argument");
    if (channels < 1 || channels > CC_MAX_CHANNELS) return set_error(EG_ERR_UNSUPPORTED, "1 <= channels <= 8");
    if (rows < 1 || rows > (1ll << 40)) return set_error(EG_ERR_ARG, "rows must be in [1, 2^40]");
    if (capacity < 1) return set_error(EG_ERR_ARG, "capacity must be >= 1");
    const size_t per_block = (size_t)channels * 4 * sizeof(unsigned long long);
    if (workspace_bytes < per_block) return set_error(EG_ERR_ARG, "workspace smaller than one workgroup's partial");
    if ((uintptr_t)workspace % 8 || (uintptr_t)history % 8 || (uintptr_t)counter % 8) return set_error(EG_ERR_ARG, "misaligned 64-bit buffer");
    const long long rows_per_block = (long long)CC_THREADS * CC_UNROLL;
    long long blocks = (rows + rows_per_block - 1) / rows_per_block;
    if (blocks > CC_MAX_BLOCKS) blocks = CC_MAX_BLOCKS;
    if (blocks > (long long)(workspace_bytes / per_block)) blocks = (long long)(workspace_bytes / per_block);
    unsigned* ticket = eg_ticket_ptr((void*)stream, 3);
    if (!ticket) return set_error(EG_ERR_HIP, "no device memory for a ticket word");
    const bool vec = ((uintptr_t)pred | (uintptr_t)y | (uintptr_t)valid) % 16 == 0;
    const CountArgs a{pred, y, valid, (long long)rows, (unsigned long long*)workspace, (long long*)history, (long long)capacity,
                      (long long*)counter, ticket};
    hipStream_t s = (hipStream_t)stream;
    switch (channels) {
        case 1: launch_counts<1>(a, vec, (unsigned)blocks, s); break;
        case 2: launch_counts<2>(a, vec, (unsigned)blocks, s); break;
        case 3: launch_counts<3>(a, vec, (unsigned)blocks, s); break;
        case 4: launch_counts<4>(a, vec, (unsigned)blocks, s); break;
        case 5: launch_counts<5>(a, vec, (unsigned)blocks, s); break;
        case 6: launch_counts<6>(a, vec, (unsigned)blocks, s); break;
        case 7: launch_counts<7>(a, vec, (unsigned)blocks, s); break;
        default: launch_counts<8>(a, vec, (unsigned)blocks, s); break;
    }
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

}  // extern "C"
