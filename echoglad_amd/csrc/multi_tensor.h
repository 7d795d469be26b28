// The one-launch multi-tensor update (adam.hip, optim.hip): the pointer table travels in the kernel arguments, a workgroup owns one
// chunk of MT_CHUNK elements of one tensor, finds its (tensor, chunk) in one parallel step over the chunk counts, and the workgroup that
// leaves last advances the per-tensor step counts.  The kernel (k_mt_step) and the host function (mt_launch) are here once; an update
// is an `Op`:
//     NP, MAX             arrays per tensor (parameter, gradient, then the state arrays) and tensors per launch
//     Scalars             the hyper-parameters as they travel in the kernel arguments, with `lr_dev` and `ticket`
//     Op(a, count)        device: whatever is uniform per tensor, from the scalars and the tensor's step count (read only if used)
//     used(j)             device, uniform: whether this launch reads array j; an unused one is never offset, loaded or stored
//     update(x)           device: one element of each array in, the new values out (x[1], the gradient, is not stored)
//     check(a)            host: the hyper-parameters; the refusal's text, or nullptr
//     state(t, a, s)      host: the state pointers of entry t into s[NP - 2]; the refusal's text, or nullptr
#pragma once
#include "train_common.h"

namespace eg {

constexpr int MT_THREADS = 256;
constexpr int MT_PER = 4;                             // elements per thread: all their loads are issued before the first use
constexpr int MT_CHUNK = MT_THREADS * MT_PER;         // elements per workgroup
// the table travels in the kernel arguments: 4 KB with the scalars and the 256 hidden bytes the runtime appends
constexpr int MT_KERNARG_BYTES = 4096;
constexpr int MT_HIDDEN_BYTES = 256;
constexpr int MT_TICKET_SLOT = 2;                     // one word for all updates: launches on one stream are ordered, and it is 0 between them

__host__ __device__ constexpr int mt_chunks(int n) { return (n - 1) / MT_CHUNK + 1; }   // n >= 1; no overflow up to 2^31 - 1
static_assert(mt_chunks(2147483647) == 2097152, "the chunk count of the largest tensor an entry may name");

template <int NP, int MAX>
struct MtTable {
    float* ptr[NP][MAX];                // [0] parameters, [1] gradients (read only), [2 ...] the op's state arrays
    int n[MAX];
    float* steps;                       // [count] device floats: the number of updates of each tensor so far
    int count;
};
template <class Op>
constexpr bool mt_fits = sizeof(MtTable<Op::NP, Op::MAX>) + sizeof(typename Op::Scalars) + MT_HIDDEN_BYTES <= MT_KERNARG_BYTES;

// (tensor, chunk) of this workgroup: thread k sums the chunk counts in front of tensor k and looks whether this workgroup falls into
// its range -- one parallel step over LDS (a scalar walk over the table is a chain of dependent constant-memory loads: 15 us)
template <int MAX>
__device__ inline void mt_locate(const int (&n)[MAX], int count, int& ti, int& rest) {
    static_assert(MAX <= MT_THREADS, "one thread per tensor in the look-up");
    __shared__ int s_chunks[MAX], s_ti, s_rest;
    const int t = threadIdx.x;
    if (t < count) s_chunks[t] = mt_chunks(n[t]);
    __syncthreads();
    if (t < count) {
        int first = 0;
        for (int k = 0; k < t; ++k) first += s_chunks[k];
        if ((int)blockIdx.x >= first && (int)blockIdx.x < first + s_chunks[t]) { s_ti = t; s_rest = blockIdx.x - first; }
    }
    __syncthreads();
    ti = s_ti;
    rest = s_rest;
}

// The last workgroup out advances the step counts.  No data is handed over, so no fence: a workgroup that reads its count has used the
// value before it gets here.  *ticket is 0 before the launch and 0 again after it (atomicInc wraps at gridDim.x - 1).
__device__ inline void mt_advance_counts(unsigned* ticket, float* steps, int count) {
    __shared__ int s_last;
    const int t = threadIdx.x;
    __syncthreads();
    if (t == 0) s_last = atomicInc(ticket, gridDim.x - 1) == gridDim.x - 1;
    __syncthreads();
    if (s_last && t < count) steps[t] += 1.0f;
}

// a * b + c * d with both products rounded before the sum -- the decayed average / buffer of all three updates.  Said outright, so that
// the bits do not hang on whether the compiler packs the two multiplications into one instruction or contracts one of them into an fma.
__device__ inline float mt_mul2_add(float a, float b, float c, float d) {
#pragma clang fp contract(off)
    return a * b + c * d;
}

// Accesses are 4-byte loads and stores, thread t of a workgroup at elements t, t + 256, ...: a wave covers 256 consecutive bytes, and a
// parameter slice need only be 4-byte aligned.
template <class Op>
__global__ __launch_bounds__(MT_THREADS) void k_mt_step(const MtTable<Op::NP, Op::MAX> tb, const typename Op::Scalars a) {
    constexpr int NP = Op::NP;
    int ti, rest;
    mt_locate(tb.n, tb.count, ti, rest);
    const int t = threadIdx.x;
    const Op op(a, tb.steps[ti]);
    // (a uniform run-time index into the kernel-argument segment: scalar loads)
    const int n = tb.n[ti], lo = rest * MT_CHUNK, len = n - lo < MT_CHUNK ? n - lo : MT_CHUNK;
    float* __restrict__ ptr[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) ptr[j] = op.used(j) ? tb.ptr[j][ti] + lo : nullptr;
    float x[MT_PER][NP];
#pragma unroll
    for (int k = 0; k < MT_PER; ++k) {
        const int i = t + k * MT_THREADS, c = i < len ? i : 0;
#pragma unroll
        for (int j = 0; j < NP; ++j) x[k][j] = op.used(j) ? ptr[j][c] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < MT_PER; ++k) {
        const int i = t + k * MT_THREADS;
        if (i >= len) continue;
        op.update(x[k]);
#pragma unroll
        for (int j = 2; j < NP; ++j)
            if (op.used(j)) ptr[j][i] = x[k][j];
        ptr[0][i] = x[k][0];
    }
    mt_advance_counts(a.ticket, tb.steps, tb.count);
}

// The host side of an entry point.  Every refusal comes before the first HIP call, a bad hyper-parameter before "split the list".
template <class Op, class Entry>
int mt_launch(const Entry* tensors, int count, float* steps, typename Op::Scalars a, eg_stream_t stream) {
    if (!tensors || !steps || count < 0) return set_error(EG_ERR_ARG, "NULL argument");
    if (const char* why = Op::check(a)) return set_error(EG_ERR_ARG, why);
    if (count > Op::MAX) return set_error(EG_ERR_UNSUPPORTED, "more tensors than one call takes (EG_*_MAX_TENSORS): split the list");
    if (count == 0) return EG_OK;
    MtTable<Op::NP, Op::MAX> tb{};
    long long blocks = 0;
    for (int k = 0; k < count; ++k) {
        const Entry& t = tensors[k];
        if (!t.param || !t.grad || t.numel < 1 || t.numel >= (1ll << 31)) return set_error(EG_ERR_ARG, "bad tensor entry");
        float* state[Op::NP - 2];
        if (const char* why = Op::state(t, a, state)) return set_error(EG_ERR_ARG, why);
        tb.ptr[0][k] = t.param;
        tb.ptr[1][k] = const_cast<float*>(t.grad);
        for (int j = 2; j < Op::NP; ++j) tb.ptr[j][k] = state[j - 2];
        tb.n[k] = (int)t.numel;
        blocks += mt_chunks((int)t.numel);
    }
    tb.count = count;
    tb.steps = steps;
    if (blocks >= (1ll << 31)) return set_error(EG_ERR_ARG, "too many elements");
    a.ticket = eg_ticket_ptr((void*)stream, MT_TICKET_SLOT);
    if (!a.ticket) return set_error(EG_ERR_HIP, "no device memory for a ticket word");
    hipLaunchKernelGGL(k_mt_step<Op>, dim3((unsigned)blocks), dim3(MT_THREADS), 0, (hipStream_t)stream, tb, a);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

}  // namespace eg
