// The skeleton of a one-launch multi-tensor update (optim.hip; adam.hip carries the same scheme inline and is left as it is, so that
// its device code stays what tests/test_gpu_adam.py measured): the pointer table travels in the kernel arguments, a workgroup owns one
// chunk of MT_CHUNK elements of one tensor, finds its (tensor, chunk) in one parallel step over the chunk counts, and the workgroup that
// leaves last advances the per-tensor step counts.
#pragma once
#include "train_common.h"

namespace eg {

constexpr int MT_THREADS = 256;
constexpr int MT_PER = 4;                             // elements per thread: all their loads are issued before the first use
constexpr int MT_CHUNK = MT_THREADS * MT_PER;         // elements per workgroup
// the table travels in the kernel arguments: 4 KB with the scalars and the 256 hidden bytes the runtime appends
constexpr int MT_KERNARG_BYTES = 4096;
constexpr int MT_HIDDEN_BYTES = 256;

__host__ __device__ inline int mt_chunks(int n) { return (n - 1) / MT_CHUNK + 1; }   // n >= 1; no overflow up to 2^31 - 1

// (tensor, chunk) of this workgroup: thread k sums the chunk counts in front of tensor k and looks whether this workgroup falls into
// its range -- one parallel step over LDS (a scalar walk over the table is a chain of dependent constant-memory loads)
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

}  // namespace eg
