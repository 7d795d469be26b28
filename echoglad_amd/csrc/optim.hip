// SGD and RMSprop as ONE launch per step (gfx950): the other two names of the reference's optimizer registry
// (src/builders/optimizer_builder.py: sgd, rmsprop, adam), on the skeleton of adam.hip (multi_tensor.h).
// torch.optim.SGD has no capturable form at all and torch.optim.RMSprop(capturable=True) is a chain of _foreach_* launches; a captured
// batch-1 training step (engine.GraphedTrainStep) is host- and launch-bound, so the update is one node here as well.
// Arithmetic: torch's _single_tensor_sgd / _single_tensor_rmsprop, operation by operation (include/echoglad_hip.h spells both out).
// SGD's first update of a tensor copies the gradient into the momentum buffer WITHOUT dampening.  torch decides that on the host
// (`momentum_buffer is None`); here the kernel reads the tensor's device step count, so the launch arguments are the same in step 1 and
// in step 100 -- a captured launch replays correctly from either side of the first update.
// Accesses are 4-byte loads and stores, thread t of a workgroup at elements t, t + 256, ...: a wave covers 256 consecutive bytes, and a
// parameter slice need only be 4-byte aligned.
#include "multi_tensor.h"

namespace eg {

constexpr int SGD_MAX_TENSORS = EG_SGD_MAX_TENSORS;
constexpr int RMSPROP_MAX_TENSORS = EG_RMSPROP_MAX_TENSORS;

struct SgdTable {
    float* p[SGD_MAX_TENSORS];
    const float* g[SGD_MAX_TENSORS];
    float* b[SGD_MAX_TENSORS];          // momentum buffers (momentum == 0: not read)
    int n[SGD_MAX_TENSORS];
    float* steps;                       // [count] device floats: the number of updates of each tensor so far
    int count;
};
struct SgdScalars {
    float lr, momentum, dampening, weight_decay;
    int nesterov, maximize;
    const float* lr_dev;                // nullable: the learning rate as a device scalar
    unsigned* ticket;
};
static_assert(sizeof(SgdTable) + sizeof(SgdScalars) + MT_HIDDEN_BYTES <= MT_KERNARG_BYTES, "the kernel arguments must stay within 4 KB");

struct RmspropTable {
    float* p[RMSPROP_MAX_TENSORS];
    const float* g[RMSPROP_MAX_TENSORS];
    float* sq[RMSPROP_MAX_TENSORS];
    float* ga[RMSPROP_MAX_TENSORS];     // centered only
    float* b[RMSPROP_MAX_TENSORS];      // momentum > 0 only
    int n[RMSPROP_MAX_TENSORS];
    float* steps;
    int count;
};
struct RmspropScalars {
    float lr, alpha, eps, weight_decay, momentum;
    int centered, maximize;
    const float* lr_dev;
    unsigned* ticket;
};
// five pointers per tensor: 84 entries (the default landmark model with its coordinate graph has 82 parameter tensors, 84 with a 1 x 1
// embedder) take the table past adam.hip's round 3.5 KB, so the sum is checked against the 4 KB itself
static_assert(sizeof(RmspropTable) + sizeof(RmspropScalars) + MT_HIDDEN_BYTES <= MT_KERNARG_BYTES, "the kernel arguments must stay within 4 KB");

__global__ __launch_bounds__(MT_THREADS) void k_sgd_step(const SgdTable tb, const SgdScalars a) {
    int ti, rest;
    mt_locate(tb.n, tb.count, ti, rest);
    const int t = threadIdx.x;
    const bool has_buf = a.momentum != 0.f;
    const bool first = has_buf && tb.steps[ti] == 0.f;           // this tensor's first update: the buffer becomes a copy of g
    const float lr = a.lr_dev ? *a.lr_dev : a.lr;
    // (a uniform run-time index into the kernel-argument segment: scalar loads)
    const int n = tb.n[ti], lo = rest * MT_CHUNK, len = n - lo < MT_CHUNK ? n - lo : MT_CHUNK;
    float* __restrict__ p = tb.p[ti] + lo;
    const float* __restrict__ g = tb.g[ti] + lo;
    float* __restrict__ b = has_buf ? tb.b[ti] + lo : nullptr;
    const float w = 1.0f - a.dampening;
    float pv[MT_PER], gv[MT_PER], bv[MT_PER];
#pragma unroll
    for (int k = 0; k < MT_PER; ++k) {
        const int i = t + k * MT_THREADS, j = i < len ? i : 0;
        pv[k] = p[j]; gv[k] = g[j];
        bv[k] = has_buf ? b[j] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < MT_PER; ++k) {
        const int i = t + k * MT_THREADS;
        if (i >= len) continue;
        const float pi = pv[k];
        float gi = a.maximize ? -gv[k] : gv[k];
        if (a.weight_decay != 0.f) gi = gi + a.weight_decay * pi;
        if (has_buf) {
            const float bi = first ? gi : a.momentum * bv[k] + w * gi;
            b[i] = bi;
            gi = a.nesterov ? gi + a.momentum * bi : bi;
        }
        p[i] = pi - lr * gi;
    }
    mt_advance_counts(a.ticket, tb.steps, tb.count);
}

__global__ __launch_bounds__(MT_THREADS) void k_rmsprop_step(const RmspropTable tb, const RmspropScalars a) {
    int ti, rest;
    mt_locate(tb.n, tb.count, ti, rest);
    const int t = threadIdx.x;
    const bool has_buf = a.momentum > 0.f, centered = a.centered != 0;
    const float lr = a.lr_dev ? *a.lr_dev : a.lr;
    const int n = tb.n[ti], lo = rest * MT_CHUNK, len = n - lo < MT_CHUNK ? n - lo : MT_CHUNK;
    float* __restrict__ p = tb.p[ti] + lo;
    const float* __restrict__ g = tb.g[ti] + lo;
    float* __restrict__ sq = tb.sq[ti] + lo;
    float* __restrict__ ga = centered ? tb.ga[ti] + lo : nullptr;
    float* __restrict__ b = has_buf ? tb.b[ti] + lo : nullptr;
    const float w = 1.0f - a.alpha;
    float pv[MT_PER], gv[MT_PER], sv[MT_PER], av[MT_PER], bv[MT_PER];
#pragma unroll
    for (int k = 0; k < MT_PER; ++k) {
        const int i = t + k * MT_THREADS, j = i < len ? i : 0;
        pv[k] = p[j]; gv[k] = g[j]; sv[k] = sq[j];
        av[k] = centered ? ga[j] : 0.f;
        bv[k] = has_buf ? b[j] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < MT_PER; ++k) {
        const int i = t + k * MT_THREADS;
        if (i >= len) continue;
        const float pi = pv[k];
        float gi = a.maximize ? -gv[k] : gv[k];
        if (a.weight_decay != 0.f) gi = gi + a.weight_decay * pi;
        const float si = a.alpha * sv[k] + w * gi * gi;
        sq[i] = si;
        float avg;
        if (centered) {
            const float ai = av[k] + w * (gi - av[k]);
            ga[i] = ai;
            avg = sqrtf(si - ai * ai) + a.eps;
        } else {
            avg = sqrtf(si) + a.eps;
        }
        if (has_buf) {
            const float bi = a.momentum * bv[k] + gi / avg;
            b[i] = bi;
            p[i] = pi - lr * bi;
        } else {
            p[i] = pi - lr * gi / avg;
        }
    }
    mt_advance_counts(a.ticket, tb.steps, tb.count);
}

// the ticket word is adam.hip's (slot 2): launches on one stream are ordered, and the word is 0 between them
constexpr int OPTIM_TICKET_SLOT = 2;

}  // namespace eg

using namespace eg;

extern "C" {

int eg_sgd_step(const eg_sgd_tensor* tensors, int count, float* steps, float lr, const float* lr_device, float momentum, float dampening,
                float weight_decay, int nesterov, int maximize, eg_stream_t stream) {
    if (!tensors || !steps || count < 0) return set_error(EG_ERR_ARG, "NULL argument");
    if (!(momentum >= 0.f)) return set_error(EG_ERR_ARG, "momentum must be >= 0");
    if (!(weight_decay >= 0.f)) return set_error(EG_ERR_ARG, "weight_decay must be >= 0");
    if (nesterov && (!(momentum > 0.f) || dampening != 0.f)) return set_error(EG_ERR_ARG, "nesterov momentum requires a momentum and zero dampening");
    if (count > SGD_MAX_TENSORS) return set_error(EG_ERR_UNSUPPORTED, "more than EG_SGD_MAX_TENSORS tensors per call: split the list");
    if (count == 0) return EG_OK;
    SgdTable tb{};
    long long blocks = 0;
    for (int k = 0; k < count; ++k) {
        const eg_sgd_tensor& t = tensors[k];
        if (!t.param || !t.grad || t.numel < 1 || t.numel >= (1ll << 31)) return set_error(EG_ERR_ARG, "bad tensor entry");
        if (momentum != 0.f && !t.momentum_buffer) return set_error(EG_ERR_ARG, "momentum != 0 needs a momentum buffer for every tensor");
        tb.p[k] = t.param; tb.g[k] = t.grad; tb.b[k] = t.momentum_buffer; tb.n[k] = (int)t.numel;
        blocks += mt_chunks((int)t.numel);
    }
    tb.count = count;
    tb.steps = steps;
    if (blocks >= (1ll << 31)) return set_error(EG_ERR_ARG, "too many elements");
    unsigned* ticket = eg_ticket_ptr((void*)stream, OPTIM_TICKET_SLOT);
    if (!ticket) return set_error(EG_ERR_HIP, "no device memory for a ticket word");
    const SgdScalars a{lr, momentum, dampening, weight_decay, nesterov ? 1 : 0, maximize ? 1 : 0, lr_device, ticket};
    hipLaunchKernelGGL(k_sgd_step, dim3((unsigned)blocks), dim3(MT_THREADS), 0, (hipStream_t)stream, tb, a);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

int eg_rmsprop_step(const eg_rmsprop_tensor* tensors, int count, float* steps, float lr, const float* lr_device, float alpha, float eps,
                    float weight_decay, float momentum, int centered, int maximize, eg_stream_t stream) {
    if (!tensors || !steps || count < 0) return set_error(EG_ERR_ARG, "NULL argument");
    if (!(alpha >= 0.f) || !(eps >= 0.f) || !(momentum >= 0.f) || !(weight_decay >= 0.f))
        return set_error(EG_ERR_ARG, "alpha, eps, momentum and weight_decay must be >= 0");
    if (count > RMSPROP_MAX_TENSORS) return set_error(EG_ERR_UNSUPPORTED, "more than EG_RMSPROP_MAX_TENSORS tensors per call: split the list");
    if (count == 0) return EG_OK;
    RmspropTable tb{};
    long long blocks = 0;
    for (int k = 0; k < count; ++k) {
        const eg_rmsprop_tensor& t = tensors[k];
        if (!t.param || !t.grad || !t.square_avg || t.numel < 1 || t.numel >= (1ll << 31)) return set_error(EG_ERR_ARG, "bad tensor entry");
        if ((t.grad_avg != nullptr) != (centered != 0)) return set_error(EG_ERR_ARG, "grad_avg must be given exactly when centered is set");
        if ((t.momentum_buffer != nullptr) != (momentum > 0.f)) return set_error(EG_ERR_ARG, "momentum_buffer must be given exactly when momentum > 0");
        tb.p[k] = t.param; tb.g[k] = t.grad; tb.sq[k] = t.square_avg; tb.ga[k] = t.grad_avg; tb.b[k] = t.momentum_buffer; tb.n[k] = (int)t.numel;
        blocks += mt_chunks((int)t.numel);
    }
    tb.count = count;
    tb.steps = steps;
    if (blocks >= (1ll << 31)) return set_error(EG_ERR_ARG, "too many elements");
    unsigned* ticket = eg_ticket_ptr((void*)stream, OPTIM_TICKET_SLOT);
    if (!ticket) return set_error(EG_ERR_HIP, "no device memory for a ticket word");
    const RmspropScalars a{lr, alpha, eps, weight_decay, momentum, centered ? 1 : 0, maximize ? 1 : 0, lr_device, ticket};
    hipLaunchKernelGGL(k_rmsprop_step, dim3((unsigned)blocks), dim3(MT_THREADS), 0, (hipStream_t)stream, tb, a);
    EG_HIP_TRY(hipGetLastError());
    return EG_OK;
}

}  // extern "C"
