// SGD and RMSprop as ONE launch per step (gfx950): the other two names of the reference's optimizer registry
// (src/builders/optimizer_builder.py: sgd, rmsprop, adam), on the multi-tensor kernel of multi_tensor.h like adam.hip.
// torch.optim.SGD has no capturable form at all and torch.optim.RMSprop(capturable=True) is a chain of _foreach_* launches; a captured
// batch-1 training step (engine.GraphedTrainStep) is host- and launch-bound, so the update is one node here as well.
// Arithmetic: torch's _single_tensor_sgd / _single_tensor_rmsprop, operation by operation (include/echoglad_hip.h spells both out).
// SGD's first update of a tensor copies the gradient into the momentum buffer WITHOUT dampening.  torch decides that on the host
// (`momentum_buffer is None`); here the kernel reads the tensor's device step count, so the launch arguments are the same in step 1 and
// in step 100 -- a captured launch replays correctly from either side of the first update.
#include "multi_tensor.h"

namespace eg {

struct SgdOp {
    static constexpr int NP = 3, MAX = EG_SGD_MAX_TENSORS;      // p, g, momentum buffer (momentum == 0: not read)
    struct Scalars {
        float lr, momentum, dampening, weight_decay;
        int nesterov, maximize;
        const float* lr_dev;                // nullable: the learning rate as a device scalar
        unsigned* ticket;
    };
    const Scalars& a;
    bool has_buf, first;
    float lr, w;

    __device__ SgdOp(const Scalars& a, const float& count) : a(a) {
        has_buf = a.momentum != 0.f;
        first = has_buf && count == 0.f;                        // this tensor's first update: the buffer becomes a copy of g
        lr = a.lr_dev ? *a.lr_dev : a.lr;
        w = 1.0f - a.dampening;
    }
    __device__ bool used(int j) const { return j < 2 || has_buf; }
    __device__ void update(float (&x)[NP]) const {
        const float pi = x[0];
        float gi = a.maximize ? -x[1] : x[1];
        if (a.weight_decay != 0.f) gi = gi + a.weight_decay * pi;
        if (has_buf) {
            const float bi = first ? gi : mt_mul2_add(a.momentum, x[2], w, gi);
            x[2] = bi;
            gi = a.nesterov ? gi + a.momentum * bi : bi;
        }
        x[0] = pi - lr * gi;
    }
    static const char* check(const Scalars& a) {
        if (!(a.momentum >= 0.f)) return "momentum must be >= 0";
        if (!(a.weight_decay >= 0.f)) return "weight_decay must be >= 0";
        if (a.nesterov && (!(a.momentum > 0.f) || a.dampening != 0.f)) return "nesterov momentum requires a momentum and zero dampening";
        return nullptr;
    }
    static const char* state(const eg_sgd_tensor& t, const Scalars& a, float* (&s)[1]) {
        s[0] = t.momentum_buffer;
        return a.momentum != 0.f && !t.momentum_buffer ? "momentum != 0 needs a momentum buffer for every tensor" : nullptr;
    }
};
static_assert(mt_fits<SgdOp>, "the kernel arguments must stay within 4 KB");

struct RmspropOp {
    static constexpr int NP = 5, MAX = EG_RMSPROP_MAX_TENSORS;  // p, g, square_avg, grad_avg (centered only), momentum buffer (momentum > 0 only)
    struct Scalars {
        float lr, alpha, eps, weight_decay, momentum;
        int centered, maximize;
        const float* lr_dev;
        unsigned* ticket;
    };
    const Scalars& a;
    bool has_buf, centered;
    float lr, w;

    __device__ RmspropOp(const Scalars& a, const float&) : a(a) {
        has_buf = a.momentum > 0.f;
        centered = a.centered != 0;
        lr = a.lr_dev ? *a.lr_dev : a.lr;
        w = 1.0f - a.alpha;
    }
    __device__ bool used(int j) const { return j == 3 ? centered : j == 4 ? has_buf : true; }
    __device__ void update(float (&x)[NP]) const {
        const float pi = x[0];
        float gi = a.maximize ? -x[1] : x[1];
        if (a.weight_decay != 0.f) gi = gi + a.weight_decay * pi;
        const float si = mt_mul2_add(a.alpha, x[2], w * gi, gi);
        x[2] = si;
        float avg;
        if (centered) {
            const float ai = x[3] + w * (gi - x[3]);
            x[3] = ai;
            avg = sqrtf(si - ai * ai) + a.eps;
        } else {
            avg = sqrtf(si) + a.eps;
        }
        if (has_buf) {
            const float bi = a.momentum * x[4] + gi / avg;
            x[4] = bi;
            x[0] = pi - lr * bi;
        } else {
            x[0] = pi - lr * gi / avg;
        }
    }
    static const char* check(const Scalars& a) {
        const bool ok = a.alpha >= 0.f && a.eps >= 0.f && a.momentum >= 0.f && a.weight_decay >= 0.f;
        return ok ? nullptr : "alpha, eps, momentum and weight_decay must be >= 0";
    }
    static const char* state(const eg_rmsprop_tensor& t, const Scalars& a, float* (&s)[3]) {
        s[0] = t.square_avg;
        s[1] = t.grad_avg;
        s[2] = t.momentum_buffer;
        if (!t.square_avg) return "bad tensor entry";
        if ((t.grad_avg != nullptr) != (a.centered != 0)) return "grad_avg must be given exactly when centered is set";
        if ((t.momentum_buffer != nullptr) != (a.momentum > 0.f)) return "momentum_buffer must be given exactly when momentum > 0";
        return nullptr;
    }
};
// five pointers per tensor: 84 entries (the default landmark model with its coordinate graph has 82 parameter tensors, 84 with a 1 x 1
// embedder) fill 4016 of the 4096 bytes
static_assert(mt_fits<RmspropOp>, "the kernel arguments must stay within 4 KB");

}  // namespace eg

using namespace eg;

extern "C" {

int eg_sgd_step(const eg_sgd_tensor* tensors, int count, float* steps, float lr, const float* lr_device, float momentum, float dampening,
                float weight_decay, int nesterov, int maximize, eg_stream_t stream) {
    return mt_launch<SgdOp>(tensors, count, steps, {lr, momentum, dampening, weight_decay, nesterov ? 1 : 0, maximize ? 1 : 0, lr_device, nullptr},
                            stream);
}

int eg_rmsprop_step(const eg_rmsprop_tensor* tensors, int count, float* steps, float lr, const float* lr_device, float alpha, float eps,
                    float weight_decay, float momentum, int centered, int maximize, eg_stream_t stream) {
    return mt_launch<RmspropOp>(tensors, count, steps,
                                {lr, alpha, eps, weight_decay, momentum, centered ? 1 : 0, maximize ? 1 : 0, lr_device, nullptr}, stream);
}

}  // extern "C"
