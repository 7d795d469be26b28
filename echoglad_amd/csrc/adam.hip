// The optimizer update of the training step as ONE launch (gfx950): Adam on the multi-tensor kernel of multi_tensor.h.
// The reference trains with torch.optim.Adam (src/engine.py:60-72 via its optimizer builder).  On the GPU torch's fused form is a
// `_foreach_add_` on the step counts plus one multi-tensor launch per ~30 parameter tensors (its pointer table travels in the kernel
// arguments: 4 KB): 4 launches for the 82 tensors of the GNN stack, landmark MLPs and heads -- 34 us of a 0.9-ms captured batch-1 step,
// for 300 KB of parameters.  Here: one launch.  Up to EG_ADAM_MAX_TENSORS (p, grad, exp_avg, exp_avg_sq, numel) entries travel in the
// kernel arguments (3.5 KB), and the step counts -- steps[k] of one device array, one per tensor as in torch's state (a parameter
// without a gradient in some step falls behind the others) -- are advanced by the workgroup that leaves last.
// Arithmetic: torch's fused Adam, ADAM_MODE::ORIGINAL (aten/src/ATen/native/cuda/fused_adam_utils.cuh), amsgrad off:
//     g = grad (+ weight_decay * p);  m = m + (1 - b1) (g - m);  v = b2 v + (1 - b2) g g
//     p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)          t = step + 1, bias corrections in fp64 like there
#include "multi_tensor.h"

namespace eg {

struct AdamOp {
    static constexpr int NP = 4, MAX = EG_ADAM_MAX_TENSORS;     // p, g, exp_avg, exp_avg_sq
    struct Scalars {
        float lr, beta1, beta2, eps, weight_decay;
        int maximize;
        const float* lr_dev;            // nullable: the learning rate as a device scalar (a scheduler's changes reach a captured launch)
        unsigned* ticket;
    };
    const Scalars& a;
    float step_size, bc2_sqrt, w1, w2;

    __device__ AdamOp(const Scalars& a, const float& count) : a(a) {
        const float t_now = count + 1.0f;
        const double bc1 = 1.0 - pow((double)a.beta1, (double)t_now), bc2 = 1.0 - pow((double)a.beta2, (double)t_now);
        const float lr = a.lr_dev ? *a.lr_dev : a.lr;
        step_size = (float)((double)lr / bc1);
        bc2_sqrt = (float)sqrt(bc2);
        w1 = 1.0f - a.beta1;
        w2 = 1.0f - a.beta2;
    }
    __device__ bool used(int) const { return true; }
    __device__ void update(float (&x)[NP]) const {
        const float pi = x[0];
        float gi = a.maximize ? -x[1] : x[1];
        if (a.weight_decay != 0.f) gi += pi * a.weight_decay;
        float mi = x[2], vi = x[3];
        mi = mi + w1 * (gi - mi);
        vi = mt_mul2_add(a.beta2, vi, w2 * gi, gi);
        x[2] = mi;
        x[3] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + a.eps;
        x[0] = pi - step_size * mi / denom;
    }
    static const char* check(const Scalars& a) {
        const bool ok = a.beta1 >= 0.f && a.beta1 < 1.f && a.beta2 >= 0.f && a.beta2 < 1.f && a.eps >= 0.f;
        return ok ? nullptr : "betas must be in [0, 1), eps >= 0";
    }
    static const char* state(const eg_adam_tensor& t, const Scalars&, float* (&s)[2]) {
        s[0] = t.exp_avg;
        s[1] = t.exp_avg_sq;
        return t.exp_avg && t.exp_avg_sq ? nullptr : "bad tensor entry";
    }
};
static_assert(mt_fits<AdamOp>, "the kernel arguments must stay within 4 KB");

}  // namespace eg

using namespace eg;

extern "C" {

int eg_adam_step(const eg_adam_tensor* tensors, int count, float* steps, float lr, const float* lr_device, float beta1, float beta2, float eps,
                 float weight_decay, int maximize, eg_stream_t stream) {
    return mt_launch<AdamOp>(tensors, count, steps, {lr, beta1, beta2, eps, weight_decay, maximize ? 1 : 0, lr_device, nullptr}, stream);
}

}  // extern "C"
