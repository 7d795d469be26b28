// Host-side check of the UNet front-end's entry points under AddressSanitizer + UBSan (CPU only; built and run by
// tests/test_frontend_abi_sanitized.py).  Every call here must be refused on the host, before any launch: the pointers are
// host addresses that no kernel may ever see.  Exit code 0 = every call returned what it should, left a message, and the
// sanitizers stayed silent (they abort the process otherwise).
#include <cstdio>
#include <cstring>

#include "../../include/echoglad_hip.h"

static int failures = 0;
static void expect(int rc, int want, const char* what) {
    const char* msg = eg_last_error();
    if (rc != want || !msg || std::strlen(msg) == 0) {
        std::printf("FAIL: %s returned %d, expected %d (%s)\n", what, rc, want, msg ? msg : "(null)");
        ++failures;
    }
}

int main() {
    float d[16] = {0};
    float *x = d, *w = d + 4, *m = d + 8, *o = d + 12;
    // eg_conv3x3_relu_bn_fwd(x0, c0, side0, x1, c1, batch, side, weight, bias, bn_weight, bn_bias, bn_mean, bn_var, bn_eps, c_out, out, stream)
    expect(eg_conv3x3_relu_bn_fwd(nullptr, 4, 8, nullptr, 0, 1, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, o, nullptr), EG_ERR_ARG, "conv(x0 = NULL)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, nullptr, 0, 1, 8, nullptr, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, o, nullptr), EG_ERR_ARG, "conv(weight = NULL)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, nullptr, 0, 1, 8, w, nullptr, nullptr, nullptr, nullptr, m, 1e-5f, 4, o, nullptr), EG_ERR_ARG, "conv(bn_mean = NULL)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, nullptr, 0, 1, 8, w, nullptr, nullptr, nullptr, m, nullptr, 1e-5f, 4, o, nullptr), EG_ERR_ARG, "conv(bn_var = NULL)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, nullptr, 0, 1, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, nullptr, nullptr), EG_ERR_ARG, "conv(out = NULL)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, nullptr, 0, 0, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, o, nullptr), EG_ERR_ARG, "conv(batch = 0)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, nullptr, 0, -3, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, o, nullptr), EG_ERR_ARG, "conv(batch < 0)");
    expect(eg_conv3x3_relu_bn_fwd(x, 0, 8, nullptr, 0, 1, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, o, nullptr), EG_ERR_ARG, "conv(c0 = 0)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, nullptr, 0, 1, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 0, o, nullptr), EG_ERR_ARG, "conv(c_out = 0)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, x, -1, 1, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, o, nullptr), EG_ERR_ARG, "conv(c1 < 0)");
    expect(eg_conv3x3_relu_bn_fwd(x, 513, 8, nullptr, 0, 1, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, o, nullptr), EG_ERR_UNSUPPORTED, "conv(c0 = 513)");
    expect(eg_conv3x3_relu_bn_fwd(x, 300, 8, w, 300, 1, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, o, nullptr), EG_ERR_UNSUPPORTED, "conv(c0 + c1 = 600)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, nullptr, 0, 1, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 513, o, nullptr), EG_ERR_UNSUPPORTED, "conv(c_out = 513)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, nullptr, 0, 1, 513, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, o, nullptr), EG_ERR_UNSUPPORTED, "conv(side = 513)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 600, nullptr, 0, 1, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, o, nullptr), EG_ERR_UNSUPPORTED, "conv(side0 = 600)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, nullptr, 0, 1, 0, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, o, nullptr), EG_ERR_ARG, "conv(side = 0)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, nullptr, 4, 1, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, o, nullptr), EG_ERR_ARG, "conv(c1 > 0, x1 = NULL)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, w, 0, 1, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, o, nullptr), EG_ERR_ARG, "conv(x1 with c1 = 0)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, nullptr, 0, 1, 8, w, nullptr, nullptr, nullptr, m, m, -1.f, 4, o, nullptr), EG_ERR_ARG, "conv(bn_eps < 0)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, nullptr, 0, 1, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, x, nullptr), EG_ERR_ARG, "conv(out aliases x0)");
    expect(eg_conv3x3_relu_bn_fwd(x, 4, 8, nullptr, 0, 70000, 8, w, nullptr, nullptr, nullptr, m, m, 1e-5f, 4, o, nullptr), EG_ERR_UNSUPPORTED, "conv(batch = 70000)");
    // eg_adaptive_max_pool_fwd(x, planes, side_in, side_out, out, stream)
    expect(eg_adaptive_max_pool_fwd(nullptr, 4, 8, 4, o, nullptr), EG_ERR_ARG, "pool(x = NULL)");
    expect(eg_adaptive_max_pool_fwd(x, 4, 8, 4, nullptr, nullptr), EG_ERR_ARG, "pool(out = NULL)");
    expect(eg_adaptive_max_pool_fwd(x, 0, 8, 4, o, nullptr), EG_ERR_ARG, "pool(planes = 0)");
    expect(eg_adaptive_max_pool_fwd(x, 4, 8, 9, o, nullptr), EG_ERR_ARG, "pool(side_out > side_in)");
    expect(eg_adaptive_max_pool_fwd(x, 4, 8, 0, o, nullptr), EG_ERR_ARG, "pool(side_out = 0)");
    expect(eg_adaptive_max_pool_fwd(x, 4, 513, 4, o, nullptr), EG_ERR_UNSUPPORTED, "pool(side_in = 513)");
    expect(eg_adaptive_max_pool_fwd(x, 4, 8, 4, x, nullptr), EG_ERR_ARG, "pool(out aliases x)");
    std::printf("frontend_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
