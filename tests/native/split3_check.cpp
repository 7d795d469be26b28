// Host-side check of split3 (csrc/tile.h), the fp32 -> three bf16 pieces split of the plain eval layer's matrix product (CPU
// only; built and run by tests/test_split3_host.py as a program of its own).  Over 2^24 random bit patterns and, for every
// exponent and both signs, the all-zero, all-ones and 23 single-bit significands:
//   finite a      hi + mid + lo == a bit for bit in fp32 (either association) for |a| >= 2^-110, within 2^-133 below that (the
//                 two cases of tile.h's comment); every piece has zero low 16 bits (one bf16 value), is finite, and is zero or
//                 has a's sign;
//   non-finite a  at least one piece is non-finite (the kernel then returns a non-finite row, as tile.h's comment lists).
// Exit code 0 and the line "split3_check: 0 failure(s) over N values" = all of that held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../echoglad_amd/csrc/tile.h"

static uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }
static float from_bits(uint32_t u) { float v; std::memcpy(&v, &u, 4); return v; }

static long failures = 0, checked = 0, subnormal_pieces = 0, tiny = 0;

static void fail(uint32_t u, const char* what, float hi, float mid, float lo) {
    if (++failures <= 20) std::printf("FAIL %08x: %s (hi %08x mid %08x lo %08x)\n", u, what, bits(hi), bits(mid), bits(lo));
}

static void check(uint32_t u) {
    ++checked;
    const float a = from_bits(u);
    float hi, mid, lo;
    eg::split3(a, hi, mid, lo);
    if (!std::isfinite(a)) {
        if (std::isfinite(hi) && std::isfinite(mid) && std::isfinite(lo)) fail(u, "non-finite input, finite pieces", hi, mid, lo);
        return;
    }
    const float pieces[3] = {hi, mid, lo};
    for (float p : pieces) {
        if (bits(p) & 0xFFFFu) fail(u, "piece is not a bf16 value", hi, mid, lo);
        if (!std::isfinite(p)) fail(u, "finite input, non-finite piece", hi, mid, lo);
        if (p != 0.0f && (bits(p) >> 31) != (u >> 31)) fail(u, "piece with the other sign", hi, mid, lo);
        if (p != 0.0f && std::fabs(p) < 1.17549435e-38f) ++subnormal_pieces;
    }
    volatile float s1 = hi + mid;
    volatile float s = s1 + lo;
    volatile float t1 = mid + lo;
    volatile float t = hi + t1;
    if (std::fabs(a) >= 0x1p-110f) {
        if (bits(s) != u || bits(t) != u) fail(u, "pieces do not sum to the input", hi, mid, lo);
    } else {
        // below 2^-110 (tile.h): the mask on a subnormal remainder keeps the bits worth >= 2^-133; -0 gives (-0, +0, +0)
        ++tiny;
        if (std::fabs((double)a - ((double)hi + (double)mid + (double)lo)) >= 0x1p-133) fail(u, "tiny input, error >= 2^-133", hi, mid, lo);
    }
}

int main() {
    uint64_t x = 0x9E3779B97F4A7C15ull;                      // xorshift64*: every bit pattern is as likely as any other
    for (long i = 0; i < (1l << 24) + 4096; ++i) {
        x ^= x >> 12; x ^= x << 25; x ^= x >> 27;
        check((uint32_t)((x * 0x2545F4914F6CDD1Dull) >> 32));
    }
    for (uint32_t sign = 0; sign < 2; ++sign)
        for (uint32_t e = 0; e < 256; ++e) {
            const uint32_t base = (sign << 31) | (e << 23);
            check(base);
            check(base | 0x7FFFFFu);
            for (int b = 0; b < 23; ++b) check(base | (1u << b));
        }
    std::printf("split3_check: %ld failure(s) over %ld values (%ld of them below 2^-110, %ld pieces below the normal range)\n",
                failures, checked, tiny, subnormal_pieces);
    return failures ? 1 : 0;
}
