// Host check of the identity behind Row::div_small_int (csrc/device_utils.h): for d = 1, 2, 4, 8, 16 and every fp32 x,
//     x / d   and   x * (1 / d)
// are the same bits under IEEE round-to-nearest with subnormals kept (the forward kernels' float mode) - both are the
// correctly rounded value of the same real number.  Runs every STRIDE-th bit pattern of the whole 32-bit range
// (default 1: all of them) plus, whatever the stride, every subnormal of both signs, +-0, +-inf, +-FLT_MAX, the
// smallest normals and a set of NaNs; NaN results compare as NaN.  The divisors are read through volatiles so that
// the compiler emits real divisions.
//   c++ -O2 -o div_pow2_check tools/micro/div_pow2_check.cpp && ./div_pow2_check [STRIDE]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static inline float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static inline uint32_t to_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static volatile float g_div[5] = {1.0f, 2.0f, 4.0f, 8.0f, 16.0f};
static volatile float g_rcp[5] = {1.0f, 0.5f, 0.25f, 0.125f, 0.0625f};

int main(int argc, char **argv)
{
    const uint64_t stride = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    if (stride == 0) { std::fprintf(stderr, "stride must be >= 1\n"); return 2; }
    float d[5], r[5];
    for (int q = 0; q < 5; ++q) { d[q] = g_div[q]; r[q] = g_rcp[q]; }
    uint64_t checked = 0, bad = 0, nan_in = 0, sub_out = 0;
    auto check = [&](uint32_t u) {
        const float x = from_bits(u);
        nan_in += std::isnan(x);
        for (int q = 0; q < 5; ++q) {
            const float a = x / d[q], b = x * r[q];
            ++checked;
            sub_out += (a != 0.0f && std::fabs(a) < 1.17549435e-38f);
            const bool same = (std::isnan(a) && std::isnan(b)) || to_bits(a) == to_bits(b);
            if (!same && bad++ < 10) std::printf("MISMATCH x=%08x d=%g: %08x vs %08x\n", u, d[q], to_bits(a), to_bits(b));
        }
    };
    for (uint64_t u = 0; u < (1ull << 32); u += stride) check((uint32_t)u);
    if (stride != 1) {
        for (uint32_t m = 0; m < (1u << 23); ++m) { check(m); check(0x80000000u | m); }          // +-0 and every subnormal
        const uint32_t special[] = {0x7F800000u, 0xFF800000u, 0x7F7FFFFFu, 0xFF7FFFFFu, 0x00800000u, 0x80800000u,
                                    0x00800001u, 0x00FFFFFFu, 0x01000000u, 0x027FFFFFu, 0x7FC00000u, 0xFFC00000u,
                                    0x7F800001u, 0x7FFFFFFFu, 0xFF800001u, 0xFFFFFFFFu, 0x7FA00000u};
        for (uint32_t u : special) check(u);
    }
    std::printf("stride %llu: %llu quotient pairs compared (%llu NaN inputs, %llu subnormal quotients), %llu mismatches\n",
                (unsigned long long)stride, (unsigned long long)checked, (unsigned long long)nan_in,
                (unsigned long long)sub_out, (unsigned long long)bad);
    return bad ? 1 : 0;
}
