// stats_divisor (tbraymarcherplugin_amd/csrc/tbrm_stats_divisor.h) against the division it replaces in the UNORM binning rule:
// floor(x / d) == mulhi(x, mul) >> shift for x < 2^28, 1 <= d <= 65536. (d = 1 is the range lo == hi: it only ever divides 0.)
// The quotient can only go wrong just below a multiple of d, and the multiply-shift's excess grows with x, so per divisor the
// multiples q * d nearest 2^28 decide; the first multiples and a spread in between are checked as well, each with the value before
// it, and every dividend the kernel forms — (code - lo) * n_bins — for a few n_bins at the top code.
#include "../../tbraymarcherplugin_amd/csrc/tbrm_stats_divisor.h"

#include <cstdint>
#include <cstdio>
#include <initializer_list>

namespace {
constexpr uint32_t kLimit = 1u << 28;
unsigned long long checked = 0, wrong = 0;

void check(uint32_t x, uint32_t d, uint32_t mul, uint32_t shift)
{
    const uint32_t got = (uint32_t) (((uint64_t) x * mul) >> 32) >> shift;
    ++checked;
    if (got != x / d && wrong++ < 10) std::printf("x=%u d=%u mul=%u shift=%u: %u, not %u\n", x, d, mul, shift, got, x / d);
}
} // namespace

int main()
{
    { // d = 1 divides 0 only
        uint32_t mul = 1, shift = 1;
        tbrm::stats_divisor(1, mul, shift);
        check(0, 1, mul, shift);
    }
    for (uint32_t d = 2; d <= 65536; ++d) {
        uint32_t mul = 0, shift = 0;
        tbrm::stats_divisor(d, mul, shift);
        if (shift > 12 || ((uint64_t) mul * d) >> (32 + shift) != 1) { std::printf("d=%u: mul=%u shift=%u\n", d, mul, shift); ++wrong; }
        const uint32_t top = (kLimit - 1) / d; // the largest quotient
        check(kLimit - 1, d, mul, shift);
        for (uint32_t j = 0; j < 64; ++j) {
            const uint32_t qs[3] = {j + 1, top > j ? top - j : 1, (uint32_t) (((uint64_t) top * (j + 1)) / 65) + 1};
            for (uint32_t q : qs) {
                if (q > top) continue;
                check(q * d, d, mul, shift);
                check(q * d - 1, d, mul, shift);
            }
        }
        for (uint32_t n_bins : {1u, 7u, 256u, 1000u, 4095u, 4096u}) {
            check((d - 1) * n_bins, d, mul, shift); // the top code of the range: the last bin
            check((d / 2) * n_bins, d, mul, shift);
        }
    }
    std::printf("checked=%llu wrong=%llu\n", checked, wrong);
    return wrong ? 1 : 0;
}
