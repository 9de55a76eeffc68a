// tbrm_stats_divisor.h — the division of the UNORM binning rule (include/tbrm_volume_stats.h) without a division in the kernel.
// Plain C++, no dependencies: tests/cpp/stats_divisor_test.cpp checks it on the host.
#pragma once
#include <cstdint>

namespace tbrm {

// floor(n / d) = mulhi(n, mul) >> shift for every n < 2^28 (the largest dividend is 65535 * 4096) and 1 <= d <= 65536:
// shift = max(0, ceil(log2 d) - 4) and mul = ceil(2^(32 + shift) / d) give mul * d - 2^(32 + shift) < d <= 2^(4 + shift), which is
// the condition of Granlund & Montgomery's theorem for 28-bit dividends, and mul <= 2^29 + 1 fits a word. d = 1 only ever divides 0.
inline void stats_divisor(uint32_t d, uint32_t& mul, uint32_t& shift)
{
    if (d <= 1) { mul = 0; shift = 0; return; }
    uint32_t lg = 0;
    while (((uint32_t) 1 << lg) < d) ++lg;
    shift = lg > 4 ? lg - 4 : 0;
    const uint64_t two = (uint64_t) 1 << (32 + shift);
    mul = (uint32_t) ((two + d - 1) / d);
}

} // namespace tbrm
