// The rules of tbrm_compete_labels (tbraymarcherplugin_amd/csrc/tbrm_compete_plan.h) on their own, against restatements that take
// another road: the validation bound by bound, the float code against double arithmetic at the clamp ends and at ties, the weight
// at the format extremes, key packing at the limit 2^24 - 1 with the largest weight in 64 bits (no 32-bit overflow), and the scratch
// size of boxes of widths 1, 7, 8, 9, 17 against bricks counted voxel by voxel. Pure host code, no device;
// tests/test_compete_abi.py builds it with -fsanitize=address,undefined and runs it. Prints "failures=N" last.
#include "../../tbraymarcherplugin_amd/csrc/tbrm_compete_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <set>

using namespace tbrm;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
        }                                                                  \
    } while (0)

static int verdict(int conn, int measure, int s0, int s1, int s2, int shift, uint32_t limit, int reserved, double lo, double hi, double top, float o, float s)
{
    const int32_t step[3] = {s0, s1, s2};
    return compete_arguments(conn, measure, step, shift, limit, reserved, lo, hi, top, o, s).what;
}

// the code of a float voxel in double: the difference and the product each rounded to float32, then the clamp and the rounding
static uint32_t code_in_double(float v, float o, float s)
{
    const float d = (float) ((double) v - (double) o);
    const float m = (float) ((double) d * (double) s); // (a product of two float32 is exact in double: one rounding)
    if (m != m) return 0u;
    double c = m < 0.0f ? 0.0 : (m > 65535.0f ? 65535.0 : (double) m);
    const double f = std::floor(c), frac = c - f;
    if (frac > 0.5 || (frac == 0.5 && std::fmod(f, 2.0) == 1.0)) return (uint32_t) f + 1u; // to nearest, ties to even
    return (uint32_t) f;
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    { // validation: every bound, from both sides
        CHECK(verdict(6, 0, 1, 1, 1, 0, 0, 0, 0, 255, 255, 0, 0) == COMPETE_OK);
        CHECK(verdict(6, 1, 0, 65535, 7, 16, kCompeteMaxCost, 0, 3, 65535, 65535, 0, 0) == COMPETE_OK);
        CHECK(verdict(26, 0, 1, 1, 1, 0, 0, 0, 0, 255, 255, 0, 0) == COMPETE_CONNECTIVITY);
        CHECK(verdict(0, 0, 1, 1, 1, 0, 0, 0, 0, 255, 255, 0, 0) == COMPETE_CONNECTIVITY);
        CHECK(verdict(6, 2, 1, 1, 1, 0, 0, 0, 0, 255, 255, 0, 0) == COMPETE_MEASURE);
        CHECK(verdict(6, -1, 1, 1, 1, 0, 0, 0, 0, 255, 255, 0, 0) == COMPETE_MEASURE);
        for (int a = 0; a < 3; ++a)
            for (int bad : {-1, 65536}) {
                int32_t step[3] = {1, 1, 1};
                step[a] = bad;
                const CompeteVerdict v = compete_arguments(6, 0, step, 0, 0, 0, 0, 255, 255, 0, 0);
                CHECK(v.what == COMPETE_STEP_COST && v.axis == a);
            }
        CHECK(verdict(6, 0, 1, 1, 1, -1, 0, 0, 0, 255, 255, 0, 0) == COMPETE_SHIFT);
        CHECK(verdict(6, 0, 1, 1, 1, 17, 0, 0, 0, 255, 255, 0, 0) == COMPETE_SHIFT);
        CHECK(verdict(6, 0, 1, 1, 1, 0, kCompeteMaxCost + 1u, 0, 0, 255, 255, 0, 0) == COMPETE_LIMIT);
        CHECK(verdict(6, 0, 1, 1, 1, 0, 0xFFFFFFFFu, 0, 0, 255, 255, 0, 0) == COMPETE_LIMIT);
        CHECK(verdict(6, 0, 1, 1, 1, 0, 0, 1, 0, 255, 255, 0, 0) == COMPETE_RESERVED);
        CHECK(verdict(6, 0, 1, 1, 1, 0, 0, 0, 9, 8, 255, 0, 0) == COMPETE_RANGE);
        CHECK(verdict(6, 0, 1, 1, 1, 0, 0, 0, (double) nan, 8, 255, 0, 0) == COMPETE_RANGE);
        CHECK(verdict(6, 0, 1, 1, 1, 0, 0, 0, -1, 8, 255, 0, 0) == COMPETE_RANGE_CODES);
        CHECK(verdict(6, 0, 1, 1, 1, 0, 0, 0, 0, 256, 255, 0, 0) == COMPETE_RANGE_CODES);
        CHECK(verdict(6, 0, 1, 1, 1, 0, 0, 0, 0.5, 8, 255, 0, 0) == COMPETE_RANGE_CODES);
        CHECK(verdict(6, 0, 1, 1, 1, 0, 0, 0, 0, 256, 65535, 0, 0) == COMPETE_OK);
        CHECK(verdict(6, 0, 1, 1, 1, 0, 0, 0, -2.5, 8.25, 0, 0, 1) == COMPETE_OK); // a float volume: any finite range
        CHECK(verdict(6, 0, 1, 1, 1, 0, 0, 0, -2.5, (double) inf, 0, 0, 1) == COMPETE_RANGE_FLOAT);
        CHECK(verdict(6, 0, 1, 1, 1, 0, 0, 0, -2.5, 1e300, 0, 0, 1) == COMPETE_RANGE_FLOAT); // finite, but not as float32
        for (float s : {0.0f, -1.0f, inf, nan}) CHECK(verdict(6, 0, 1, 1, 1, 0, 0, 0, 0, 1, 0, 0, s) == COMPETE_FLOAT_SCALE);
        for (float o : {inf, -inf, nan}) CHECK(verdict(6, 0, 1, 1, 1, 0, 0, 0, 0, 1, 0, o, 1) == COMPETE_FLOAT_ORIGIN);
        CHECK(verdict(6, 0, 1, 1, 1, 0, 0, 0, 0, 255, 255, nan, nan) == COMPETE_OK); // UNORM volumes ignore the float fields
        CHECK(compete_limit(0) == kCompeteMaxCost && compete_limit(1) == 1 && compete_limit(kCompeteMaxCost) == kCompeteMaxCost);
    }
    { // the float range
        float o = 0, s = 0;
        CHECK(compete_float_range(-1000.0, 3000.0, &o, &s) && o == -1000.0f && s == (float) (65535.0 / 4000.0));
        CHECK(compete_float_range(0.0, 1.0, &o, &s) && o == 0.0f && s == 65535.0f);
        o = 5.0f;
        CHECK(!compete_float_range(1.0, 1.0, &o, &s) && !compete_float_range(2.0, 1.0, &o, &s) && !compete_float_range(0.0, (double) inf, &o, &s));
        CHECK(!compete_float_range((double) nan, 1.0, &o, &s) && !compete_float_range(0.0, 1e-320, &o, &s) && !compete_float_range(-1e300, 1e300, &o, &s));
        CHECK(o == 5.0f); // a refusal writes nothing
    }
    { // the code: the clamp ends, ties to even, NaN, and a sweep against double arithmetic
        CHECK(compete_float_code(-5.0f, 0.0f, 1.0f) == 0u && compete_float_code(0.0f, 0.0f, 1.0f) == 0u && compete_float_code(-0.0f, 0.0f, 1.0f) == 0u);
        CHECK(compete_float_code(65535.0f, 0.0f, 1.0f) == 65535u && compete_float_code(65535.4f, 0.0f, 1.0f) == 65535u && compete_float_code(1e30f, 0.0f, 1.0f) == 65535u);
        CHECK(compete_float_code(inf, 0.0f, 1.0f) == 65535u && compete_float_code(-inf, 0.0f, 1.0f) == 0u && compete_float_code(nan, 0.0f, 1.0f) == 0u);
        CHECK(compete_float_code(0.5f, 0.0f, 1.0f) == 0u && compete_float_code(1.5f, 0.0f, 1.0f) == 2u && compete_float_code(2.5f, 0.0f, 1.0f) == 2u && compete_float_code(3.5f, 0.0f, 1.0f) == 4u);
        CHECK(compete_float_code(65534.5f, 0.0f, 1.0f) == 65534u && compete_float_code(65533.5f, 0.0f, 1.0f) == 65534u);
        CHECK(compete_float_code(0.50000006f, 0.0f, 1.0f) == 1u && compete_float_code(0.49999997f, 0.0f, 1.0f) == 0u);
        uint32_t state = 12345u;
        for (int i = 0; i < 200000; ++i) {
            state = state * 1664525u + 1013904223u;
            const float v = -1200.0f + 4400.0f * (float) (state >> 8) / 16777216.0f;
            CHECK(compete_float_code(v, -1000.0f, 16.38375f) == code_in_double(v, -1000.0f, 16.38375f));
            if (failures) break;
        }
    }
    { // the weight at the format extremes
        CHECK(compete_weight(0, 0, 0, 0) == 0u && compete_weight(0, 255, 0, 0) == 255u && compete_weight(0, 0, 255, 0) == 255u);
        CHECK(compete_weight(65535, 0, 65535, 0) == 131070u && compete_weight(65535, 65535, 0, 0) == 131070u);
        CHECK(compete_weight(65535, 0, 65535, 16) == 65535u && compete_weight(7, 65535, 0, 15) == 8u && compete_weight(7, 65535, 1, 15) == 8u && compete_weight(7, 32768, 1, 15) == 7u);
        for (uint32_t cu : {0u, 1u, 254u, 255u, 32768u, 65534u, 65535u})
            for (uint32_t cv : {0u, 1u, 255u, 256u, 65535u})
                for (int shift : {0, 1, 8, 15, 16})
                    for (uint32_t step : {0u, 1u, 65535u}) {
                        const long long d = (long long) cu - (long long) cv;
                        CHECK((long long) compete_weight(step, cu, cv, shift) == (long long) step + ((d < 0 ? -d : d) >> shift));
                    }
    }
    { // keys: packing and the offer against 64-bit arithmetic, at the largest limit with the largest weight
        CHECK(compete_key(0, 0) == 0u && compete_key(0, 255) == 255u && compete_key(kCompeteMaxCost, 255) == kCompeteUnreached && compete_key(kCompeteMaxCost, 254) == 0xFFFFFFFEu);
        CHECK(compete_key_cost(0xFFFFFFFEu) == kCompeteMaxCost && compete_key_label(0xFFFFFFFEu) == 254u);
        const uint32_t w_max = compete_weight(65535, 0, 65535, 0);
        for (uint32_t limit : {1u, 2u, 255u, 65535u, kCompeteMaxCost - 1u, kCompeteMaxCost})
            for (uint32_t cost : {0u, 1u, 2u, 255u, 256u, 65535u, kCompeteMaxCost - w_max - 1u, kCompeteMaxCost - w_max, kCompeteMaxCost - w_max + 1u, kCompeteMaxCost - 1u, kCompeteMaxCost})
                for (uint32_t label : {0u, 1u, 254u, 255u})
                    for (uint32_t w : {0u, 1u, 255u, 65535u, w_max}) {
                        const uint64_t sum = (uint64_t) cost + w;
                        const uint64_t want = sum <= limit ? ((sum << 8) | label) : 0xFFFFFFFFull;
                        CHECK(want <= 0xFFFFFFFFull); // (what passes the limit fits the word)
                        CHECK((uint64_t) compete_offer(compete_key(cost, label), w, limit) == want);
                    }
        // an offer is never below the key it was made from, and the unreached word offers nothing that lowers a key
        CHECK(compete_offer(kCompeteUnreached, 0, kCompeteMaxCost) == kCompeteUnreached && compete_offer(kCompeteUnreached, 1, kCompeteMaxCost) == kCompeteUnreached);
        CHECK(compete_offer(kCompeteUnreached, w_max, kCompeteMaxCost) == kCompeteUnreached);
    }
    { // the scratch: 2 KiB of keys, 64 claimable bytes and two activity words per brick the box touches, 256-byte aligned parts
        const CompeteLayout one = compete_layout(1);
        CHECK(one.keys == 0 && one.claim == 2048 && one.act[0] == 2048 + 256 && one.act[1] == 2048 + 512 && one.counts == 2048 + 768);
        CHECK(one.ctl == one.counts + ((size_t) COMPETE_COUNTS * 8 + 255) / 256 * 256 && one.bytes == one.ctl + ((size_t) COMPETE_CTL_WORDS * 4 + 255) / 256 * 256);
        const size_t fixed = one.bytes - one.counts;
        for (int width : {1, 7, 8, 9, 17})
            for (int o = 0; o + width <= 40; ++o) {
                std::set<int> bricks;
                for (int v = o; v < o + width; ++v) bricks.insert(v / 8);
                const size_t nb[3] = {bricks.size(), 2, 3}; // y: [5, 14) touches 2 bricks, z: [3, 20) touches 3
                const size_t n = nb[0] * nb[1] * nb[2];
                const VoxelBox box{{o, 5, 3}, {o + width, 14, 20}};
                auto up = [](size_t b) { return (b + 255) / 256 * 256; };
                CHECK(compete_scratch_bytes(box) == up(n * 2048) + up(n * 64) + 2 * up(n * 4) + fixed);
                const VoxelBox turned{{5, 3, o}, {14, 20, o + width}};
                CHECK(compete_scratch_bytes(turned) == compete_scratch_bytes(box));
            }
        const VoxelBox whole{{0, 0, 0}, {512, 512, 512}}; // a whole 512^3 volume: 512 MiB of keys and 18 MiB beside them
        CHECK(compete_layout(262144).act[0] == (512ull + 16ull) << 20 && compete_scratch_bytes(whole) < (512ull + 19ull) << 20);
    }
    std::printf("failures=%d\n", failures);
    return failures != 0;
}
