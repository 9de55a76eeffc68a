// scissors_plan_test.cpp — the host-compilable rules of view-space scissors (tbrm_scissors_plan.h) against loops: the
// exact floor division, the bound check, the corner rectangle, the mask summary, the verdict and the polygon fill. Stand-alone: no
// device, no library. tests/test_scissors_abi.py builds it with -fsanitize=address,undefined and runs it.
#include "../../tbraymarcherplugin_amd/csrc/tbrm_scissors_plan.h"

#include <cstdio>
#include <random>
#include <vector>

using namespace tbrm;

static int failures = 0;
#define CHECK(cond, ...)                                                                                                  \
    do {                                                                                                                  \
        if (!(cond)) {                                                                                                    \
            if (++failures <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                                                 \
    } while (0)

static std::mt19937_64 rng(20261020);
static int64_t uniform(int64_t lo, int64_t hi) { return std::uniform_int_distribution<int64_t>(lo, hi)(rng); }

// floor(U / W) by the language's own division
static int64_t floor_div(int64_t U, int64_t W)
{
    int64_t q = U / W;
    if ((U % W != 0) && ((U < 0) != (W < 0))) --q;
    return q;
}

static void test_quotient()
{
    const int64_t top = 1ll << kScissorsCoordBits;
    for (int t = 0; t < 400000; ++t) {
        const int n = (int) uniform(1, kScissorsMaxImage);
        const int bits = (int) uniform(0, kScissorsCoordBits);
        int64_t W = bits == 0 ? 1 : uniform(1ll << (bits - 1), (1ll << bits) - 1);
        if (t % 7 == 0) W = top - 1 - uniform(0, 3);
        const int64_t q = t % 5 == 0 ? n - 1 : uniform(0, n - 1);
        const int64_t r = t % 3 == 0 ? 0 : (t % 3 == 1 ? W - 1 : uniform(0, W - 1));
        const int64_t U = q * W + r; // < n * W < 2^60
        const float rcp = scissors_rcp(W);
        CHECK(scissors_quotient(U, W, rcp, n) == q, "U %lld W %lld n %d", (long long) U, (long long) W, n);
        CHECK(scissors_pixel(U, W, rcp, n) == q, "U %lld W %lld n %d", (long long) U, (long long) W, n);
        // beyond the frame on either side, and exactly on its edges
        CHECK(scissors_pixel(-1 - r, W, rcp, n) == -1, "negative U");
        CHECK(scissors_pixel((int64_t) n * W + r, W, rcp, n) == n, "U beyond n W");
        CHECK(scissors_pixel((int64_t) n * W - 1, W, rcp, n) == n - 1, "the last pixel");
        CHECK(scissors_pixel(0, W, rcp, n) == 0, "U = 0");
        // the clamp agrees with the plain floor division wherever that is in range
        const int64_t any = uniform(-top + 1, top - 1), f = floor_div(any, W);
        const int64_t want = f < 0 ? -1 : (f >= n ? n : f);
        CHECK(scissors_pixel(any, W, rcp, n) == want, "U %lld W %lld n %d", (long long) any, (long long) W, n);
    }
}

static void test_bounds()
{
    const __int128 limit = (__int128) 1 << kScissorsCoordBits;
    for (int t = 0; t < 200000; ++t) {
        int dims[3];
        for (int c = 0; c < 3; ++c) dims[c] = t % 11 == 0 ? 1 : (int) uniform(1, t % 2 ? 600 : 70000);
        int64_t r[4];
        for (int c = 0; c < 4; ++c) {
            const int bits = (int) uniform(0, 62);
            r[c] = uniform(0, (1ll << bits)) * (uniform(0, 1) ? 1 : -1);
        }
        if (t % 13 == 0) r[(int) uniform(0, 3)] = INT64_MIN;
        if (t % 3 == 0) { // just round the limit
            const int c = (int) uniform(0, 3);
            r[0] = r[1] = r[2] = r[3] = 0;
            const int64_t n = c < 3 ? (dims[c] > 1 ? dims[c] - 1 : 1) : 1;
            r[c] = ((int64_t) (limit / n) + uniform(-1, 1)) * (uniform(0, 1) ? 1 : -1);
        }
        __int128 sum = 0;
        for (int c = 0; c < 4; ++c) {
            const __int128 a = r[c] < 0 ? -(__int128) r[c] : (__int128) r[c];
            sum += a * (c < 3 ? dims[c] - 1 : 1);
        }
        CHECK(scissors_row_admissible(r, dims) == (sum < limit), "row (%lld %lld %lld %lld) dims (%d %d %d)", (long long) r[0], (long long) r[1], (long long) r[2], (long long) r[3], dims[0], dims[1], dims[2]);
    }
    tbrm_scissors_projection p{};
    const int dims[3] = {40, 24, 19};
    p.w[3] = 4; p.w_min = 1; p.w_max = 4; p.width = 1; p.height = kScissorsMaxImage;
    CHECK(scissors_arguments(p, 0, dims) == SCISSORS_OK, "the smallest and the largest image");
    p.width = 0; CHECK(scissors_arguments(p, 0, dims) == SCISSORS_WIDTH, "width 0");
    p.width = kScissorsMaxImage + 1; CHECK(scissors_arguments(p, 0, dims) == SCISSORS_WIDTH, "width beyond");
    p.width = 8; p.height = 0; CHECK(scissors_arguments(p, 0, dims) == SCISSORS_HEIGHT, "height 0");
    p.height = 8; p.u[0] = 1ll << 41; CHECK(scissors_arguments(p, 0, dims) == SCISSORS_U, "u");
    p.u[0] = 0; p.v[3] = -(1ll << 46); CHECK(scissors_arguments(p, 0, dims) == SCISSORS_V, "v");
    p.v[3] = -(1ll << 46) + 1; CHECK(scissors_arguments(p, 0, dims) == SCISSORS_OK, "v just inside");
    p.w[2] = 1ll << 42; CHECK(scissors_arguments(p, 0, dims) == SCISSORS_W, "w");
    p.w[2] = 0; p.w_min = 0; CHECK(scissors_arguments(p, 0, dims) == SCISSORS_W_MIN, "w_min");
    p.w_min = 5; CHECK(scissors_arguments(p, 0, dims) == SCISSORS_W_MAX, "w_max");
    p.w_min = 4; CHECK(scissors_arguments(p, 4, dims) == SCISSORS_OP && scissors_arguments(p, -1, dims) == SCISSORS_OP && scissors_arguments(p, 3, dims) == SCISSORS_OK, "op");
    // stray bits
    std::vector<uint32_t> words(scissors_mask_words(33, 3), 0xffffffffu);
    CHECK(scissors_mask_stray_row(words.data(), 33, 3) == 0, "stray bits in row 0");
    for (int y = 0; y < 3; ++y) words[(size_t) y * 2 + 1] = 1u;
    CHECK(scissors_mask_stray_row(words.data(), 33, 3) == -1, "no stray bits");
    words[5] = 3u;
    CHECK(scissors_mask_stray_row(words.data(), 33, 3) == 2, "stray bit in row 2");
    CHECK(scissors_mask_stray_row(words.data(), 64, 3) == -1, "a width of whole words has none");
}

// the summary of a mask by loops: the kernels' three steps, one after the other
static std::vector<ScissorsCell> summary_of(const std::vector<uint32_t>& words, int width, int height)
{
    const int cw = scissors_cells_x(width), ch = scissors_cells_y(height), pitch = cw + 1;
    std::vector<ScissorsCell> sat(scissors_summary_entries(width, height), ScissorsCell{0u, 0u});
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            bool full = true, clear = true;
            for (int y = cy * kScissorsCellRows; y < (cy + 1) * kScissorsCellRows && y < height; ++y)
                for (int x = cx * 32; x < cx * 32 + 32 && x < width; ++x) {
                    const bool bit = (words[(size_t) y * scissors_row_words(width) + (size_t) (x >> 5)] >> (x & 31)) & 1u;
                    full = full && bit;
                    clear = clear && !bit;
                }
            sat[(size_t) (cy + 1) * pitch + cx + 1] = ScissorsCell{full ? 1u : 0u, clear ? 1u : 0u};
        }
    for (int y = 1; y <= ch; ++y)
        for (int x = 1; x <= cw; ++x) {
            ScissorsCell& e = sat[(size_t) y * pitch + x];
            const ScissorsCell a = sat[(size_t) (y - 1) * pitch + x], b = sat[(size_t) y * pitch + x - 1], c = sat[(size_t) (y - 1) * pitch + x - 1];
            e.full += a.full + b.full - c.full;
            e.clear += a.clear + b.clear - c.clear;
        }
    return sat;
}

static bool bit_of(const std::vector<uint32_t>& words, int width, int px, int py) { return (words[(size_t) py * scissors_row_words(width) + (size_t) (px >> 5)] >> (px & 31)) & 1u; }

static std::vector<uint32_t> random_mask(int width, int height, int kind)
{
    std::vector<uint32_t> words(scissors_mask_words(width, height), 0u);
    const int ex = (int) uniform(0, width), ey = (int) uniform(0, height);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const bool bit = kind == 0 ? x < ex : (kind == 1 ? y >= ey : (kind == 2 ? true : (kind == 3 ? false : ((x / 40 + y / 24) & 1))));
            if (bit) words[(size_t) y * scissors_row_words(width) + (size_t) (x >> 5)] |= 1u << (x & 31);
        }
    return words;
}

static void test_summary()
{
    int told = 0;
    for (int t = 0; t < 60; ++t) {
        const int width = (int) uniform(1, 200), height = (int) uniform(1, 90);
        const std::vector<uint32_t> words = random_mask(width, height, t % 5);
        const std::vector<ScissorsCell> sat = summary_of(words, width, height);
        for (int k = 0; k < 300; ++k) {
            const int x0 = (int) uniform(0, width - 1), x1 = (int) uniform(x0, width - 1), y0 = (int) uniform(0, height - 1), y1 = (int) uniform(y0, height - 1);
            bool all = true, none = true;
            for (int y = y0; y <= y1; ++y)
                for (int x = x0; x <= x1; ++x) { const bool b = bit_of(words, width, x, y); all = all && b; none = none && !b; }
            const int s = scissors_summary_query(sat.data(), scissors_cells_x(width), x0, y0, x1, y1);
            CHECK(s != SCISSORS_ALL_SET || all, "all set claimed: %d x %d, (%d %d) .. (%d %d)", width, height, x0, y0, x1, y1);
            CHECK(s != SCISSORS_ALL_CLEAR || none, "all clear claimed: %d x %d, (%d %d) .. (%d %d)", width, height, x0, y0, x1, y1);
            told += s != SCISSORS_NEITHER;
        }
        if (t % 5 == 2) CHECK(scissors_summary_query(sat.data(), scissors_cells_x(width), 0, 0, width - 1, height - 1) == SCISSORS_ALL_SET, "a full mask is all set, ragged last word and rows included");
        if (t % 5 == 3) CHECK(scissors_summary_query(sat.data(), scissors_cells_x(width), 0, 0, width - 1, height - 1) == SCISSORS_ALL_CLEAR, "an empty mask is all clear");
    }
    CHECK(told > 3000, "the summary tells something: %d", told);
}

static bool in_M(const ScissorsRows& p, const std::vector<uint32_t>& words, int x, int y, int z)
{
    const int64_t U = scissors_dot(p.u, x, y, z), V = scissors_dot(p.v, x, y, z), W = scissors_dot(p.w, x, y, z);
    if (W <= 0 || W < p.w_min || W > p.w_max) return false;
    const int64_t px = floor_div(U, W), py = floor_div(V, W);
    return px >= 0 && px < p.width && py >= 0 && py < p.height && bit_of(words, p.width, (int) px, (int) py);
}

static void test_corners_and_verdict()
{
    int verdicts[3] = {0, 0, 0}, straddle = 0;
    for (int t = 0; t < 400; ++t) {
        const int dims[3] = {(int) uniform(1, 30), (int) uniform(1, 30), (int) uniform(1, 30)};
        ScissorsRows p{};
        p.width = (int) uniform(1, 160);
        p.height = (int) uniform(1, 120);
        const int64_t s = uniform(1, 64);
        for (int c = 0; c < 3; ++c) { p.u[c] = uniform(-8, 8) * s; p.v[c] = uniform(-8, 8) * s; p.w[c] = t % 3 ? uniform(-2, 2) * s / 4 : 0; }
        p.u[3] = uniform(-40, 200) * s;
        p.v[3] = uniform(-40, 200) * s;
        p.w[3] = uniform(t % 3 == 1 ? -4 : 1, 30) * s;
        p.w_min = uniform(1, 8 * s);
        p.w_max = p.w_min + uniform(0, 40 * s);
        const std::vector<uint32_t> words = random_mask(p.width, p.height, t % 5);
        const std::vector<ScissorsCell> sat = summary_of(words, p.width, p.height);
        for (int bz = 0; bz * kBrick < dims[2]; ++bz)
            for (int by = 0; by * kBrick < dims[1]; ++by)
                for (int bx = 0; bx * kBrick < dims[0]; ++bx) {
                    const ScissorsCorners k = scissors_corners(p, dims, bx, by, bz);
                    const int verdict = scissors_verdict(k, p, sat.data(), scissors_cells_x(p.width));
                    ++verdicts[verdict];
                    straddle += k.positive != 0 && k.positive != 8;
                    for (int z = bz * kBrick; z < bz * kBrick + kBrick && z < dims[2]; ++z)
                        for (int y = by * kBrick; y < by * kBrick + kBrick && y < dims[1]; ++y)
                            for (int x = bx * kBrick; x < bx * kBrick + kBrick && x < dims[0]; ++x) {
                                const int64_t W = scissors_dot(p.w, x, y, z);
                                if (k.positive == 0) CHECK(W <= 0, "W <= 0 at every corner, not at (%d %d %d)", x, y, z);
                                if (k.positive == 8) {
                                    CHECK(W >= k.w_lo && W <= k.w_hi, "W outside the corners' range at (%d %d %d)", x, y, z);
                                    const int64_t fx = floor_div(scissors_dot(p.u, x, y, z), W), fy = floor_div(scissors_dot(p.v, x, y, z), W);
                                    const int64_t cx = fx < 0 ? -1 : (fx >= p.width ? p.width : fx), cy = fy < 0 ? -1 : (fy >= p.height ? p.height : fy);
                                    CHECK(cx >= k.px0 && cx <= k.px1 && cy >= k.py0 && cy <= k.py1, "pixel (%lld %lld) outside the corners' rectangle (%d %d) .. (%d %d) at (%d %d %d), case %d",
                                          (long long) cx, (long long) cy, k.px0, k.py0, k.px1, k.py1, x, y, z, t);
                                }
                                const bool m = in_M(p, words, x, y, z);
                                if (verdict == SCISSORS_INSIDE) CHECK(m, "inside, but (%d %d %d) is not in M, case %d", x, y, z, t);
                                if (verdict == SCISSORS_OUTSIDE) CHECK(!m, "outside, but (%d %d %d) is in M, case %d", x, y, z, t);
                            }
                }
    }
    CHECK(verdicts[SCISSORS_INSIDE] > 50 && verdicts[SCISSORS_OUTSIDE] > 50 && verdicts[SCISSORS_PROJECT] > 50 && straddle > 10, "every verdict occurs: %d inside, %d outside, %d projected, %d straddle W = 0",
          verdicts[SCISSORS_INSIDE], verdicts[SCISSORS_OUTSIDE], verdicts[SCISSORS_PROJECT], straddle);
}

static void test_apply()
{
    for (uint32_t vol : {0xffu, 0x1fu, 0x01u, 0u})
        for (uint32_t S = 0; S < 256; ++S)
            for (uint32_t M = 0; M < 256; M += 5) {
                const uint32_t s = S & vol, m = M & vol;
                CHECK(scissors_apply(SCISSORS_ERASE_INSIDE, s, m, vol) == (s & ~m), "erase inside");
                CHECK(scissors_apply(SCISSORS_ERASE_OUTSIDE, s, m, vol) == (s & m), "erase outside");
                CHECK(scissors_apply(SCISSORS_FILL_INSIDE, s, m, vol) == (s | m), "fill inside");
                CHECK(scissors_apply(SCISSORS_FILL_OUTSIDE, s, m, vol) == (s | (vol & ~m)), "fill outside");
            }
}

static void test_polygon()
{
    const int width = 45, height = 20;
    std::vector<uint32_t> words(scissors_mask_words(width, height), 0xdeadbeefu);
    const double square[8] = {3.5, 2.5, 40.5, 2.5, 40.5, 9.5, 3.5, 9.5}; // edges through pixel centres: half-open, a centre on the left or upper edge is inside
    CHECK(scissors_polygon(square, 4, width, height, words.data()), "a square");
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) CHECK(bit_of(words, width, x, y) == (x >= 3 && x < 40 && y >= 2 && y < 9), "square at (%d %d)", x, y);
    CHECK(scissors_mask_stray_row(words.data(), width, height) == -1, "no bit beyond the width");
    const double big[6] = {-100.0, -50.0, 500.0, -50.0, 200.0, 300.0}; // mostly outside the frame
    CHECK(scissors_polygon(big, 3, width, height, words.data()), "a triangle round the frame");
    CHECK(scissors_mask_stray_row(words.data(), width, height) == -1 && bit_of(words, width, 44, 0) && bit_of(words, width, 0, 19), "the frame is covered and nothing beyond it");
    CHECK(!scissors_polygon(big, 2, width, height, words.data()), "two points are no polygon");
    const double bad[6] = {0.0, 0.0, NAN, 1.0, 2.0, 2.0};
    CHECK(!scissors_polygon(bad, 3, width, height, words.data()), "a NaN");
}

int main()
{
    test_quotient();
    test_bounds();
    test_summary();
    test_corners_and_verdict();
    test_apply();
    test_polygon();
    std::printf("failures=%d\n", failures);
    return failures ? 1 : 0;
}
