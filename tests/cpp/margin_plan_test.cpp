// The plan of tbrm_margin_labels (tbraymarcherplugin_amd/csrc/tbrm_margin_plan.h) on its own: the reaches against a loop, the brick
// range of the box grown by them and clamped to the volume against voxel-by-voxel answers, the transforms of the four operators and
// the bounds of the weights' quantisation. Pure host code, no device; tests/test_margin_abi.py builds it with
// -fsanitize=address,undefined and runs it. Prints "failures=N" last.
#include "../../tbraymarcherplugin_amd/csrc/tbrm_margin_plan.h"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace tbrm;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
        }                                                                  \
    } while (0)

// the largest n with w n^2 <= limit, by counting up
static int reach_by_loop(uint32_t w, uint32_t limit)
{
    uint64_t n = 0;
    while ((uint64_t) w * (n + 1) * (n + 1) <= (uint64_t) limit) ++n;
    return (int) n;
}

// the brick range by counting: the bricks that hold a voxel within `reach` of the box along this axis, inside the volume
static void brick_range_by_counting(int dim, int o, int e, int reach, int& b0, int& nb)
{
    int first = INT_MAX, last = -1;
    for (int v = 0; v < dim; ++v)
        if (v >= o - reach && v < e + reach) {
            if (v / 8 < first) first = v / 8;
            last = v / 8;
        }
    b0 = first;
    nb = last - first + 1;
}

int main()
{
    { // the reaches
        const uint32_t ws[] = {1u, 2u, 3u, 255u, 256u, 257u, 400u, 1600u, 3265u, 4096u, 65535u, 1u << 20, 0x7fffffffu, 0xffffffffu};
        const uint32_t limits[] = {1u, 2u, 3u, 4u, 8u, 9u, 255u, 256u, 257u, 1023u, 1024u, 4095u, 4096u, 4097u, 13061u, 65535u, 65536u, 1048576u, 0x7ffffffeu, 0x7fffffffu};
        for (uint32_t w : ws)
            for (uint32_t l : limits) CHECK(margin_reach(w, l) == reach_by_loop(w, l));
        for (uint32_t n = 0; n <= 65535; n += 257) { // perfect squares and their neighbours
            CHECK(margin_reach(1, n * n) == (int) n);
            if (n > 0) CHECK(margin_reach(1, n * n - 1) == (int) n - 1);
        }
        CHECK(margin_reach(1, 0xffffffffu) == 65535);
        int n[3] = {-7, -7, -7};
        const uint32_t iso[3] = {1, 1, 1}, aniso[3] = {256, 400, 1600}, zero[3] = {1, 0, 1}, lop[3] = {1, 4096, 4096};
        CHECK(margin_reaches(iso, 4096, n) && n[0] == 64 && n[1] == 64 && n[2] == 64);
        CHECK(margin_reaches(aniso, 256 * 9, n) && n[0] == 3 && n[1] == 2 && n[2] == 1);
        CHECK(margin_reaches(lop, 4096, n) && n[0] == 64 && n[1] == 1 && n[2] == 1);
        CHECK(margin_reaches(lop, 4095, n) && n[0] == 63 && n[1] == 0 && n[2] == 0);
        n[0] = n[1] = n[2] = -7;
        CHECK(!margin_reaches(iso, 4225, n));        // a reach of 65
        CHECK(!margin_reaches(iso, 0, n));
        CHECK(!margin_reaches(iso, 0x80000000u, n));
        CHECK(!margin_reaches(zero, 4, n));
        CHECK(!margin_reaches(aniso, 255, n));       // every reach 0
        CHECK(!margin_reaches(nullptr, 4, n) && !margin_reaches(iso, 4, nullptr));
        CHECK(n[0] == -7 && n[1] == -7 && n[2] == -7); // a refusal leaves the reaches alone
        const uint32_t top[3] = {0x7fffffffu, 0x7fffffffu, 1u << 19};
        CHECK(margin_reaches(top, 0x7fffffffu, n) && n[0] == 1 && n[1] == 1 && n[2] == 63);
    }

    { // the brick ranges: widths 1, 7, 8, 9, 17 and 137 at every origin of a 160-voxel axis would be slow voxel by voxel for all three
      // axes at once: the axes are independent, so one axis varies and the others hold a fixed box
        const int dims[3] = {160, 24, 19};
        const uint32_t weight_sets[][3] = {{1, 1, 1}, {1, 4096, 4096}, {256, 400, 1600}};
        const uint32_t limit_sets[][5] = {{1, 9, 64, 289, 4096}, {64, 81, 289, 3969, 4096}, {256, 2304, 6400, 65536, 1048576}};
        for (int s = 0; s < 3; ++s)
            for (uint32_t limit : limit_sets[s])
                for (int width : {1, 7, 8, 9, 17, 137})
                    for (int o = 0; o + width <= dims[0]; o += (width == 137 ? 1 : 3))
                        for (int op = MARGIN_EXPAND; op <= MARGIN_CLOSE; ++op) {
                            const int origin[3] = {o, 5, 3}, end[3] = {o + width, 14, 10};
                            MarginPlan p;
                            std::memset(&p, 0xff, sizeof(p));
                            CHECK(margin_plan(dims, origin, end, op, weight_sets[s], limit, &p));
                            const bool two = op == MARGIN_OPEN || op == MARGIN_CLOSE;
                            CHECK(p.transforms == (two ? 2 : 1));
                            CHECK(p.shrink[0] == (op == MARGIN_SHRINK || op == MARGIN_OPEN));
                            CHECK(p.shrink[1] == (op == MARGIN_CLOSE));
                            for (int c = 0; c < 3; ++c) {
                                CHECK(p.reach[c] == reach_by_loop(weight_sets[s][c], limit));
                                CHECK(p.total[c] == p.transforms * p.reach[c]);
                                int b0, nb;
                                brick_range_by_counting(dims[c], origin[c], end[c], p.total[c], b0, nb);
                                CHECK(p.b0[c] == b0 && p.nb[c] == nb);
                                CHECK(p.b0[c] >= 0 && (p.b0[c] + p.nb[c] - 1) * 8 < dims[c]); // every brick holds a voxel of the volume
                                brick_range_by_counting(dims[c], origin[c], end[c], 0, b0, nb);
                                CHECK(p.wb0[c] == b0 && p.wnb[c] == nb);
                                CHECK(p.wb0[c] >= p.b0[c] && p.wb0[c] + p.wnb[c] <= p.b0[c] + p.nb[c]);
                            }
                        }
        const uint32_t iso[3] = {1, 1, 1};
        const int o[3] = {0, 0, 0}, e[3] = {160, 24, 19};
        MarginPlan q;
        std::memset(&q, 0x5a, sizeof(q));
        const MarginPlan before = q;
        const int far[3] = {INT_MAX, INT_MAX, INT_MAX}, big[3] = {INT_MAX, INT_MAX, INT_MAX}, last[3] = {INT_MAX - 1, INT_MAX - 1, INT_MAX - 1};
        CHECK(!margin_plan(dims, o, e, 4, iso, 4, &q) && !margin_plan(dims, o, e, -1, iso, 4, &q));
        CHECK(!margin_plan(dims, o, e, MARGIN_OPEN, iso, 0, &q) && !margin_plan(dims, o, e, MARGIN_OPEN, iso, 4225, &q));
        CHECK(!margin_plan(dims, o, far, MARGIN_OPEN, iso, 4, &q) && !margin_plan(dims, e, e, MARGIN_OPEN, iso, 4, &q));
        CHECK(!margin_plan(nullptr, o, e, MARGIN_OPEN, iso, 4, &q) && !margin_plan(dims, o, e, MARGIN_OPEN, iso, 4, nullptr));
        CHECK(!margin_plan(dims, o, e, MARGIN_OPEN, nullptr, 4, &q));
        CHECK(std::memcmp(&q, &before, sizeof(q)) == 0);
        CHECK(margin_plan(big, last, far, MARGIN_CLOSE, iso, 4096, &q) && q.total[0] == 128); // the largest coordinates: no overflow on the way
        CHECK(q.b0[0] == (INT_MAX - 1 - 128) >> 3 && q.b0[0] + q.nb[0] - 1 == (INT_MAX - 1) >> 3);
    }

    { // the quantisation
        uint32_t w[3] = {7, 7, 7}, limit = 7;
        const double iso[3] = {0.7, 0.7, 0.7}, ct[3] = {0.7, 0.7, 2.5}, yx[3] = {2.0, 1.0, 4.0};
        CHECK(margin_weights(iso, 0.7 * 3.0, w, &limit) && w[0] == 256 && w[1] == 256 && w[2] == 256);
        CHECK(limit == (uint32_t) std::floor((0.7 * 3.0 / 0.7) * (0.7 * 3.0 / 0.7) * 256.0));
        CHECK(margin_weights(ct, 5.0, w, &limit) && w[0] == 256 && w[1] == 256 && w[2] == 3265 && limit == 13061);
        CHECK(margin_weights(yx, 3.0, w, &limit) && w[0] == 1024 && w[1] == 256 && w[2] == 4096 && limit == 2304);
        // a weight is off by at most half a unit: 1 part in 512 of a squared ratio >= 1
        for (double ratio = 1.0; ratio < 40.0; ratio += 0.0137) {
            const double sp[3] = {1.0, ratio, 1.0};
            CHECK(margin_weights(sp, 2.0, w, &limit));
            const double exact = ratio * ratio * 256.0;
            CHECK(std::fabs((double) w[1] - exact) <= 0.5 && std::fabs((double) w[1] - exact) / exact <= 1.0 / 512.0);
            CHECK(limit == 1024 && w[0] == 256 && w[2] == 256);
        }
        // the bounds: what comes out always passes margin_reaches, whatever goes in
        const double spacings[] = {1e-9, 1e-3, 0.5, 0.7, 1.0, 2.5, 40.0, 1e6, 1e12};
        const double radii[] = {1e-9, 0.01, 0.5, 0.7, 1.0, 5.0, 44.0, 45.5, 64.0, 64.01, 100.0, 3000.0, 1e9};
        for (double sx : spacings)
            for (double sz : spacings)
                for (double r : radii) {
                    const double sp[3] = {sx, 1.0, sz};
                    uint32_t ww[3] = {9, 9, 9}, ll = 9;
                    int n[3];
                    if (margin_weights(sp, r, ww, &ll)) {
                        CHECK(margin_reaches(ww, ll, n));
                        CHECK(ll >= 1 && ll < 0x80000000u && ww[0] >= 256 && ww[1] >= 256 && ww[2] >= 256);
                        CHECK(ww[0] == 256 || ww[1] == 256 || ww[2] == 256);
                    } else
                        CHECK(ww[0] == 9 && ww[1] == 9 && ww[2] == 9 && ll == 9); // a refusal leaves the outputs alone
                }
        const double nan = std::nan(""), inf = INFINITY;
        const double bad[][4] = {{0, 1, 1, 1}, {1, -1, 1, 1}, {1, 1, nan, 1}, {1, 1, inf, 1}, {1, 1, 1, 0}, {1, 1, 1, -2}, {1, 1, 1, nan}, {1, 1, 1, inf},
                                 {1, 1, 1, 65}, {1, 1, 1, 0.05}, {1, 1, 1, 0.7}, {1e-3, 1, 1, 3000}, {1, 1e6, 1, 1}};
        for (const auto& b : bad) CHECK(!margin_weights(b, b[3], w, &limit));
        CHECK(!margin_weights(nullptr, 1.0, w, &limit) && !margin_weights(iso, 1.0, nullptr, &limit) && !margin_weights(iso, 1.0, w, nullptr));
        const double one[3] = {1, 1, 1};
        CHECK(margin_weights(one, 64.0, w, &limit) && limit == 256u * 4096u);
    }
    std::printf("failures=%d\n", failures);
    return failures != 0;
}
