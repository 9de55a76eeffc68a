// The plan of tbrm_smooth_labels (tbraymarcherplugin_amd/csrc/tbrm_smooth_plan.h) on its own: the reaches, the brick range of the box
// grown by them and clamped to the volume against voxel-by-voxel answers, every refused bound, the radii of a spacing, and the two
// index rules the counting kernel takes from tbrm_brick_boards.h (clipped_extent, row_window) against loops. Pure host code, no
// device; tests/test_smooth_abi.py builds it with -fsanitize=address,undefined and runs it. Prints "failures=N" last.
#include "../../tbraymarcherplugin_amd/csrc/tbrm_smooth_plan.h"

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
    { // the brick ranges: widths 1, 7, 8, 9, 17 at every third origin of a 160-voxel axis; the axes are independent, so one axis varies
      // and the others hold a fixed box
        const int dims[3] = {160, 24, 19};
        const int32_t radii[][3] = {{1, 1, 1}, {2, 1, 0}, {0, 0, 3}, {3, 2, 1}, {7, 8, 9}, {16, 16, 16}, {16, 0, 1}};
        for (const auto& radius : radii)
            for (int iterations : {1, 2, 3, 4, 7, 64})
                for (int width : {1, 7, 8, 9, 17})
                    for (int o = 0; o + width <= dims[0]; o += 3) {
                        const int origin[3] = {o, 5, 3}, end[3] = {o + width, 14, 10};
                        SmoothPlan p;
                        std::memset(&p, 0xff, sizeof(p));
                        const SmoothPlan before = p;
                        const int most = radius[0] > radius[1] ? (radius[0] > radius[2] ? radius[0] : radius[2]) : (radius[1] > radius[2] ? radius[1] : radius[2]);
                        if (iterations * most > kSmoothMaxReach) {
                            CHECK(!smooth_plan(dims, origin, end, radius, iterations, &p) && std::memcmp(&p, &before, sizeof(p)) == 0);
                            continue;
                        }
                        CHECK(smooth_plan(dims, origin, end, radius, iterations, &p));
                        CHECK(p.passes == iterations);
                        for (int c = 0; c < 3; ++c) {
                            CHECK(p.radius[c] == radius[c] && p.reach[c] == iterations * radius[c]);
                            int b0, nb;
                            brick_range_by_counting(dims[c], origin[c], end[c], p.reach[c], b0, nb);
                            CHECK(p.b0[c] == b0 && p.nb[c] == nb);
                            CHECK(p.b0[c] >= 0 && (p.b0[c] + p.nb[c] - 1) * 8 < dims[c]); // every brick holds a voxel of the volume
                            brick_range_by_counting(dims[c], origin[c], end[c], 0, b0, nb);
                            CHECK(p.wb0[c] == b0 && p.wnb[c] == nb);
                            CHECK(p.wb0[c] >= p.b0[c] && p.wb0[c] + p.wnb[c] <= p.b0[c] + p.nb[c]);
                        }
                    }
        const int32_t one[3] = {1, 1, 1}, top[3] = {16, 16, 16};
        const int o[3] = {0, 0, 0}, e[3] = {160, 24, 19};
        SmoothPlan q;
        std::memset(&q, 0x5a, sizeof(q));
        const SmoothPlan before = q;
        const int far[3] = {INT_MAX, INT_MAX, INT_MAX}, big[3] = {INT_MAX, INT_MAX, INT_MAX}, last[3] = {INT_MAX - 1, INT_MAX - 1, INT_MAX - 1};
        CHECK(!smooth_plan(dims, o, e, one, 0, &q) && !smooth_plan(dims, o, e, one, 65, &q) && !smooth_plan(dims, o, e, top, 5, &q));
        CHECK(!smooth_plan(dims, o, far, one, 1, &q) && !smooth_plan(dims, e, e, one, 1, &q));
        CHECK(!smooth_plan(nullptr, o, e, one, 1, &q) && !smooth_plan(dims, o, e, one, 1, nullptr) && !smooth_plan(dims, o, e, nullptr, 1, &q));
        CHECK(!smooth_plan(dims, nullptr, e, one, 1, &q) && !smooth_plan(dims, o, nullptr, one, 1, &q));
        CHECK(std::memcmp(&q, &before, sizeof(q)) == 0);
        CHECK(smooth_plan(big, last, far, top, 4, &q) && q.reach[0] == 64); // the largest coordinates: no overflow on the way
        CHECK(q.b0[0] == (INT_MAX - 1 - 64) >> 3 && q.b0[0] + q.nb[0] - 1 == (INT_MAX - 1) >> 3);
    }

    { // every refused bound, and the bounds themselves
        int axis = -7;
        const int32_t one[3] = {1, 1, 1}, top[3] = {16, 16, 16}, none[3] = {0, 0, 0}, over[3] = {1, 17, 1}, under[3] = {1, 1, -1}, flat[3] = {0, 2, 0};
        CHECK(smooth_arguments(one, 1, 2, 1, &axis) == SMOOTH_OK && axis == -7);
        CHECK(smooth_arguments(top, 255, 256, 4, &axis) == SMOOTH_OK && smooth_arguments(one, 0, 1, 64, &axis) == SMOOTH_OK);
        CHECK(smooth_arguments(flat, 0, 256, 32, &axis) == SMOOTH_OK && axis == -7);
        CHECK(smooth_arguments(over, 1, 2, 1, &axis) == SMOOTH_RADIUS && axis == 1);
        CHECK(smooth_arguments(under, 1, 2, 1, &axis) == SMOOTH_RADIUS && axis == 2);
        CHECK(smooth_arguments(none, 1, 2, 1, &axis) == SMOOTH_NO_RADIUS);
        CHECK(smooth_arguments(one, 1, 2, 0, &axis) == SMOOTH_ITERATIONS && smooth_arguments(one, 1, 2, 65, &axis) == SMOOTH_ITERATIONS);
        CHECK(smooth_arguments(one, 1, 2, INT_MIN, &axis) == SMOOTH_ITERATIONS && smooth_arguments(one, 1, 2, INT_MAX, &axis) == SMOOTH_ITERATIONS);
        CHECK(smooth_arguments(top, 1, 2, 5, &axis) == SMOOTH_REACH && axis == 0);
        CHECK(smooth_arguments(flat, 1, 2, 33, &axis) == SMOOTH_REACH && axis == 1);
        CHECK(smooth_arguments(one, 1, 0, 1, nullptr) == SMOOTH_RANK_DEN && smooth_arguments(one, 1, 257, 1, nullptr) == SMOOTH_RANK_DEN);
        CHECK(smooth_arguments(one, 0, INT_MIN, 1, nullptr) == SMOOTH_RANK_DEN);
        CHECK(smooth_arguments(one, 2, 2, 1, nullptr) == SMOOTH_RANK_NUM && smooth_arguments(one, -1, 2, 1, nullptr) == SMOOTH_RANK_NUM);
        CHECK(smooth_arguments(one, 256, 256, 1, nullptr) == SMOOTH_RANK_NUM && smooth_arguments(one, INT_MAX, 256, 1, nullptr) == SMOOTH_RANK_NUM);
        // under the bounds every product the kernel forms fits 32 bits
        CHECK((int64_t) 33 * 33 * 33 * kSmoothMaxRankDen < INT32_MAX && 33 * 33 <= 65535 && 33 * 33 * 33 <= 65535);
    }

    { // the radii of a spacing: r_a = floor(radius / spacing_a + 0.5)
        int32_t r[3] = {-7, -7, -7};
        const double iso[3] = {1, 1, 1}, ct[3] = {0.7, 0.7, 2.5}, yx[3] = {1.0, 2.0, 4.0};
        CHECK(smooth_radii(iso, 2.0, r) && r[0] == 2 && r[1] == 2 && r[2] == 2);
        CHECK(smooth_radii(ct, 2.0, r) && r[0] == 3 && r[1] == 3 && r[2] == 1);
        CHECK(smooth_radii(yx, 1.0, r) && r[0] == 1 && r[1] == 1 && r[2] == 0);
        CHECK(smooth_radii(iso, 16.4, r) && r[0] == 16 && smooth_radii(iso, 0.5, r) && r[0] == 1);
        const double spacings[] = {1e-9, 1e-3, 0.5, 0.7, 1.0, 2.5, 40.0, 1e6, 1e12};
        const double radii[] = {1e-9, 0.01, 0.5, 0.7, 1.0, 5.0, 16.0, 16.5, 100.0, 1e9, 1e300};
        for (double sx : spacings)
            for (double sz : spacings)
                for (double radius : radii) {
                    const double sp[3] = {sx, 1.0, sz};
                    int32_t rr[3] = {9, 9, 9};
                    if (smooth_radii(sp, radius, rr)) {
                        CHECK(smooth_arguments(rr, 1, 2, 1, nullptr) == SMOOTH_OK);
                        for (int c = 0; c < 3; ++c) CHECK(rr[c] == (int32_t) std::floor(radius / sp[c] + 0.5));
                    } else
                        CHECK(rr[0] == 9 && rr[1] == 9 && rr[2] == 9); // a refusal leaves the outputs alone
                }
        const double nan = std::nan(""), inf = INFINITY;
        const double bad[][4] = {{0, 1, 1, 1}, {1, -1, 1, 1}, {1, 1, nan, 1}, {1, 1, inf, 1}, {1, 1, 1, 0}, {1, 1, 1, -2}, {1, 1, 1, nan}, {1, 1, 1, inf},
                                 {1, 1, 1, 16.5}, {1, 1, 0.1, 2}, {1, 1, 1, 0.4}, {1e-300, 1, 1, 1}};
        for (const auto& b : bad) CHECK(!smooth_radii(b, b[3], r));
        CHECK(!smooth_radii(nullptr, 1.0, r) && !smooth_radii(iso, 1.0, nullptr));
    }

    { // tbrm_brick_boards.h: the window clipped to an axis, and the x window of a row word, against loops
        for (int dim : {1, 2, 7, 8, 9, 17, 40})
            for (int r = 0; r <= 16; ++r)
                for (int v = -3; v < dim + 3; ++v) {
                    int n = 0;
                    if (v >= 0 && v < dim)
                        for (int u = v - r; u <= v + r; ++u) n += u >= 0 && u < dim;
                    CHECK(clipped_extent(dim, v, r) == n);
                }
        CHECK(clipped_extent(INT_MAX, INT_MAX - 1, 16) == 17 && clipped_extent(INT_MAX, 0, 16) == 17 && clipped_extent(INT_MAX, 1000, 16) == 33);
        for (int r = 0; r <= 16; ++r)
            for (int i = 0; i < 8; ++i) {
                uint64_t want = 0;
                for (int x = i - r; x <= i + r; ++x) want |= 1ull << (kRowWordShift + x); // bit p: the voxel x = p - 16 of the brick's row
                CHECK(row_window(i, r) == want);
                CHECK((row_window(i, r) >> 40) == 0);                                     // five bricks' bytes hold every window
            }
    }
    std::printf("failures=%d\n", failures);
    return failures != 0;
}
