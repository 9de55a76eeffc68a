// paint_plan_test.cpp — the host-compilable rules of the paint brush (tbrm_paint_plan.h) against loops: the distance
// rule against an exact comparison in 128-bit integers, the row form against the voxel form, the corner verdict against every voxel,
// the reaches at the bounds, the argument checks, the segments' and runs' boxes, the work box and the stroke helper. Stand-alone: no
// device, no library. tests/test_paint_abi.py builds it with -fsanitize=address,undefined and runs it.
#include "../../tbraymarcherplugin_amd/csrc/tbrm_paint_plan.h"

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

static std::mt19937_64 rng(20261021);
static int64_t uniform(int64_t lo, int64_t hi) { return std::uniform_int_distribution<int64_t>(lo, hi)(rng); }

typedef __int128 wide;

// The definition with no early rejection, in 128 bits: the squared distance to the nearest point a + t d, t = de / dd clamped to
// [0, 1], compared with limit after multiplying through by dd.
static bool within_exactly(const int32_t a[3], const int32_t d[3], const int32_t w[3], int64_t limit, int x, int y, int z)
{
    const int64_t e[3] = {8ll * x - a[0], 8ll * y - a[1], 8ll * z - a[2]};
    wide dd = 0, de = 0, ee = 0;
    for (int c = 0; c < 3; ++c) {
        dd += (wide) w[c] * d[c] * d[c];
        de += (wide) w[c] * d[c] * e[c];
        ee += (wide) w[c] * e[c] * e[c];
    }
    if (de <= 0) return ee <= limit;
    if (de >= dd) return ee - 2 * de + dd <= limit;
    return ee * dd - de * de <= (wide) limit * dd;
}

static PaintSegment segment(const int32_t a[3], const int32_t b[3], const int32_t w[3], const int reach[3])
{
    PaintSegment g{};
    for (int c = 0; c < 3; ++c) {
        g.a[c] = a[c];
        g.d[c] = b[c] - a[c];
        g.lo[c] = paint_ceil8(std::min(a[c], b[c]) - reach[c]);
        g.hi[c] = paint_floor8(std::max(a[c], b[c]) + reach[c]);
    }
    g.dd = (int32_t) paint_dot(w, g.d, g.d);
    return g;
}

static void test_rounding()
{
    for (int v = -100; v <= 100; ++v) {
        int f = v / 8;
        if (v % 8 != 0 && v < 0) --f;
        CHECK(paint_floor8(v) == f, "floor8 %d", v);
        CHECK(paint_ceil8(v) == (v % 8 == 0 ? f : f + 1), "ceil8 %d", v);
    }
    for (uint32_t v : {0u, 1u, 2u, 3u, 4u, 15u, 16u, 17u, 262143u, 262144u, 262145u, 0x3FFFFFFFu, 0xFFFFFFFFu, 0xFFFE0001u, 0xFFFE0000u}) {
        const uint64_t n = paint_isqrt(v);
        CHECK(n * n <= v && (n + 1) * (n + 1) > v, "isqrt %u", v);
    }
    for (int t = 0; t < 200000; ++t) {
        const uint32_t v = (uint32_t) uniform(0, 0xFFFFFFFFll);
        const uint64_t n = paint_isqrt(v);
        CHECK(n * n <= v && (n + 1) * (n + 1) > v, "isqrt %u", v);
    }
    // the reach: w n^2 <= limit < w (n + 1)^2, also at the bounds
    for (uint32_t w : {1u, 2u, 255u, 256u, 65535u})
        for (uint32_t limit : {1u, 63u, 64u, 65u, 262143u, 262144u, kPaintMaxLimit}) {
            const uint64_t n = (uint64_t) paint_reach8(limit, w);
            CHECK(w * n * n <= limit && w * (n + 1) * (n + 1) > limit, "reach8 %u %u", limit, w);
        }
    CHECK(paint_reach_voxels(0) == 0 && paint_reach_voxels(1) == 1 && paint_reach_voxels(8) == 1 && paint_reach_voxels(9) == 2 && paint_reach_voxels(512) == 64 && paint_reach_voxels(513) == 65, "reach in voxels");
}

// the rule against the exact comparison: random segments near a small volume, and the extremes the bounds allow
static void test_rule()
{
    for (int t = 0; t < 3000; ++t) {
        const int32_t w[3] = {(int32_t) uniform(1, t % 4 == 0 ? kPaintMaxWeight : 300), (int32_t) uniform(1, 300), (int32_t) uniform(1, t % 5 == 0 ? kPaintMaxWeight : 300)};
        const int dims[3] = {(int) uniform(1, 20), (int) uniform(1, 12), (int) uniform(1, 12)};
        int32_t a[3], b[3];
        for (int c = 0; c < 3; ++c) a[c] = (int32_t) uniform(-40, 8 * dims[c] + 40);
        // a second point whose dd stays below 2^30
        for (;;) {
            const int span = t % 3 == 0 ? 4 : 200;
            for (int c = 0; c < 3; ++c) b[c] = a[c] + (int32_t) uniform(-span, span);
            const int32_t d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
            if (paint_dot(w, d, d) < (1ll << 30)) break;
        }
        if (t % 11 == 0) for (int c = 0; c < 3; ++c) b[c] = a[c]; // a ball
        const int64_t limit = t % 7 == 0 ? (int64_t) kPaintMaxLimit : uniform(1, 1ll << uniform(1, 29));
        const int reach[3] = {0, 0, 0};
        const PaintSegment g = segment(a, b, w, reach);
        for (int z = 0; z < dims[2]; ++z)
            for (int y = 0; y < dims[1]; ++y)
                for (int x0 = 0; x0 < dims[0]; x0 += 8) {
                    const uint32_t row = paint_row_within(g, w, limit, x0, y, z);
                    for (int i = 0; i < 8; ++i) {
                        const bool want = within_exactly(g.a, g.d, w, limit, x0 + i, y, z);
                        CHECK(paint_voxel_within(g, w, limit, x0 + i, y, z) == want, "voxel (%d, %d, %d) of case %d", x0 + i, y, z, t);
                        CHECK((bool) ((row >> i) & 1u) == want, "row bit %d at (%d, %d, %d) of case %d", i, x0, y, z, t);
                    }
                }
    }
    // the coordinate bounds: a point and voxels at opposite ends, the largest weights — ee < 2^56 is formed and rejected
    {
        const int32_t w[3] = {kPaintMaxWeight, kPaintMaxWeight, kPaintMaxWeight};
        const int32_t a[3] = {-kPaintMaxCoord, -kPaintMaxCoord, -kPaintMaxCoord}, b[3] = {-kPaintMaxCoord + 70, -kPaintMaxCoord - 70, -kPaintMaxCoord + 70};
        const int reach[3] = {0, 0, 0};
        const PaintSegment g = segment(a, b, w, reach);
        CHECK(g.dd > 0 && (int64_t) g.dd < (1ll << 30), "dd");
        for (int v : {0, 1, kPaintMaxDim - 1, kPaintMaxDim + 6}) {
            CHECK(!paint_voxel_within(g, w, kPaintMaxLimit, v, v, v), "far voxel");
            CHECK(paint_row_within(g, w, kPaintMaxLimit, v & ~7, v, v) == 0u, "far row");
        }
        const int32_t a2[3] = {kPaintMaxCoord, kPaintMaxCoord, kPaintMaxCoord};
        const PaintSegment g2 = segment(a2, a2, w, reach);
        CHECK(!paint_voxel_within(g2, w, kPaintMaxLimit, 0, 0, 0), "far voxel");
    }
    // the products at their largest: the longest segment, the largest limit, voxels just inside the early rejection
    {
        const int32_t w[3] = {kPaintMaxWeight, kPaintMaxWeight, kPaintMaxWeight};
        const int32_t a[3] = {-120, -120, -120}, b[3] = {-47, -47, -47};
        const int reach[3] = {0, 0, 0};
        const PaintSegment g = segment(a, b, w, reach);
        int64_t ee, de;
        paint_products(g, w, 3, 3, 3, ee, de);
        CHECK(ee <= 2 * ((int64_t) g.dd + kPaintMaxLimit) && ee > (3ll << 30), "the case is past the rejection with ee near 2^32");
        for (int z = 0; z < 8; ++z)
            for (int y = 0; y < 8; ++y)
                for (int x = 0; x < 8; ++x) CHECK(paint_voxel_within(g, w, kPaintMaxLimit, x, y, z) == within_exactly(g.a, g.d, w, kPaintMaxLimit, x, y, z), "extreme (%d, %d, %d)", x, y, z);
    }
    // the tie: a voxel at exactly the limit is in, one unit less and it is out
    {
        const int32_t w[3] = {1, 1, 1}, a[3] = {48, 64, 64}, b[3] = {128, 64, 64};
        const int reach[3] = {24, 24, 24};
        const PaintSegment g = segment(a, b, w, reach);
        CHECK(paint_voxel_within(g, w, 576, 10, 11, 8) && !paint_voxel_within(g, w, 575, 10, 11, 8), "beside the inside");
        CHECK(paint_voxel_within(g, w, 576, 3, 8, 8) && !paint_voxel_within(g, w, 575, 3, 8, 8), "before a");
        CHECK(paint_voxel_within(g, w, 576, 19, 8, 8) && !paint_voxel_within(g, w, 575, 19, 8, 8), "behind b");
    }
}

// a brick whose corners are within one segment is within it entirely; and the verdict is not vacuous
static void test_corners()
{
    int whole = 0;
    for (int t = 0; t < 4000; ++t) {
        const int32_t w[3] = {(int32_t) uniform(1, 6), (int32_t) uniform(1, 6), (int32_t) uniform(1, 6)};
        int32_t a[3], b[3];
        for (int c = 0; c < 3; ++c) { a[c] = (int32_t) uniform(-100, 300); b[c] = a[c] + (int32_t) uniform(-150, 150); }
        const int64_t limit = uniform(200, 60000);
        const int reach[3] = {paint_reach8((uint32_t) limit, (uint32_t) w[0]), paint_reach8((uint32_t) limit, (uint32_t) w[1]), paint_reach8((uint32_t) limit, (uint32_t) w[2])};
        const PaintSegment g = segment(a, b, w, reach);
        const int dims[3] = {(int) uniform(9, 30), (int) uniform(9, 30), (int) uniform(9, 30)};
        const int bx = (int) uniform(0, (dims[0] - 1) / 8), by = (int) uniform(0, (dims[1] - 1) / 8), bz = (int) uniform(0, (dims[2] - 1) / 8);
        const int32_t blo[3] = {bx * 8, by * 8, bz * 8}, bhi[3] = {paint_corner(dims[0], bx, 1), paint_corner(dims[1], by, 1), paint_corner(dims[2], bz, 1)};
        CHECK(bhi[0] < dims[0] && bhi[0] >= blo[0] && bhi[0] - blo[0] <= 7 && paint_corner(dims[0], bx, 0) == blo[0], "corner");
        const bool verdict = paint_corners_within(g, w, limit, blo, bhi), meets = paint_boxes_meet(g.lo, g.hi, blo, bhi);
        bool all = true, any = false;
        for (int z = blo[2]; z <= bhi[2]; ++z)
            for (int y = blo[1]; y <= bhi[1]; ++y)
                for (int x = blo[0]; x <= bhi[0]; ++x) {
                    const bool in = paint_voxel_within(g, w, limit, x, y, z);
                    all = all && in;
                    any = any || in;
                }
        CHECK(verdict == all, "case %d: corners say %d, the voxels %d", t, (int) verdict, (int) all);
        CHECK(meets || !any, "case %d: a voxel within a segment whose grown box misses the brick", t);
        whole += verdict;
    }
    CHECK(whole > 50, "only %d whole bricks", whole);
}

static void test_arguments()
{
    const int dims[3] = {40, 27, 19};
    const uint32_t w[3] = {1, 1, 1};
    const int32_t pts[9] = {0, 0, 0, 100, 50, 20, -30, 400, 7};
    CHECK(paint_arguments(dims, PAINT_PAINT, 0, w, 576, pts, 3).what == PAINT_OK, "a good call");
    CHECK(paint_arguments(dims, PAINT_ERASE, 1, w, kPaintMaxLimit / 4096, pts, 1).what == PAINT_OK, "a good call");
    const int big[3] = {40, kPaintMaxDim + 1, 19}, edge[3] = {kPaintMaxDim, 1, 1};
    PaintVerdict v = paint_arguments(big, 0, 0, w, 576, pts, 3);
    CHECK(v.what == PAINT_DIMS && v.axis == 1, "dims");
    CHECK(paint_arguments(edge, 0, 0, w, 576, pts, 3).what == PAINT_OK, "dims at the bound");
    CHECK(paint_arguments(dims, 0, 0, w, 576, pts, 0).what == PAINT_N_POINTS, "no point");
    std::vector<int32_t> many(3 * (kPaintMaxPoints + 1), 5);
    CHECK(paint_arguments(dims, 0, 0, w, 576, many.data(), kPaintMaxPoints + 1).what == PAINT_N_POINTS, "too many points");
    CHECK(paint_arguments(dims, 0, 0, w, 576, many.data(), kPaintMaxPoints).what == PAINT_OK, "points at the bound");
    CHECK(paint_arguments(dims, 2, 0, w, 576, pts, 3).what == PAINT_OP && paint_arguments(dims, -1, 0, w, 576, pts, 3).what == PAINT_OP, "op");
    CHECK(paint_arguments(dims, 0, 2, w, 576, pts, 3).what == PAINT_GATE, "gate");
    const uint32_t w0[3] = {1, 0, 1}, wbig[3] = {1, 1, 65536}, wtop[3] = {65535, 65535, 65535};
    v = paint_arguments(dims, 0, 0, w0, 576, pts, 3);
    CHECK(v.what == PAINT_WEIGHT && v.axis == 1, "weight 0");
    v = paint_arguments(dims, 0, 0, wbig, 576, pts, 3);
    CHECK(v.what == PAINT_WEIGHT && v.axis == 2, "weight 65536");
    CHECK(paint_arguments(dims, 0, 0, w, 0, pts, 3).what == PAINT_LIMIT && paint_arguments(dims, 0, 0, wtop, kPaintMaxLimit + 1u, pts, 1).what == PAINT_LIMIT, "limit");
    CHECK(paint_arguments(dims, 0, 0, wtop, kPaintMaxLimit, pts, 1).what == PAINT_OK, "limit at the bound");
    // the reach: 512 eighths = 64 voxels is the last one in
    CHECK(paint_arguments(dims, 0, 0, w, 513 * 513 - 1, pts, 1).what == PAINT_OK && paint_arguments(dims, 0, 0, w, 513 * 513, pts, 1).what == PAINT_REACH, "reach");
    const uint32_t w4[3] = {4, 4, 1};
    v = paint_arguments(dims, 0, 0, w4, 4 * 512 * 512, pts, 1);
    CHECK(v.what == PAINT_REACH && v.axis == 2, "the reach of the lightest axis");
    int32_t far[6] = {0, 0, 0, 0, kPaintMaxCoord, -kPaintMaxCoord};
    CHECK(paint_arguments(dims, 0, 0, w, 576, far + 3, 1).what == PAINT_OK, "coordinates at the bound");
    far[5] = -kPaintMaxCoord - 1;
    v = paint_arguments(dims, 0, 0, w, 576, far, 2);
    CHECK(v.what == PAINT_COORD && v.index == 1 && v.axis == 2, "a coordinate beyond");
    const int32_t longish[9] = {0, 0, 0, 10, 10, 10, 10 + 32768, 10, 10};
    v = paint_arguments(dims, 0, 0, w, 576, longish, 3);
    CHECK(v.what == PAINT_SEGMENT && v.index == 1, "a segment with dd = 2^30");
    const int32_t just[6] = {0, 0, 0, 32767, 0, 0};
    CHECK(paint_arguments(dims, 0, 0, w, 576, just, 2).what == PAINT_OK, "a segment with dd = 2^30 - 65535");
}

// the boxes of segments and runs hold every voxel within them; the work box is the box cut to the stroke's; runs are 64 segments
static void test_plan()
{
    for (int t = 0; t < 60; ++t) {
        const int dims[3] = {(int) uniform(1, 40), (int) uniform(1, 30), (int) uniform(1, 20)};
        const uint32_t w[3] = {(uint32_t) uniform(1, 5), (uint32_t) uniform(1, 5), (uint32_t) uniform(1, 5)};
        const int32_t wi[3] = {(int32_t) w[0], (int32_t) w[1], (int32_t) w[2]};
        const uint32_t limit = (uint32_t) uniform(1, 3000);
        const size_t n = t % 6 == 0 ? 1 : (size_t) uniform(2, t % 5 == 0 ? 200 : 6);
        std::vector<int32_t> pts(3 * n);
        for (size_t k = 0; k < n; ++k)
            for (int c = 0; c < 3; ++c) pts[3 * k + c] = k == 0 || t % 5 != 0 ? (int32_t) uniform(-60, 8 * dims[c] + 60) : pts[3 * (k - 1) + c] + (int32_t) uniform(-9, 9);
        VoxelBox box{};
        for (int c = 0; c < 3; ++c) {
            box.origin[c] = t % 2 ? (int) uniform(0, dims[c] - 1) : 0;
            box.end[c] = t % 2 ? (int) uniform(box.origin[c] + 1, dims[c]) : dims[c];
        }
        PaintPlan plan;
        paint_plan(box, w, limit, pts.data(), n, plan);
        CHECK((int) plan.segs.size() == paint_segments(n) && plan.runs.size() == (plan.segs.size() + kPaintRun - 1) / kPaintRun, "counts of case %d", t);
        int covered = 0;
        for (size_t r = 0; r < plan.runs.size(); ++r) {
            const PaintRun& run = plan.runs[r];
            CHECK(run.first == covered && run.count >= 1 && run.count <= kPaintRun && (r + 1 == plan.runs.size() || run.count == kPaintRun), "run %zu of case %d", r, t);
            for (int j = 0; j < run.count; ++j) {
                const PaintSegment& g = plan.segs[(size_t) (run.first + j)];
                CHECK(paint_boxes_meet(g.lo, g.hi, run.lo, run.hi), "segment outside its run");
                for (int c = 0; c < 3; ++c) CHECK(run.lo[c] <= g.lo[c] && run.hi[c] >= g.hi[c] && plan.lo[c] <= run.lo[c] && plan.hi[c] >= run.hi[c], "nesting");
            }
            covered += run.count;
        }
        CHECK(covered == (int) plan.segs.size(), "the runs cover the stroke");
        // every voxel of the volume within a segment lies in its box, and inside the box it lies in the work box
        bool any_in_box = false;
        for (const PaintSegment& g : plan.segs) {
            const int32_t* b = n > 1 ? &pts[3 * (size_t) (&g - plan.segs.data()) + 3] : g.a;
            for (int c = 0; c < 3; ++c) CHECK(g.d[c] == b[c] - g.a[c], "d");
            CHECK((int64_t) g.dd == paint_dot(wi, g.d, g.d), "dd");
            for (int z = 0; z < dims[2]; ++z)
                for (int y = 0; y < dims[1]; ++y)
                    for (int x = 0; x < dims[0]; ++x) {
                        if (!paint_voxel_within(g, wi, limit, x, y, z)) continue;
                        const int32_t v[3] = {x, y, z};
                        CHECK(paint_boxes_meet(g.lo, g.hi, v, v), "a voxel within a segment outside its box (case %d)", t);
                        const bool in_box = x >= box.origin[0] && x < box.end[0] && y >= box.origin[1] && y < box.end[1] && z >= box.origin[2] && z < box.end[2];
                        if (!in_box) continue;
                        any_in_box = true;
                        CHECK(!plan.empty && x >= plan.work.origin[0] && x < plan.work.end[0] && y >= plan.work.origin[1] && y < plan.work.end[1] && z >= plan.work.origin[2] &&
                              z < plan.work.end[2], "a stamped voxel of the box outside the work box (case %d)", t);
                    }
        }
        if (plan.empty) {
            CHECK(!any_in_box && range_bricks(plan.range) == 0, "an empty plan");
            continue;
        }
        for (int c = 0; c < 3; ++c) {
            CHECK(plan.work.origin[c] == std::max(box.origin[c], plan.lo[c]) && plan.work.end[c] == std::min(box.end[c], plan.hi[c] + 1), "the work box");
            CHECK(plan.range.b0[c] == plan.work.origin[c] / 8 && plan.range.b0[c] + plan.range.nb[c] - 1 == (plan.work.end[c] - 1) / 8, "its bricks");
            CHECK(plan.reach8[c] == paint_reach8(limit, w[c]), "reach");
        }
    }
    // the box is as tight as the reach: a ball of radius exactly 3 voxels at voxel (5, 5, 5)
    {
        const uint32_t w[3] = {1, 1, 1};
        const int32_t p[3] = {40, 40, 40};
        const VoxelBox box{{0, 0, 0}, {16, 16, 16}};
        PaintPlan plan;
        paint_plan(box, w, 576, p, 1, plan);
        CHECK(plan.lo[0] == 2 && plan.hi[0] == 8 && plan.work.origin[2] == 2 && plan.work.end[2] == 9, "a ball's box");
        paint_plan(box, w, 575, p, 1, plan);
        CHECK(plan.lo[0] == 3 && plan.hi[0] == 7, "a ball's box below the tie");
        const VoxelBox aside{{9, 0, 0}, {16, 16, 16}};
        paint_plan(aside, w, 575, p, 1, plan);
        CHECK(plan.empty, "a box beside the stroke");
    }
}

static void test_stroke()
{
    const int32_t dims[3] = {41, 27, 19};
    const uint32_t w[3] = {1, 1, 1};
    const float uvw[] = {0.0f, 0.5f, 1.0f, 0.0f, 0.5f, 1.0f, -3.0f, 0.5f, 2.0f, 0.25f, 0.26f, NAN, 1.0f, 1.0f, 1.0f};
    std::vector<int32_t> out;
    paint_stroke(dims, uvw, 5, w, out);
    const int32_t want[] = {0, 104, 144, 80, 54, 0, 320, 208, 144}; // duplicates dropped: the clamped third equals the first two
    CHECK(out.size() == 9, "points %zu", out.size());
    for (size_t i = 0; i < out.size() && i < 9; ++i) CHECK(out[i] == want[i], "point word %zu = %d", i, out[i]);
    // a long segment under heavy weights is split into the fewest equal parts below 2^30
    const int32_t big[3] = {16384, 16384, 16384};
    const uint32_t heavy[3] = {65535, 65535, 65535};
    const float ends[] = {0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 0.5f};
    paint_stroke(big, ends, 2, heavy, out);
    const size_t n = out.size() / 3;
    CHECK(n > 2 && n <= (size_t) kPaintMaxPoints * 4, "parts %zu", n);
    const int32_t hw[3] = {65535, 65535, 65535};
    int64_t longest = 0;
    for (size_t k = 0; k + 1 < n; ++k) {
        const int32_t d[3] = {out[3 * k + 3] - out[3 * k], out[3 * k + 4] - out[3 * k + 1], out[3 * k + 5] - out[3 * k + 2]};
        longest = std::max(longest, paint_dot(hw, d, d));
        for (int c = 0; c < 3; ++c) {
            const int64_t b = c < 2 ? 8 * 16383 : (int64_t) nearbyint(8.0 * 16383 * 0.5), num = (int64_t) (k + 1) * b;
            CHECK(out[3 * k + 3 + c] == (int32_t) (num / (int64_t) (n - 1)), "an inserted point is rounded down");
        }
    }
    CHECK(longest < (1ll << 30), "a part reaches 2^30");
    // ... the fewest: one part less and some part reaches it
    {
        const int64_t k = (int64_t) n - 2;
        const int32_t a[3] = {0, 0, 0}, b[3] = {out[3 * (n - 1)], out[3 * (n - 1) + 1], out[3 * (n - 1) + 2]};
        bool fits = true;
        int32_t p[3] = {0, 0, 0};
        for (int64_t j = 1; j <= k; ++j) {
            const int32_t q[3] = {paint_part(a[0], b[0], j, k), paint_part(a[1], b[1], j, k), paint_part(a[2], b[2], j, k)};
            const int32_t s[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
            fits = fits && paint_dot(hw, s, s) < (1ll << 30);
            for (int c = 0; c < 3; ++c) p[c] = q[c];
        }
        CHECK(!fits && paint_parts(hw, a, b) == (int64_t) n - 1, "fewer parts would do");
    }
    CHECK(paint_part(10, -11, 1, 2) == -1 && paint_part(-10, 11, 1, 2) == 0 && paint_part(5, 5, 3, 7) == 5, "rounded down, also downhill");
}

int main()
{
    test_rounding();
    test_rule();
    test_corners();
    test_arguments();
    test_plan();
    test_stroke();
    std::printf("failures=%d\n", failures);
    return failures ? 1 : 0;
}
