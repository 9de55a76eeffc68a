// tbrm_paint_plan.h — the rules of tbrm_paint_labels (include/tbrm_paint.h) that are plain integer (and, for the two
// host functions, double) arithmetic: the bounds, the reaches, the distance rule of a voxel and a segment, the segments' and runs'
// grown boxes, the work box, and the two host helpers. The distance rule and the box tests are what k_paint runs, and they compile as
// host C++ too: tests/cpp/paint_plan_test.cpp checks them against loops under the sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "tbrm_box.h"

namespace tbrm {

constexpr int kPaintMaxPoints = 4096;
constexpr int kPaintMaxCoord = 1 << 18;
constexpr int kPaintMaxDim = 16384;
constexpr int kPaintMaxWeight = 65535;
constexpr uint32_t kPaintMaxLimit = (1u << 30) - 1u;
constexpr int kPaintMaxReach = 64;
constexpr int kPaintRun = 64;        // segments to a run: a lane each
constexpr int kPaintMaxRuns = (kPaintMaxPoints + kPaintRun - 1) / kPaintRun; // 64: a lane each
constexpr int kPaintOps = 2;
constexpr int kPaintLaunches = 3;    // k_morph_load, k_paint, k_morph_write
enum : int { PAINT_PAINT = 0, PAINT_ERASE = 1 };

// ---- the bounds ----------------------------------------------------------------------------------------------------------------------
// the largest n with n * n <= v
inline uint32_t paint_isqrt(uint32_t v)
{
    uint64_t n = (uint64_t) sqrt((double) v);
    while (n * n > v) --n;
    while ((n + 1) * (n + 1) <= v) ++n;
    return (uint32_t) n;
}

// the reach along an axis of weight w (>= 1) in eighths of a voxel: the largest n with w n^2 <= limit; and in voxels, rounded up
inline int paint_reach8(uint32_t limit, uint32_t w) { return (int) paint_isqrt(limit / w); }
inline int paint_reach_voxels(int reach8) { return (reach8 + 7) / 8; }

inline int paint_floor8(int v) { return v >= 0 ? v / 8 : -((7 - v) / 8); } // floor(v / 8)
inline int paint_ceil8(int v) { return -paint_floor8(-v); }                // ceil(v / 8)

inline int paint_segments(size_t n_points) { return n_points > 1 ? (int) n_points - 1 : 1; } // one point is one ball

// <p, q> of two vectors in eighths (|p_a|, |q_a| <= 2^19: below 2^56)
TBRM_BOARDS_HD int64_t paint_dot(const int32_t w[3], const int32_t p[3], const int32_t q[3])
{
    return (int64_t) w[0] * p[0] * q[0] + (int64_t) w[1] * p[1] * q[1] + (int64_t) w[2] * p[2] * q[2];
}

enum PaintRefusal : int { PAINT_OK = 0, PAINT_DIMS, PAINT_N_POINTS, PAINT_OP, PAINT_GATE, PAINT_WEIGHT, PAINT_LIMIT, PAINT_REACH, PAINT_COORD, PAINT_SEGMENT };
struct PaintVerdict { int what, index, axis; }; // index: the point or the segment; axis: of a weight, a reach, a coordinate

// everything of a call but the box, the labels and the gate's range
inline PaintVerdict paint_arguments(const int dims[3], int op, int gate, const uint32_t weights[3], uint32_t limit, const int32_t* points, size_t n_points)
{
    for (int c = 0; c < 3; ++c)
        if (dims[c] > kPaintMaxDim) return {PAINT_DIMS, 0, c};
    if (n_points < 1 || n_points > (size_t) kPaintMaxPoints) return {PAINT_N_POINTS, 0, 0};
    if (op < 0 || op >= kPaintOps) return {PAINT_OP, 0, 0};
    if (gate != 0 && gate != 1) return {PAINT_GATE, 0, 0};
    for (int c = 0; c < 3; ++c)
        if (weights[c] < 1u || weights[c] > (uint32_t) kPaintMaxWeight) return {PAINT_WEIGHT, 0, c};
    if (limit < 1u || limit > kPaintMaxLimit) return {PAINT_LIMIT, 0, 0};
    for (int c = 0; c < 3; ++c)
        if (paint_reach_voxels(paint_reach8(limit, weights[c])) > kPaintMaxReach) return {PAINT_REACH, 0, c};
    for (size_t k = 0; k < n_points; ++k)
        for (int c = 0; c < 3; ++c)
            if (points[3 * k + c] < -kPaintMaxCoord || points[3 * k + c] > kPaintMaxCoord) return {PAINT_COORD, (int) k, c};
    const int32_t w[3] = {(int32_t) weights[0], (int32_t) weights[1], (int32_t) weights[2]};
    for (size_t k = 0; k + 1 < n_points; ++k) {
        const int32_t d[3] = {points[3 * k + 3] - points[3 * k], points[3 * k + 4] - points[3 * k + 1], points[3 * k + 5] - points[3 * k + 2]};
        if (paint_dot(w, d, d) >= (int64_t) 1 << 30) return {PAINT_SEGMENT, (int) k, 0};
    }
    return {PAINT_OK, 0, 0};
}

// ---- what the kernel runs ------------------------------------------------------------------------------------------------------------
// a segment a -> a + d with dd = <d, d> and the voxels [lo, hi] its grown bounding box holds (not cut to the volume); 64 bytes
struct PaintSegment {
    int32_t a[3], d[3];
    int32_t dd;
    int32_t lo[3], hi[3];
    int32_t pad[3];
};
// a run of consecutive segments and the union of their boxes
struct PaintRun {
    int32_t lo[3], hi[3];
    int32_t first, count;
};
static_assert(sizeof(PaintSegment) == 64 && sizeof(PaintRun) == 32, "staged as they are");

// THE distance rule (include/tbrm_paint.h): is a voxel with these products within the segment? ee, |de| < 2^56; dd, limit < 2^30.
TBRM_BOARDS_HD bool paint_within(int64_t ee, int64_t de, int64_t dd, int64_t limit)
{
    if (ee > 2 * (dd + limit)) return false; // beyond every voxel within the segment; behind it ee < 2^32 and the products fit
    if (de <= 0) return ee <= limit;
    if (de >= dd) return ee - 2 * de + dd <= limit;
    return ee * dd - de * de <= limit * dd;
}

// ee and de of the voxel (x, y, z)
TBRM_BOARDS_HD void paint_products(const PaintSegment& g, const int32_t w[3], int x, int y, int z, int64_t& ee, int64_t& de)
{
    const int32_t e[3] = {8 * x - g.a[0], 8 * y - g.a[1], 8 * z - g.a[2]};
    ee = paint_dot(w, e, e);
    de = paint_dot(w, g.d, e);
}

TBRM_BOARDS_HD bool paint_voxel_within(const PaintSegment& g, const int32_t w[3], int64_t limit, int x, int y, int z)
{
    int64_t ee, de;
    paint_products(g, w, x, y, z, ee, de);
    return paint_within(ee, de, g.dd, limit);
}

// the 8 voxels x0 .. x0 + 7 of the row (y, z): bit i is voxel x0 + i. The products advance along x by additions:
// ee(x + 1) - ee(x) = w_x ((e_x + 8)^2 - e_x^2) = w_x (16 e_x + 64), de(x + 1) - de(x) = 8 w_x d_x.
TBRM_BOARDS_HD uint32_t paint_row_within(const PaintSegment& g, const int32_t w[3], int64_t limit, int x0, int y, int z)
{
    int64_t ee, de;
    paint_products(g, w, x0, y, z, ee, de);
    int64_t ee_step = (int64_t) w[0] * (16 * (int64_t) (8 * x0 - g.a[0]) + 64);
    const int64_t ee_step2 = 128 * (int64_t) w[0], de_step = 8 * (int64_t) w[0] * g.d[0];
    uint32_t bits = 0u;
    TBRM_BOARDS_UNROLL
    for (int i = 0; i < kBrick; ++i) {
        bits |= (uint32_t) paint_within(ee, de, g.dd, limit) << i;
        ee += ee_step;
        ee_step += ee_step2;
        de += de_step;
    }
    return bits;
}

// do the voxels [lo, hi] and [blo, bhi] share one?
TBRM_BOARDS_HD bool paint_boxes_meet(const int32_t lo[3], const int32_t hi[3], const int32_t blo[3], const int32_t bhi[3])
{
    return lo[0] <= bhi[0] && hi[0] >= blo[0] && lo[1] <= bhi[1] && hi[1] >= blo[1] && lo[2] <= bhi[2] && hi[2] >= blo[2];
}

// the corner k (bit 0: x, 1: y, 2: z; set: the far one) of the in-volume part of brick b along an axis of dim voxels: the rule of
// scissors_corner
TBRM_BOARDS_HD int paint_corner(int dim, int b, int far)
{
    const int lo = b * kBrick;
    if (!far) return lo;
    return lo + kBrick - 1 < dim ? lo + kBrick - 1 : dim - 1;
}

// are the eight corners of the voxels [blo, bhi] all within the segment? Then every voxel between them is: the set is convex.
TBRM_BOARDS_HD bool paint_corners_within(const PaintSegment& g, const int32_t w[3], int64_t limit, const int32_t blo[3], const int32_t bhi[3])
{
    bool all = true;
    for (int c = 0; c < 8; ++c)
        all = all && paint_voxel_within(g, w, limit, (c & 1) ? bhi[0] : blo[0], (c & 2) ? bhi[1] : blo[1], (c & 4) ? bhi[2] : blo[2]);
    return all;
}

// the result bits of a row from its source bits S, its M bits (inside vol) and its in-volume bits
TBRM_BOARDS_HD uint32_t paint_apply(int op, uint32_t S, uint32_t M) { return op == PAINT_PAINT ? (S | M) : (S & ~M); }

// ---- the plan of a call ----------------------------------------------------------------------------------------------------------------
struct PaintPlan {
    int reach8[3];                  // per axis, in eighths
    std::vector<PaintSegment> segs;
    std::vector<PaintRun> runs;
    int32_t lo[3], hi[3];           // the voxels the stroke's bounding box grown by the reach holds (not cut to anything)
    bool empty;                     // the work box holds no voxel: the call does nothing
    VoxelBox work;                  // the box cut to [lo, hi]
    BrickRange range;               // the bricks it touches
};

// of admissible arguments (paint_arguments) and a box inside the volume
inline void paint_plan(const VoxelBox& box, const uint32_t weights[3], uint32_t limit, const int32_t* points, size_t n_points, PaintPlan& plan)
{
    const int32_t w[3] = {(int32_t) weights[0], (int32_t) weights[1], (int32_t) weights[2]};
    for (int c = 0; c < 3; ++c) plan.reach8[c] = paint_reach8(limit, weights[c]);
    const int n_seg = paint_segments(n_points);
    plan.segs.assign((size_t) n_seg, PaintSegment{});
    plan.runs.clear();
    for (int k = 0; k < n_seg; ++k) {
        PaintSegment& g = plan.segs[(size_t) k];
        const int32_t* a = points + 3 * (size_t) k;
        const int32_t* b = n_points > 1 ? a + 3 : a;
        for (int c = 0; c < 3; ++c) {
            g.a[c] = a[c];
            g.d[c] = b[c] - a[c];
            g.lo[c] = paint_ceil8(std::min(a[c], b[c]) - plan.reach8[c]);
            g.hi[c] = paint_floor8(std::max(a[c], b[c]) + plan.reach8[c]);
        }
        g.dd = (int32_t) paint_dot(w, g.d, g.d);
        if (k % kPaintRun == 0) {
            PaintRun r{};
            for (int c = 0; c < 3; ++c) { r.lo[c] = g.lo[c]; r.hi[c] = g.hi[c]; }
            r.first = k;
            plan.runs.push_back(r);
        }
        PaintRun& r = plan.runs.back();
        for (int c = 0; c < 3; ++c) { r.lo[c] = std::min(r.lo[c], g.lo[c]); r.hi[c] = std::max(r.hi[c], g.hi[c]); }
        ++r.count;
    }
    plan.empty = false;
    for (int c = 0; c < 3; ++c) {
        plan.lo[c] = plan.runs[0].lo[c];
        plan.hi[c] = plan.runs[0].hi[c];
        for (const PaintRun& r : plan.runs) { plan.lo[c] = std::min(plan.lo[c], r.lo[c]); plan.hi[c] = std::max(plan.hi[c], r.hi[c]); }
        plan.work.origin[c] = std::max(box.origin[c], plan.lo[c]);
        plan.work.end[c] = std::min(box.end[c], plan.hi[c] + 1);
        if (plan.work.end[c] <= plan.work.origin[c]) plan.empty = true;
    }
    plan.range = BrickRange{};
    if (plan.empty) plan.work = VoxelBox{};
    else
        for (int c = 0; c < 3; ++c) axis_bricks(plan.work.origin[c], plan.work.end[c], plan.range.b0[c], plan.range.nb[c]);
}

// ---- host only: spacing and radius -> limit; unit-cube positions -> points (include/tbrm_paint.h) ---------------------------------------
// the margin's weights and limit (tbrm_host_margin_weights) as the brush's: false when they break the brush's bounds
inline bool paint_brush_admissible(const uint32_t weights[3], uint32_t margin_limit, uint32_t* limit)
{
    if (margin_limit < 1u || margin_limit > kPaintMaxLimit / 64u) return false;
    for (int c = 0; c < 3; ++c) {
        if (weights[c] < 1u || weights[c] > (uint32_t) kPaintMaxWeight) return false;
        if (paint_reach_voxels(paint_reach8(margin_limit * 64u, weights[c])) > kPaintMaxReach) return false;
    }
    *limit = margin_limit * 64u;
    return true;
}

// the point of a unit-cube position
inline void paint_quantise(const int32_t dims[3], const float uvw[3], int32_t out[3])
{
    for (int c = 0; c < 3; ++c) {
        double u = (double) uvw[c];
        u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
        if (!(u == u)) u = 0.0;
        out[c] = (int32_t) nearbyint(8.0 * (double) (dims[c] - 1) * u);
    }
}

// a + floor(j (b - a) / k) for 0 <= j <= k
inline int32_t paint_part(int32_t a, int32_t b, int64_t j, int64_t k)
{
    const int64_t n = j * ((int64_t) b - a);
    return (int32_t) (a + (n >= 0 ? n / k : -((-n + k - 1) / k)));
}

// the fewest equal parts of a -> b whose dd all stay below 2^30
inline int64_t paint_parts(const int32_t w[3], const int32_t a[3], const int32_t b[3])
{
    const int32_t d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const int64_t dd = paint_dot(w, d, d), top = (int64_t) 1 << 30;
    if (dd < top) return 1;
    int64_t k = (int64_t) sqrt((double) dd / (double) top); // parts of length 1 / k have dd / k^2 before rounding: no fewer than this
    if (k < 2) k = 2;
    for (;; ++k) {
        bool fits = true;
        int32_t p[3] = {a[0], a[1], a[2]};
        for (int64_t j = 1; j <= k && fits; ++j) {
            const int32_t q[3] = {paint_part(a[0], b[0], j, k), paint_part(a[1], b[1], j, k), paint_part(a[2], b[2], j, k)};
            const int32_t s[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
            fits = paint_dot(w, s, s) < top;
            for (int c = 0; c < 3; ++c) p[c] = q[c];
        }
        if (fits) return k;
    }
}

// tbrm_host_paint_stroke: the points (appended to out); dims >= 1, weights 1 .. 65535
inline void paint_stroke(const int32_t dims[3], const float* uvw, size_t n, const uint32_t weights[3], std::vector<int32_t>& out)
{
    const int32_t w[3] = {(int32_t) weights[0], (int32_t) weights[1], (int32_t) weights[2]};
    out.clear();
    for (size_t i = 0; i < n; ++i) {
        int32_t q[3];
        paint_quantise(dims, uvw + 3 * i, q);
        if (!out.empty()) {
            int32_t p[3];
            memcpy(p, out.data() + out.size() - 3, sizeof(p));
            if (p[0] == q[0] && p[1] == q[1] && p[2] == q[2]) continue;
            const int64_t k = paint_parts(w, p, q);
            for (int64_t j = 1; j < k; ++j)
                for (int c = 0; c < 3; ++c) out.push_back(paint_part(p[c], q[c], j, k));
        }
        out.insert(out.end(), q, q + 3);
    }
}

} // namespace tbrm
