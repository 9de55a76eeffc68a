// tbrm_scissors_plan.h — the rules of tbrm_scissors_labels (include/tbrm_scissors.h) that are plain integer (and, for
// the two host functions, double) arithmetic: the bounds, the exact floor division, the verdict a brick's corners give, the mask
// summary's cells and its query, the projection rows of a camera and the polygon fill. The first four are what k_scissors runs, and
// they compile as host C++ too: tests/cpp/scissors_plan_test.cpp checks them against loops under the sanitizers.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "tbrm_box.h"
#include "../../include/tbrm_scissors.h"

namespace tbrm {

constexpr int kScissorsMaxImage = 16384;
constexpr int kScissorsCoordBits = 46;
constexpr int kScissorsOps = 4;
constexpr int kScissorsCellRows = 8;      // a cell of the mask summary: one word of 32 pixels, 8 rows
constexpr int kScissorsSummaryLaunches = 3;
enum : int { SCISSORS_ERASE_INSIDE = 0, SCISSORS_ERASE_OUTSIDE = 1, SCISSORS_FILL_INSIDE = 2, SCISSORS_FILL_OUTSIDE = 3 };

// ---- the bounds ----------------------------------------------------------------------------------------------------------------------
inline uint64_t scissors_abs(int64_t v) { return v < 0 ? 0ull - (uint64_t) v : (uint64_t) v; }

// |r0| (dim_x - 1) + |r1| (dim_y - 1) + |r2| (dim_z - 1) + |r3| < 2^46, formed without overflow: a term is refused before it is multiplied
inline bool scissors_row_admissible(const int64_t r[4], const int dims[3])
{
    const uint64_t limit = 1ull << kScissorsCoordBits;
    uint64_t sum = scissors_abs(r[3]);
    if (sum >= limit) return false;
    for (int c = 0; c < 3; ++c) {
        const uint64_t n = (uint64_t) (dims[c] - 1);
        if (n == 0) continue;
        const uint64_t a = scissors_abs(r[c]);
        if (a > limit / n) return false;
        sum += a * n; // (each term <= 2^46: four of them fit)
    }
    return sum < limit;
}

enum ScissorsRefusal : int { SCISSORS_OK = 0, SCISSORS_WIDTH, SCISSORS_HEIGHT, SCISSORS_U, SCISSORS_V, SCISSORS_W, SCISSORS_W_MIN, SCISSORS_W_MAX, SCISSORS_OP };

inline size_t scissors_row_words(int width) { return (size_t) ((width + 31) >> 5); }
inline size_t scissors_mask_words(int width, int height) { return scissors_row_words(width) * (size_t) height; }

inline ScissorsRefusal scissors_arguments(const tbrm_scissors_projection& p, int op, const int dims[3])
{
    if (p.width < 1 || p.width > kScissorsMaxImage) return SCISSORS_WIDTH;
    if (p.height < 1 || p.height > kScissorsMaxImage) return SCISSORS_HEIGHT;
    if (!scissors_row_admissible(p.u, dims)) return SCISSORS_U;
    if (!scissors_row_admissible(p.v, dims)) return SCISSORS_V;
    if (!scissors_row_admissible(p.w, dims)) return SCISSORS_W;
    if (p.w_min < 1) return SCISSORS_W_MIN;
    if (p.w_max < p.w_min) return SCISSORS_W_MAX;
    if (op < 0 || op >= kScissorsOps) return SCISSORS_OP;
    return SCISSORS_OK;
}

// the first row of the mask with a bit at or beyond width, or -1
inline int scissors_mask_stray_row(const uint32_t* words, int width, int height)
{
    if ((width & 31) == 0) return -1;
    const size_t rw = scissors_row_words(width);
    const uint32_t beyond = ~0u << (width & 31);
    for (int y = 0; y < height; ++y)
        if (words[(size_t) y * rw + rw - 1] & beyond) return y;
    return -1;
}

// ---- what the kernel runs ------------------------------------------------------------------------------------------------------------
struct ScissorsRows {
    int64_t u[4], v[4], w[4];
    int64_t w_min, w_max;
    int32_t width, height;
};

TBRM_BOARDS_HD int64_t scissors_dot(const int64_t r[4], int x, int y, int z) { return r[0] * x + r[1] * y + r[2] * z + r[3]; }

// 1 / W as the quotient's estimate uses it (W > 0)
TBRM_BOARDS_HD float scissors_rcp(int64_t W) { return 1.0f / (float) W; }

// floor(U / W) for W > 0 and 0 <= U < n * W with n <= 2^14 and n * W < 2^60: an estimate in float, then the integer correction — the
// result q is the one with q * W <= U < (q + 1) * W, whatever the estimate was
TBRM_BOARDS_HD int32_t scissors_quotient(int64_t U, int64_t W, float rcp, int32_t n)
{
    int64_t q = (int64_t) ((float) U * rcp);
    q = q < 0 ? 0 : (q > n - 1 ? n - 1 : q);
    int64_t r = U - q * W;
    while (r < 0) { --q; r += W; }
    while (r >= W) { ++q; r -= W; }
    return (int32_t) q;
}

// floor(U / W) clamped to [-1, n] for W > 0: -1 stands for every negative pixel, n for every pixel at or beyond n. Clamping is
// monotone, so a rectangle of clamped pixels still holds every clamped pixel between its corners, and a pixel of the frame is its own clamp.
TBRM_BOARDS_HD int32_t scissors_pixel(int64_t U, int64_t W, float rcp, int32_t n)
{
    if (U < 0) return -1;
    if (U >= (int64_t) n * W) return n;
    return scissors_quotient(U, W, rcp, n);
}

// the corner k (bit 0: x, 1: y, 2: z; set: the far one) of the in-volume part of brick b: b * 8, or b * 8 + 7 clamped to dim - 1
TBRM_BOARDS_HD int scissors_corner(int dim, int b, int far)
{
    const int lo = b * kBrick;
    if (!far) return lo;
    return lo + kBrick - 1 < dim ? lo + kBrick - 1 : dim - 1;
}

// ---- the mask summary ------------------------------------------------------------------------------------------------------------------
// A cell is the word cx of the rows 8 cy .. 8 cy + 7 that the mask has. It is FULL when every pixel of it inside the frame is set and
// CLEAR when none is. The summary is a summed-area table of both counts with a zero border: entry (cy, cx), cy <= ch, cx <= cw, counts
// the cells [0, cy) x [0, cx).
struct ScissorsCell { uint32_t full, clear; };
inline int scissors_cells_x(int width) { return (width + 31) >> 5; }
inline int scissors_cells_y(int height) { return (height + kScissorsCellRows - 1) / kScissorsCellRows; }
inline size_t scissors_summary_entries(int width, int height) { return (size_t) (scissors_cells_x(width) + 1) * (size_t) (scissors_cells_y(height) + 1); }

enum : int { SCISSORS_NEITHER = 0, SCISSORS_ALL_SET = 1, SCISSORS_ALL_CLEAR = 2 };

// the pixels [px0, px1] x [py0, py1], inside the frame: all set, all clear, or neither (also where it cannot tell)
TBRM_BOARDS_HD int scissors_summary_query(const ScissorsCell* sat, int cw, int px0, int py0, int px1, int py1)
{
    const int cx0 = px0 >> 5, cx1 = (px1 >> 5) + 1, cy0 = py0 / kScissorsCellRows, cy1 = py1 / kScissorsCellRows + 1;
    const size_t pitch = (size_t) cw + 1;
    const ScissorsCell a = sat[(size_t) cy0 * pitch + cx0], b = sat[(size_t) cy0 * pitch + cx1], c = sat[(size_t) cy1 * pitch + cx0], d = sat[(size_t) cy1 * pitch + cx1];
    const uint32_t cells = (uint32_t) (cx1 - cx0) * (uint32_t) (cy1 - cy0);
    if (d.full - b.full - c.full + a.full == cells) return SCISSORS_ALL_SET;
    if (d.clear - b.clear - c.clear + a.clear == cells) return SCISSORS_ALL_CLEAR;
    return SCISSORS_NEITHER;
}

// ---- the verdict of a brick's corners -------------------------------------------------------------------------------------------------
// Of the eight corner voxels of the brick's in-volume part: how many have W > 0, and of those (when all have) the extremes of W and of
// the clamped pixels. Every voxel of the brick has its W between the corners' and, when all eight are positive, its clamped pixel inside
// the rectangle: W is affine, U / W and V / W take their extremes over a box at its corners where W > 0, floor and the clamp are monotone.
struct ScissorsCorners {
    int positive;          // corners with W > 0
    int64_t w_lo, w_hi;
    int32_t px0, py0, px1, py1;
};

enum : int { SCISSORS_PROJECT = 0, SCISSORS_INSIDE = 1, SCISSORS_OUTSIDE = 2 };

TBRM_BOARDS_HD int scissors_verdict(const ScissorsCorners& k, const ScissorsRows& p, const ScissorsCell* sat, int cw)
{
    if (k.positive == 0) return SCISSORS_OUTSIDE; // W <= 0 at every corner, so at every voxel
    if (k.positive != 8) return SCISSORS_PROJECT;
    if (k.w_hi < p.w_min || k.w_lo > p.w_max) return SCISSORS_OUTSIDE;
    if (k.px1 < 0 || k.px0 >= p.width || k.py1 < 0 || k.py0 >= p.height) return SCISSORS_OUTSIDE;
    // the rectangle cut to the frame: what lies outside the frame is outside M anyway
    const int x0 = k.px0 < 0 ? 0 : k.px0, y0 = k.py0 < 0 ? 0 : k.py0, x1 = k.px1 >= p.width ? p.width - 1 : k.px1, y1 = k.py1 >= p.height ? p.height - 1 : k.py1;
    const int s = scissors_summary_query(sat, cw, x0, y0, x1, y1);
    if (s == SCISSORS_ALL_CLEAR) return SCISSORS_OUTSIDE;
    const bool framed = k.px0 >= 0 && k.py0 >= 0 && k.px1 < p.width && k.py1 < p.height;
    if (s == SCISSORS_ALL_SET && framed && k.w_lo >= p.w_min && k.w_hi <= p.w_max) return SCISSORS_INSIDE;
    return SCISSORS_PROJECT;
}

// the corners of brick (bx, by, bz), one after the other (the kernel takes one per lane and reduces)
inline ScissorsCorners scissors_corners(const ScissorsRows& p, const int dims[3], int bx, int by, int bz)
{
    ScissorsCorners k{0, INT64_MAX, INT64_MIN, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN};
    for (int c = 0; c < 8; ++c) {
        const int x = scissors_corner(dims[0], bx, c & 1), y = scissors_corner(dims[1], by, (c >> 1) & 1), z = scissors_corner(dims[2], bz, c >> 2);
        const int64_t W = scissors_dot(p.w, x, y, z);
        if (W <= 0) continue;
        ++k.positive;
        const float rcp = scissors_rcp(W);
        const int32_t px = scissors_pixel(scissors_dot(p.u, x, y, z), W, rcp, p.width), py = scissors_pixel(scissors_dot(p.v, x, y, z), W, rcp, p.height);
        k.w_lo = std::min(k.w_lo, W); k.w_hi = std::max(k.w_hi, W);
        k.px0 = std::min(k.px0, px); k.px1 = std::max(k.px1, px);
        k.py0 = std::min(k.py0, py); k.py1 = std::max(k.py1, py);
    }
    return k;
}

// the result bits of a row from its source bits S, its M bits and its in-volume bits
TBRM_BOARDS_HD uint32_t scissors_apply(int op, uint32_t S, uint32_t M, uint32_t vol)
{
    switch (op) {
    case SCISSORS_ERASE_INSIDE: return S & ~M;
    case SCISSORS_ERASE_OUTSIDE: return S & M;
    case SCISSORS_FILL_INSIDE: return (S | M) & vol;
    default: return (S | ~M) & vol;
    }
}

// ---- host only: the rows of a camera (include/tbrm_scissors.h) ------------------------------------------------------------------------
namespace scissors_host {

struct V3 { double x, y, z; };
inline V3 cross(const V3& a, const V3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double dot(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// FQuat::RotateVector, as tbrm_host_math.cpp states it
inline V3 rotate(const tbrm_quatd& q, const V3& v)
{
    const V3 qv{q.x, q.y, q.z};
    const V3 t0 = cross(qv, v), t{2.0 * t0.x, 2.0 * t0.y, 2.0 * t0.z}, c = cross(qv, t);
    return {v.x + t.x * q.w + c.x, v.y + t.y * q.w + c.y, v.z + t.z * q.w + c.z};
}
inline bool finite3(const tbrm_vec3d& v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// floor(x * 2^k + 0.5) as int64, for |x * 2^k| below 2^62
inline int64_t scaled(double x, int k) { return (int64_t) floor(ldexp(x, k) + 0.5); }

} // namespace scissors_host

enum ScissorsProjectionRefusal : int { SCISSORS_PROJ_OK = 0, SCISSORS_PROJ_DIMS, SCISSORS_PROJ_IMAGE, SCISSORS_PROJ_NOT_FINITE, SCISSORS_PROJ_TANGENT, SCISSORS_PROJ_DEPTH, SCISSORS_PROJ_SCALE };

// the three rows before scaling, [row][column], in double
inline ScissorsProjectionRefusal scissors_rows_double(const int32_t dims[3], const tbrm_transform& t, const tbrm_camera& cam, double rows[3][4])
{
    using namespace scissors_host;
    for (int c = 0; c < 3; ++c)
        if (dims[c] < 1) return SCISSORS_PROJ_DIMS;
    if (cam.width < 1 || cam.width > kScissorsMaxImage || cam.height < 1 || cam.height > kScissorsMaxImage) return SCISSORS_PROJ_IMAGE;
    if (!finite3(cam.position) || !finite3(cam.forward) || !finite3(cam.right) || !finite3(cam.up) || !isfinite(cam.tan_half_fov_x) || !isfinite(cam.tan_half_fov_y) ||
        !finite3(t.translation) || !finite3(t.scale3d) || !isfinite(t.rotation.x) || !isfinite(t.rotation.y) || !isfinite(t.rotation.z) || !isfinite(t.rotation.w))
        return SCISSORS_PROJ_NOT_FINITE;
    if (!(cam.tan_half_fov_x > 0.0) || !(cam.tan_half_fov_y > 0.0)) return SCISSORS_PROJ_TANGENT;
    const V3 axes[3] = {rotate(t.rotation, V3{t.scale3d.x, 0, 0}), rotate(t.rotation, V3{0, t.scale3d.y, 0}), rotate(t.rotation, V3{0, 0, t.scale3d.z})};
    // P(i) - position = sum_a axes[a] * ((i_a + 0.5) / d_a - 0.5) + translation - position
    V3 p0{t.translation.x - cam.position.x, t.translation.y - cam.position.y, t.translation.z - cam.position.z};
    V3 step[3];
    for (int a = 0; a < 3; ++a) {
        const double d = (double) dims[a], k0 = 0.5 / d - 0.5;
        step[a] = V3{axes[a].x / d, axes[a].y / d, axes[a].z / d};
        p0 = V3{p0.x + axes[a].x * k0, p0.y + axes[a].y * k0, p0.z + axes[a].z * k0};
    }
    const V3 right{cam.right.x, cam.right.y, cam.right.z}, up{cam.up.x, cam.up.y, cam.up.z}, fwd{cam.forward.x, cam.forward.y, cam.forward.z};
    const double hw = 0.5 * (double) cam.width, hh = 0.5 * (double) cam.height;
    for (int j = 0; j < 4; ++j) {
        const V3& g = j < 3 ? step[j] : p0;
        const double cr = dot(g, right), cu = dot(g, up), cf = dot(g, fwd);
        rows[0][j] = (cr / cam.tan_half_fov_x + cf) * hw;
        rows[1][j] = (cf - cu / cam.tan_half_fov_y) * hh;
        rows[2][j] = cf;
    }
    for (int r = 0; r < 3; ++r)
        for (int j = 0; j < 4; ++j)
            if (!isfinite(rows[r][j])) return SCISSORS_PROJ_NOT_FINITE;
    return SCISSORS_PROJ_OK;
}

inline ScissorsProjectionRefusal scissors_projection(const int32_t dims[3], const tbrm_transform& t, const tbrm_camera& cam, double depth_min, double depth_max,
                                                     tbrm_scissors_projection* out)
{
    using namespace scissors_host;
    double rows[3][4];
    if (const ScissorsProjectionRefusal e = scissors_rows_double(dims, t, cam, rows)) return e;
    if (isnan(depth_min) || isnan(depth_max) || depth_max < depth_min) return SCISSORS_PROJ_DEPTH;
    const int d[3] = {dims[0], dims[1], dims[2]};
    double reach = 0.0;
    for (int r = 0; r < 3; ++r) {
        double s = fabs(rows[r][3]);
        for (int c = 0; c < 3; ++c) {
            if (d[c] == 1) rows[r][c] = 0.0; // multiplies nothing
            s += fabs(rows[r][c]) * (double) (d[c] - 1);
        }
        reach = std::max(reach, s);
    }
    if (!(reach > 0.0) || !isfinite(reach)) return SCISSORS_PROJ_SCALE;
    // reach * 2^k0 lies in [2^46, 2^47): the largest admissible k is k0 or just below it (rounding moves a row's reach by a few units)
    const int k0 = kScissorsCoordBits - ilogb(reach);
    for (int k = k0; k >= k0 - 3; --k) {
        if (k < -1000 || k > 1000) continue;
        tbrm_scissors_projection p{};
        for (int j = 0; j < 4; ++j) { p.u[j] = scaled(rows[0][j], k); p.v[j] = scaled(rows[1][j], k); p.w[j] = scaled(rows[2][j], k); }
        if (!scissors_row_admissible(p.u, d) || !scissors_row_admissible(p.v, d) || !scissors_row_admissible(p.w, d)) continue;
        if (!(p.w[0] | p.w[1] | p.w[2] | p.w[3])) return SCISSORS_PROJ_SCALE;
        const double two63 = 9223372036854775808.0;
        const double lo = ceil(ldexp(depth_min, k)), hi = floor(ldexp(depth_max, k));
        p.w_min = lo < 1.0 ? 1 : (lo >= two63 ? INT64_MAX : (int64_t) lo);
        p.w_max = hi >= two63 ? INT64_MAX : (hi < 0.0 ? 0 : (int64_t) hi);
        if (p.w_max < p.w_min) return SCISSORS_PROJ_DEPTH; // the depth range holds no W
        p.width = cam.width;
        p.height = cam.height;
        p.scale_log2 = k;
        *out = p;
        return SCISSORS_PROJ_OK;
    }
    return SCISSORS_PROJ_SCALE;
}

// ---- host only: a polygon as a mask (include/tbrm_scissors.h) -----------------------------------------------------------------------
// Even-odd at the pixel centres. For a row yc and an edge a -> b that crosses it (half-open in y), the centres to the left of the edge
// are the pixels [0, L): L is estimated from the crossing and settled by the sign of the cross product alone. A pixel is inside when
// an odd number of the row's L lie beyond it.
inline bool scissors_polygon(const double* xy, size_t n, int width, int height, uint32_t* words)
{
    if (!xy || !words || n < 3 || width < 1 || width > kScissorsMaxImage || height < 1 || height > kScissorsMaxImage) return false;
    for (size_t i = 0; i < 2 * n; ++i)
        if (!isfinite(xy[i])) return false;
    const size_t rw = scissors_row_words(width);
    memset(words, 0, rw * (size_t) height * sizeof(uint32_t));
    std::vector<int> ends;
    for (int py = 0; py < height; ++py) {
        const double yc = (double) py + 0.5;
        ends.clear();
        for (size_t i = 0; i < n; ++i) {
            const double ax = xy[2 * i], ay = xy[2 * i + 1], bx = xy[2 * ((i + 1) % n)], by = xy[2 * ((i + 1) % n) + 1];
            const bool up = ay <= yc && yc < by, down = by <= yc && yc < ay;
            if (!up && !down) continue;
            // the centre xc is left of the crossing: cross > 0 on an upward edge, < 0 on a downward one
            auto left = [&](int px) {
                const double xc = (double) px + 0.5, cr = (bx - ax) * (yc - ay) - (by - ay) * (xc - ax);
                return up ? cr > 0.0 : cr < 0.0;
            };
            const double at = ax + (yc - ay) * (bx - ax) / (by - ay) - 0.5; // an estimate only
            int L = at <= 0.0 ? 0 : (at >= (double) width ? width : (int) ceil(at));
            while (L > 0 && !left(L - 1)) --L;
            while (L < width && left(L)) ++L;
            ends.push_back(L);
        }
        std::sort(ends.begin(), ends.end());
        for (size_t e = 0; e + 1 < ends.size(); e += 2)
            for (int px = ends[e]; px < ends[e + 1]; ++px) words[(size_t) py * rw + (size_t) (px >> 5)] |= 1u << (px & 31);
    }
    return true;
}

} // namespace tbrm
