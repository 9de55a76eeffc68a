// The footprint rules of the light occlusion (tbraymarcherplugin_amd/csrc/tbrm_occ_footprint.h) on their own, each against the answer
// found position by position: texel_split against exact double arithmetic, the tap span of a block's two ends against the minimum and
// maximum over every position of the block, brick range / border flag / staging decision against the bricks that the taps of every
// sample of a unit touch, the staged block filled through the staged brick order and read through the staged offsets against the
// bricked volume, a pass's tap spans (the block-list signature) against the per-unit rule, factor_block around its cap.
// Pure host code, no device; tests/test_occ_footprint.py builds it with -ffp-contract=off -fsanitize=address,undefined and runs it.
// Prints "failures=N" last.
#include "../../tbraymarcherplugin_amd/csrc/tbrm_occ_footprint.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace tbrm;

static int failures = 0;
static long checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) {                                                     \
            if (++failures <= 20) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
        }                                                                  \
    } while (0)

static const int kWidths[8] = {1, 7, 8, 9, 17, 40, 48, 96};
// offsets in texels of the light volume; the last three only meet the clamp
static const float kNaN = std::numeric_limits<float>::quiet_NaN();
static const float kOffsets[13] = {0.0f, 1e-8f, -1e-8f, 0.3f, -0.3f, 1.0f, -1.0f, 2.6f, -2.6f, kNaN, 1e30f, -1e30f, 0.0f};
static const int kFiniteOffsets = 9, kAllOffsets = 12;

static float uvw_offset(int k, int lv) { return kOffsets[k] / (float) lv; }
static int clampi(int c, int n) { return std::min(std::max(c, 0), n - 1); }

// ---- texel_split against double arithmetic that is exact at every step ------------------------------------------------------------
static void check_texel_split(float u, float n)
{
    int i0;
    float f;
    texel_split(u, n, i0, f);
    const float prod = (float) ((double) u * (double) n); // exact product, one rounding: the float multiplication
    float x = (float) ((double) prod - 0.5);              // exact difference, one rounding
    if (std::isnan(x) || x < -0x1p30f) x = -0x1p30f;      // fmax(NaN, a) = a
    if (x > 0x1p30f) x = 0x1p30f;
    const double fl = std::floor((double) x);
    const float want_f = (float) ((double) x - fl);
    CHECK(i0 == (int) fl);
    CHECK(std::memcmp(&f, &want_f, 4) == 0);
    CHECK(base_tap(u, n) == i0);
    const float xc = texel_coord(u, n);
    CHECK(std::memcmp(&xc, &x, 4) == 0);
}

// ---- one axis: spans, brick ranges, border flags ------------------------------------------------------------------------------------------
struct Axis {
    int data, lv;     // texels of the data volume, positions of the light volume
    int ns;
    float off[2];
};
static int tap_of(const Axis& a, int si, int pos) { return base_tap(sample_coord(pos, a.lv, a.off[si]), (float) a.data); }

// the positions first .. last (either order): span from the two ends == span over every position; then the bricks and the border flag
// against every tap
static void check_span(const Axis& a, int first, int last)
{
    int lo = INT32_MAX, hi = INT32_MIN;
    for (int si = 0; si < a.ns; ++si) tap_span_add(first, last, a.lv, a.off[si], a.data, lo, hi);
    int lo_all = INT32_MAX, hi_all = INT32_MIN, b_min = INT32_MAX, b_max = INT32_MIN;
    bool outside = false;
    for (int si = 0; si < a.ns; ++si)
        for (int pos = std::min(first, last); pos <= std::max(first, last); ++pos) {
            const int i0 = tap_of(a, si, pos);
            lo_all = std::min(lo_all, i0);
            hi_all = std::max(hi_all, i0 + 1);
            for (int t = i0; t <= i0 + 1; ++t) {
                outside = outside || t < 0 || t >= a.data;
                b_min = std::min(b_min, clampi(t, a.data) >> 3);
                b_max = std::max(b_max, clampi(t, a.data) >> 3);
            }
        }
    CHECK(lo == lo_all && hi == hi_all); // the monotonicity every user of the rule relies on
    const int bn = (a.data + 7) >> 3;
    int b0, nb;
    bool border;
    brick_span(lo, hi, a.data, bn, b0, nb, border);
    CHECK(border == outside);
    CHECK(nb >= 0 && b0 >= 0 && b0 + nb <= std::max(bn, b0));
    if (nb > 0) CHECK(b0 == b_min && b0 + nb - 1 == b_max);
    else CHECK(hi < 0 || lo >= a.data || (lo < 0 && hi < 8)); // no brick: every tap lies outside the volume (the unit is not staged)
    if (nb == 0) CHECK(border);
}

static void check_axis(const Axis& a)
{
    for (int si = 0; si < a.ns; ++si)
        for (int pos = 0; pos < a.lv; ++pos) check_texel_split(sample_coord(pos, a.lv, a.off[si]), (float) a.data);
    for (int b = 0; b * kOccTile < a.lv; ++b) { // plane blocks
        int first, last;
        block_ends(b, a.lv, first, last);
        CHECK(first == b * 16 && last == std::min(b * 16 + 15, a.lv - 1));
        check_span(a, first, last);
    }
    for (int dir = -1; dir <= 1; dir += 2) // slice groups, both pass directions
        for (int k0 = 0; k0 < a.lv; k0 += kOccDepth) {
            int first, last;
            group_ends(k0, a.lv, dir > 0 ? 0 : a.lv - 1, dir, first, last);
            CHECK(first >= 0 && first < a.lv && last >= 0 && last < a.lv && (last - first) * dir == std::min(kOccDepth, a.lv - k0) - 1);
            check_span(a, first, last);
        }
}

// ---- a volume: units, the staging decision, the staged block ---------------------------------------------------------------------------
struct Scene {
    int data[3], lv[3];
    int ns, dir, esz;
    float off[2][3];
};

static void check_units(const Scene& s, long& staged_units, long& unstaged_units, long& edge_units)
{
    const int bn[3] = {(s.data[0] + 7) >> 3, (s.data[1] + 7) >> 3, (s.data[2] + 7) >> 3};
    const int bnx = bn[0], bnxy = bn[0] * bn[1];
    const size_t voxels = (size_t) bnxy * bn[2] * kBrickVoxels;
    std::vector<unsigned char> vol(voxels * s.esz);
    for (size_t i = 0; i < vol.size(); ++i) vol[i] = (unsigned char) ((i * 2654435761u) >> 13); // (esz = 4: distinct voxels up to 2^19)
    if (s.esz == 4)
        for (size_t i = 0; i < voxels; ++i) { const uint32_t v = (uint32_t) i; std::memcpy(&vol[4 * i], &v, 4); }
    const int budget = 96 * 1024, pieces = kBrickVoxels * s.esz / 16;
    std::vector<unsigned char> lds;
    for (int gz = 0; gz * kOccDepth < s.lv[2]; ++gz)
        for (int gy = 0; gy * kOccTile < s.lv[1]; ++gy)
            for (int gx = 0; gx * kOccTile < s.lv[0]; ++gx) {
                int first[3], last[3];
                block_ends(gx, s.lv[0], first[0], last[0]);
                block_ends(gy, s.lv[1], first[1], last[1]);
                group_ends(gz * kOccDepth, s.lv[2], s.dir > 0 ? 0 : s.lv[2] - 1, s.dir, first[2], last[2]);
                int b0[3], nb[3];
                bool border = false;
                for (int a = 0; a < 3; ++a) {
                    int lo = INT32_MAX, hi = INT32_MIN;
                    for (int si = 0; si < s.ns; ++si) tap_span_add(first[a], last[a], s.lv[a], s.off[si][a], s.data[a], lo, hi);
                    bool b;
                    brick_span(lo, hi, s.data[a], bn[a], b0[a], nb[a], b);
                    border = border || b;
                }
                const int count = nb[0] * nb[1] * nb[2];
                const bool staged = bricks_staged(count, s.esz, budget);
                // the bricks every tap of every sample touches, clamped into the volume
                int t_lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, t_hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
                bool outside = false;
                for (int a = 0; a < 3; ++a)
                    for (int si = 0; si < s.ns; ++si)
                        for (int pos = std::min(first[a], last[a]); pos <= std::max(first[a], last[a]); ++pos) {
                            const int i0 = base_tap(sample_coord(pos, s.lv[a], s.off[si][a]), (float) s.data[a]);
                            for (int t = i0; t <= i0 + 1; ++t) {
                                outside = outside || t < 0 || t >= s.data[a];
                                t_lo[a] = std::min(t_lo[a], clampi(t, s.data[a]) >> 3);
                                t_hi[a] = std::max(t_hi[a], clampi(t, s.data[a]) >> 3);
                            }
                        }
                CHECK(border == outside);
                const long touched = (long) (t_hi[0] - t_lo[0] + 1) * (t_hi[1] - t_lo[1] + 1) * (t_hi[2] - t_lo[2] + 1);
                if (count > 0) {
                    CHECK(count == touched);
                    CHECK(staged == (touched <= kOccMaxBricks && touched * kBrickVoxels * s.esz <= budget));
                } else CHECK(!staged);
                if (!staged) { ++unstaged_units; continue; }
                ++staged_units;
                // fill the staged block through the staged brick order
                lds.assign((size_t) count * kBrickVoxels * s.esz, 0xEE);
                const int nxy = nb[0] * nb[1];
                for (int c = 0; c < count * pieces; ++c) {
                    const int lb = c / pieces;
                    const uint32_t gb = staged_brick_xy(lb % nxy, b0[0], b0[1], nb[0], bnx) + staged_brick_z(lb / nxy, b0[2], bnxy);
                    const size_t src = staged_piece_src(gb, c, pieces, s.esz);
                    CHECK(src + 16 <= vol.size());
                    if (src + 16 <= vol.size()) std::memcpy(&lds[(size_t) c * 16], &vol[src], 16);
                }
                // every tap of every sample: the staged offset reads what the volume's offset reads
                bool beyond = false; // some unclamped tap lies outside the staged block
                for (int si = 0; si < s.ns; ++si)
                    for (int pz = std::min(first[2], last[2]); pz <= std::max(first[2], last[2]); ++pz)
                        for (int py = first[1]; py <= last[1]; ++py)
                            for (int px = first[0]; px <= last[0]; ++px) {
                                const int pos[3] = {px, py, pz};
                                int i0[3];
                                for (int a = 0; a < 3; ++a) i0[a] = base_tap(sample_coord(pos[a], s.lv[a], s.off[si][a]), (float) s.data[a]);
                                for (int k = 0; k < 8; ++k) {
                                    const int x = i0[0] + (k & 1), y = i0[1] + ((k >> 1) & 1), z = i0[2] + (k >> 2);
                                    beyond = beyond || (x >> 3) < b0[0] || (x >> 3) >= b0[0] + nb[0] || (y >> 3) < b0[1] || (y >> 3) >= b0[1] + nb[1] || (z >> 3) < b0[2] ||
                                             (z >> 3) >= b0[2] + nb[2];
                                    const int cx = tap_coord(x, s.data[0]), cy = tap_coord(y, s.data[1]), cz = tap_coord(z, s.data[2]);
                                    CHECK(cx == clampi(x, s.data[0]) && cy == clampi(y, s.data[1]) && cz == clampi(z, s.data[2]));
                                    const uint32_t so = staged_off<0>(cx, b0[0], nb[0], 1u) + staged_off<1>(cy, b0[1], nb[1], (uint32_t) nb[0]) + staged_off<2>(cz, b0[2], nb[2], (uint32_t) nxy);
                                    const uint32_t vo = brick_off_x(cx) + brick_off_y(cy, bnx) + brick_off_z(cz, bnxy);
                                    CHECK((size_t) so < (size_t) count * kBrickVoxels && (size_t) vo < voxels);
                                    if ((size_t) so < (size_t) count * kBrickVoxels && (size_t) vo < voxels)
                                        CHECK(std::memcmp(&lds[(size_t) so * s.esz], &vol[(size_t) vo * s.esz], s.esz) == 0);
                                }
                            }
                if (beyond) ++edge_units;
            }
}

// ---- the block-list signature: a pass's spans from the one function == the per-unit rule ----------------------------------------
static void check_signature(const Scene& sc, int axis)
{
    OccPassShape s;
    const int dim_u = axis == 0 ? 1 : 0, dim_v = axis == 2 ? 1 : 2;
    s.axis = axis; s.W = sc.lv[dim_u]; s.H = sc.lv[dim_v]; s.dir = sc.dir;
    const int depth = (sc.lv[axis] + 7) / 8 * 8; // (a swept pass runs over whole brick layers)
    s.start = sc.dir > 0 ? 0 : depth - 1;
    s.slices = depth;
    s.blocks_x = (s.W + 15) / 16; s.blocks_y = (s.H + 15) / 16; s.groups = depth / 8 + 1; // (one group past the last slice)
    s.ns = sc.ns;
    for (int a = 0; a < 3; ++a) { s.data_dims[a] = sc.data[a]; s.lv_dims[a] = sc.lv[a]; s.uvw_off[0][a] = sc.off[0][a]; s.uvw_off[1][a] = sc.off[1][a]; }
    std::vector<int> sig;
    pass_tap_spans(s, [&](int lo, int hi) { sig.push_back(lo); sig.push_back(hi); });
    CHECK((int) sig.size() == 2 * (s.blocks_x + s.blocks_y + s.groups));
    size_t at = 0;
    auto expect = [&](int dim, int first, int last) {
        int lo = INT32_MAX, hi = INT32_MIN;
        for (int si = 0; si < sc.ns; ++si)
            for (int pos : {first, last}) tap_span_add(base_tap(sample_coord(pos, sc.lv[dim], sc.off[si][dim]), (float) sc.data[dim]), lo, hi);
        CHECK(at + 2 <= sig.size() && sig[at] == lo && sig[at + 1] == hi);
        at += 2;
    };
    for (int bx = 0; bx < s.blocks_x; ++bx) expect(dim_u, bx * 16, std::min(bx * 16 + 16, s.W) - 1);
    for (int by = 0; by < s.blocks_y; ++by) expect(dim_v, by * 16, std::min(by * 16 + 16, s.H) - 1);
    for (int zg = 0; zg < s.groups - 1; ++zg) expect(axis, s.start + zg * 8 * s.dir, s.start + (zg * 8 + 7) * s.dir);
    CHECK(at + 2 == sig.size() && sig[at] == 0 && sig[at + 1] == -1); // the group past the last slice
    int lo = 7, hi = 7;
    CHECK(!pass_tap_span(s, 2, s.groups - 1, lo, hi) && lo == 7 && hi == 7);
}

int main()
{
    // one axis: every width, light volume of the same and of half resolution, every offset, one and two streams
    for (int n : kWidths)
        for (int lv : {n, (n + 1) / 2})
            for (int k = 0; k < kAllOffsets; ++k)
                for (int ns = 1; ns <= 2; ++ns) {
                    Axis a{n, lv, ns, {uvw_offset(k, lv), uvw_offset(k + 1, lv)}};
                    check_axis(a);
                }
    for (float u : {0.0f, 1.0f, -0.0f, 0.5f, 1e-38f, -1e-38f, 3e38f, -3e38f, kNaN, 0.49999997f, 0x1p30f, -0x1p30f})
        for (float n : {1.0f, 8.0f, 9.0f, 96.0f, 256.0f}) check_texel_split(u, n);

    // volumes: units against every tap of every sample, and the staged block
    const int volumes[5][3] = {{17, 40, 9}, {96, 17, 9}, {40, 48, 8}, {1, 7, 17}, {9, 8, 96}};
    long staged_units = 0, unstaged_units = 0, edge_units = 0, combo = 0;
    for (const auto& v : volumes)
        for (int half = 0; half < 2; ++half)
            for (int k = 0; k < kFiniteOffsets; k += 2)
                for (int dir = -1; dir <= 1; dir += 2) {
                    Scene s;
                    for (int a = 0; a < 3; ++a) {
                        s.data[a] = v[a];
                        s.lv[a] = half ? (v[a] + 1) / 2 : v[a];
                        s.off[0][a] = uvw_offset((k + 3 * a) % kFiniteOffsets, s.lv[a]);
                        s.off[1][a] = uvw_offset((k + 3 * a + 4) % kFiniteOffsets, s.lv[a]);
                    }
                    s.ns = 1 + (int) (combo % 2);
                    s.dir = dir;
                    s.esz = (combo / 2) % 2 ? 4 : 1;
                    ++combo;
                    check_units(s, staged_units, unstaged_units, edge_units);
                    for (int axis = 0; axis < 3; ++axis) check_signature(s, axis);
                }
    // units of both kinds occurred, and staged units with taps outside their block (outside the volume: clamped into it)
    CHECK(staged_units > 0 && unstaged_units > 0 && edge_units > 0);
    // a coordinate beyond the staged block reads the block's edge brick (the kernels never ask for one: a unit's own ends span its taps)
    CHECK(staged_off<0>(3, 2, 3, 1u) == 3u && staged_off<0>(16, 2, 3, 1u) == 0u && staged_off<0>(95, 2, 3, 1u) == 2u * 512u + 7u);
    CHECK(staged_off<1>(95, 2, 3, 5u) == (2u * 5u * 512u) + (7u << 3));
    CHECK(tap_coord(-4, 96) == 0 && tap_coord(200, 96) == 95 && staged_off<2>(0, 0, 2, 20u) == 0u && staged_off<2>(95, 0, 2, 20u) == 20u * 512u + (7u << 6));

    // a clamp-only scene: NaN and +-1e30 offsets in the second stream of a volume
    {
        Scene s;
        for (int a = 0; a < 3; ++a) { s.data[a] = 17; s.lv[a] = 9; s.off[0][a] = 0.0f; s.off[1][a] = a == 0 ? kNaN : (a == 1 ? 1e30f : -1e30f); }
        s.ns = 2; s.dir = 1; s.esz = 1;
        long a = 0, b = 0, c = 0;
        check_units(s, a, b, c);
        for (int axis = 0; axis < 3; ++axis) check_signature(s, axis);
    }

    // factor_block on both sides of cap, and with cap = 0
    {
        static float keep[4 * kOccBlockFloats], spill[4 * kOccBlockFloats];
        static_assert(kOccBlockFloats == 2048 && kOccSliceFloats == 256, "a factor block is 8 slices of 16 x 16 floats");
        CHECK(factor_block(keep, spill, 3u, 0u) == keep);
        CHECK(factor_block(keep, spill, 3u, 2u) == keep + 2 * 2048);
        CHECK(factor_block(keep, spill, 3u, 3u) == spill);
        CHECK(factor_block(keep, spill, 3u, 5u) == spill + 2 * 2048);
        CHECK(factor_block(keep, spill, 0u, 0u) == spill);
        CHECK(factor_block(keep, spill, 0u, 3u) == spill + 3 * 2048);
        CHECK(factor_block((const float*) keep, (const float*) spill, 1u, 1u) == spill);
    }
    // the LDS estimate: same resolution 3 x 3 x 2 bricks, half resolution 5 x 5 x 3
    {
        const int d[3] = {96, 80, 144}, same[3] = {96, 80, 144}, half[3] = {48, 40, 72};
        CHECK(occ_lds_estimate(d, same, 2, 4) == (size_t) 3 * 3 * 2 * 2048);
        CHECK(occ_lds_estimate(d, half, 2, 4) == (size_t) 5 * 5 * 3 * 2048);
        CHECK(occ_lds_estimate(d, half, 0, 1) == (size_t) 3 * 5 * 5 * 512);
    }
    std::printf("checks=%ld staged_units=%ld unstaged_units=%ld edge_units=%ld\n", checks, staged_units, unstaged_units, edge_units);
    std::printf("failures=%d\n", failures);
    return failures ? 1 : 0;
}
