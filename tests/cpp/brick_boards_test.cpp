// The index rules of the label tools (tbraymarcherplugin_amd/csrc/tbrm_brick_boards.h) and the host's box rule (tbrm_box.h) on their
// own, each against the voxel-by-voxel answer: the box of a call and its refusals, the bricks a box touches, the row and slice masks on
// ragged edge bricks and clipped rows, range positions, the byte helpers, the in-slice spread of a dilation, bounding box to bricks.
// Pure host code, no device; tests/test_brick_boards.py builds it with -fsanitize=address,undefined and runs it. Prints "failures=N"
// last.
#include "../../tbraymarcherplugin_amd/csrc/tbrm_brick_boards.h"
#include "../../tbraymarcherplugin_amd/csrc/tbrm_box.h"

#include <climits>
#include <cstdio>
#include <set>
#include <tuple>

using namespace tbrm;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++failures <= 20) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
        }                                                                  \
    } while (0)

static const int kWidths[5] = {1, 7, 8, 9, 17}; // one ragged brick, one short of a brick, a brick, one over, two bricks and one
struct Pair { uint32_t x, y; };                 // the 8 bytes of a row, as uint2 holds them

static int bricks_of(int width) { return (width + 7) / 8; }

static bool refused(const int dims[3], const int32_t o[3], const int32_t e[3], bool zero_is_whole, int what, int axis)
{
    VoxelBox box;
    BrickRange range;
    for (int c = 0; c < 3; ++c) { box.origin[c] = box.end[c] = -7; range.b0[c] = range.nb[c] = -7; }
    const BoxVerdict v = box_resolve(dims, o, e, zero_is_whole, &box, &range);
    for (int c = 0; c < 3; ++c) CHECK(box.origin[c] == -7 && box.end[c] == -7 && range.b0[c] == -7 && range.nb[c] == -7); // left alone
    return v.what == what && v.axis == axis;
}

// every mask of a box in a volume against the voxel-by-voxel answer, over every brick of the grid
static void check_masks(const int dims[3], const VoxelBox& box, const BrickRange& range)
{
    std::set<std::tuple<int, int, int>> touched;
    for (int bz = 0; bz < bricks_of(dims[2]); ++bz)
        for (int by = 0; by < bricks_of(dims[1]); ++by)
            for (int bx = 0; bx < bricks_of(dims[0]); ++bx)
                for (int z = bz * 8; z < bz * 8 + 8; ++z) {
                    uint64_t slice = 0;
                    for (int y = by * 8; y < by * 8 + 8; ++y) {
                        uint32_t in_box = 0, in_vol = 0;
                        for (int i = 0; i < 8; ++i) {
                            const int x = bx * 8 + i;
                            const bool vol = x < dims[0] && y < dims[1] && z < dims[2];
                            const bool in = x >= box.origin[0] && x < box.end[0] && y >= box.origin[1] && y < box.end[1] && z >= box.origin[2] && z < box.end[2];
                            in_vol |= (uint32_t) vol << i;
                            in_box |= (uint32_t) in << i;
                            if (in) touched.insert(std::make_tuple(bx, by, bz));
                        }
                        CHECK(row_in_box(box, bx, y, z) == in_box);
                        CHECK(row_in_volume(dims, bx, y, z) == in_vol);
                        slice |= (uint64_t) in_vol << (8 * (y & 7));
                    }
                    CHECK(slice_in_volume(dims, bx, by, z) == slice);
                }
    // the range is the set of bricks that hold a voxel of the box, and its positions round-trip
    CHECK(range_bricks(range) == touched.size());
    std::set<std::tuple<int, int, int>> listed;
    for (uint32_t k = 0; k < (uint32_t) range_bricks(range); ++k) {
        int bx, by, bz;
        range_brick(range, k, bx, by, bz);
        CHECK(touched.count(std::make_tuple(bx, by, bz)) == 1);
        CHECK(range_holds(range, bx, by, bz) && range_position(range, bx, by, bz) == k);
        listed.insert(std::make_tuple(bx, by, bz));
    }
    CHECK(listed == touched);
    // "inside the range" for the 26 neighbours of the corner bricks (and the corners themselves)
    for (int corner = 0; corner < 8; ++corner) {
        int b[3];
        for (int c = 0; c < 3; ++c) b[c] = ((corner >> c) & 1) ? range.b0[c] + range.nb[c] - 1 : range.b0[c];
        for (int n = 0; n < 27; ++n) {
            const int bx = b[0] + n % 3 - 1, by = b[1] + (n / 3) % 3 - 1, bz = b[2] + n / 9 - 1;
            CHECK(range_holds(range, bx, by, bz) == (touched.count(std::make_tuple(bx, by, bz)) == 1));
        }
    }
}

// the bit (x, y) of a slice word's spread: some set bit within one step (6: along one axis; 26: along both)
static uint64_t spread_by_bits(uint64_t w, bool conn26)
{
    uint64_t out = 0;
    for (int y = 0; y < 8; ++y)
        for (int x = 0; x < 8; ++x) {
            bool any = false;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!conn26 && dx != 0 && dy != 0) continue;
                    const int xx = x + dx, yy = y + dy;
                    if (xx < 0 || xx > 7 || yy < 0 || yy > 7) continue;
                    any = any || ((w >> (yy * 8 + xx)) & 1ull);
                }
            out |= (uint64_t) any << (y * 8 + x);
        }
    return out;
}

int main()
{
    // ---- the box rule, the range and the masks: every box along one axis, the other two axes fixed at a small ragged box --------------
    for (int axis = 0; axis < 3; ++axis)
        for (int width : kWidths) {
            int dims[3] = {9, 7, 17};
            int32_t o[3] = {1, 2, 5}, e[3] = {8, 4, 6}; // (x crosses a brick face, y stays inside a brick, z ends one short of a face)
            dims[axis] = width;
            for (int oo = 0; oo < width; ++oo)
                for (int ee = 1; ee <= width - oo; ++ee) {
                    o[axis] = oo;
                    e[axis] = ee;
                    VoxelBox box;
                    BrickRange range;
                    const BoxVerdict v = box_resolve(dims, o, e, true, &box, &range);
                    CHECK(v.what == BOX_OK);
                    for (int c = 0; c < 3; ++c) CHECK(box.origin[c] == o[c] && box.end[c] == o[c] + e[c]);
                    check_masks(dims, box, range);
                    VoxelBox same;
                    CHECK(box_resolve(dims, o, e, false, &same, nullptr).what == BOX_OK && same.origin[axis] == oo && same.end[axis] == oo + ee);
                    CHECK(box_resolve(nullptr, o, e, false, nullptr, nullptr).what == BOX_OK); // (no volume known: nothing to leave)
                }
            // the refusals, along this axis
            o[axis] = 0; e[axis] = 0;            CHECK(refused(dims, o, e, true, BOX_EMPTY, axis));  // one extent 0 is not the whole volume
            e[axis] = -1;                        CHECK(refused(dims, o, e, true, BOX_EMPTY, axis));
            e[axis] = INT_MIN;                   CHECK(refused(dims, o, e, false, BOX_EMPTY, axis));
            e[axis] = 1; o[axis] = -1;           CHECK(refused(dims, o, e, true, BOX_LEAVES, axis));
            CHECK(refused(nullptr, o, e, false, BOX_LEAVES, axis));                                   // (no volume holds a negative origin)
            o[axis] = INT_MIN;                   CHECK(refused(dims, o, e, true, BOX_LEAVES, axis));
            o[axis] = width;                     CHECK(refused(dims, o, e, true, BOX_LEAVES, axis));
            o[axis] = 0; e[axis] = width + 1;    CHECK(refused(dims, o, e, true, BOX_LEAVES, axis));
            o[axis] = width - 1; e[axis] = 2;    CHECK(refused(dims, o, e, true, BOX_LEAVES, axis));
            o[axis] = INT_MAX; e[axis] = INT_MAX; CHECK(refused(dims, o, e, true, BOX_LEAVES, axis)); // (no overflow on the way)
            CHECK(refused(nullptr, o, e, false, BOX_LEAVES, axis));
            o[axis] = 1; e[axis] = INT_MAX;      CHECK(refused(nullptr, o, e, false, BOX_LEAVES, axis));
            const int32_t zero[3] = {0, 0, 0};
            CHECK(refused(dims, o, zero, false, BOX_EMPTY, 0)); // all-zero is the whole volume only where the call says so
            CHECK(refused(nullptr, o, zero, true, BOX_EMPTY, 0));
        }

    // ---- the whole-volume form and the in-volume masks, every combination of the widths -------------------------------------------
    for (int wx : kWidths)
        for (int wy : kWidths)
            for (int wz : kWidths) {
                const int dims[3] = {wx, wy, wz};
                const int32_t off[3] = {5, -6, INT_MAX}, zero[3] = {0, 0, 0}; // the origin is ignored with an all-zero extent
                VoxelBox box, none;
                BrickRange range, grid;
                CHECK(box_resolve(dims, off, zero, true, &box, &range).what == BOX_OK);
                CHECK(box_resolve(dims, nullptr, nullptr, true, &none, &grid).what == BOX_OK); // no box at all
                for (int c = 0; c < 3; ++c) {
                    CHECK(box.origin[c] == 0 && box.end[c] == dims[c] && range.b0[c] == 0 && range.nb[c] == bricks_of(dims[c]));
                    CHECK(none.origin[c] == 0 && none.end[c] == dims[c] && grid.b0[c] == 0 && grid.nb[c] == bricks_of(dims[c]));
                }
                check_masks(dims, box, range);
                // the grid index is the position in the whole grid's range
                for (uint32_t k = 0; k < (uint32_t) range_bricks(range); ++k) {
                    int bx, by, bz;
                    range_brick(range, k, bx, by, bz);
                    CHECK(grid_index(range.nb[0], range.nb[0] * range.nb[1], bx, by, bz) == k);
                }
                // a one-voxel box in the far corner
                const int32_t o[3] = {wx - 1, wy - 1, wz - 1}, one[3] = {1, 1, 1};
                CHECK(box_resolve(dims, o, one, true, &box, &range).what == BOX_OK);
                check_masks(dims, box, range);
            }

    // ---- the bytes of a row ------------------------------------------------------------------------------------------------------------
    for (uint32_t label = 0; label < 256; ++label)
        for (int i = 0; i < 8; ++i) {
            const Pair base = {0x03020100u + 0x10101010u * (label & 7), 0xf7f6f5f4u - 0x01010101u * (label & 3)};
            Pair v = base;
            set_byte(v, i, label);
            uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            mask[label >> 5] = 1u << (label & 31); // the mask that holds this label alone
            uint32_t want = 0;
            for (int j = 0; j < 8; ++j) {
                const uint32_t was = ((j < 4 ? base.x : base.y) >> (8 * (j & 3))) & 255u; // (spelled out: not byte_of)
                CHECK(byte_of(base, j) == was);
                CHECK(byte_of(v, j) == (j == i ? label : was));
                want |= (uint32_t) ((j == i ? label : was) == label) << j;
            }
            CHECK(row_in_mask(v, mask) == want && ((want >> i) & 1u));
            for (int w = 0; w < 8; ++w) mask[w] = ~mask[w]; // every label but this one
            CHECK(row_in_mask(v, mask) == (~want & 0xffu));
        }

    // ---- the in-slice spread -----------------------------------------------------------------------------------------------------------
    for (int bit = 0; bit < 64; ++bit) {
        CHECK(slice_spread<0>(1ull << bit) == spread_by_bits(1ull << bit, false));
        CHECK(slice_spread<1>(1ull << bit) == spread_by_bits(1ull << bit, true));
    }
    uint64_t state = 0x9e3779b97f4a7c15ull;
    for (int n = 0; n < 300; ++n) {
        state = state * 6364136223846793005ull + 1442695040888963407ull; // (Knuth's MMIX LCG)
        uint64_t w = state;
        if (n % 3 == 1) w &= state >> 17 & state << 11; // sparse words as well as dense ones
        if (n % 3 == 2) w |= state >> 23;
        CHECK(slice_spread<0>(w) == spread_by_bits(w, false));
        CHECK(slice_spread<1>(w) == spread_by_bits(w, true));
    }
    CHECK(slice_spread<0>(0ull) == 0ull && slice_spread<1>(0ull) == 0ull && slice_spread<0>(~0ull) == ~0ull && slice_spread<1>(~0ull) == ~0ull);

    // ---- a bounding box to bricks ------------------------------------------------------------------------------------------------------
    for (int lo = 0; lo < 26; ++lo)
        for (int hi = lo; hi < 26; ++hi) {
            const int32_t mn[3] = {lo, 0, hi}, mx[3] = {hi, lo, 25};
            int b0[3], b1[3];
            bbox_bricks(mn, mx, b0, b1);
            for (int c = 0; c < 3; ++c)
                for (int b = 0; b < 5; ++b) { // brick b is in [b0, b1) exactly when it holds a voxel of [mn, mx]
                    bool holds = false;
                    for (int x = b * 8; x < b * 8 + 8; ++x) holds = holds || (x >= mn[c] && x <= mx[c]);
                    CHECK((b >= b0[c] && b < b1[c]) == holds);
                }
        }

    // ---- the class of a board, a range of stored values ---------------------------------------------------------------------------------
    CHECK(board_class(false, false) == MORPH_EMPTY && board_class(false, true) == MORPH_EMPTY); // (no bit: empty even where no bit is in the volume)
    CHECK(board_class(true, true) == MORPH_FULL && board_class(true, false) == MORPH_MIXED);
    const double nan = std::nan(""), inf = HUGE_VAL;
    CHECK(value_range_refusal(3, 3, false, 0, 255) == RANGE_OK && value_range_refusal(0, 255, false, 0, 255) == RANGE_OK);
    CHECK(value_range_refusal(4, 3, false, 0, 255) == RANGE_ORDER && value_range_refusal(nan, 3, false, 0, 255) == RANGE_ORDER && value_range_refusal(3, nan, true, 0, 0) == RANGE_ORDER);
    CHECK(value_range_refusal(-1, 3, false, 0, 255) == RANGE_CODES && value_range_refusal(0, 256, false, 0, 255) == RANGE_CODES && value_range_refusal(1.5, 3, false, 0, 255) == RANGE_CODES);
    CHECK(value_range_refusal(-255, 0, false, -255, 255) == RANGE_OK && value_range_refusal(-256, 0, false, -255, 255) == RANGE_CODES);
    CHECK(value_range_refusal(-inf, inf, false, 0, 65535) == RANGE_CODES && value_range_refusal(0, inf, true, 0, 0) == RANGE_FLOAT && value_range_refusal(-inf, 0, true, 0, 0) == RANGE_FLOAT);
    CHECK(value_range_refusal(-1e30, 1e30, true, 0, 0) == RANGE_OK && value_range_refusal(0, 1e39, true, 0, 0) == RANGE_FLOAT && value_range_refusal(-1.5, 2.25, true, 0, 0) == RANGE_OK);

    std::printf("failures=%d\n", failures);
    return failures != 0;
}
