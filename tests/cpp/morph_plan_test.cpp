// The step plan of tbrm_morph_labels (tbraymarcherplugin_amd/csrc/tbrm_morph_plan.h) on its own: the reach, the brick range of the box
// grown by it and clamped to the volume, and the split of the steps into launches for every morph_steps. Pure host code, no device;
// tests/test_morph_abi.py builds it with -fsanitize=address,undefined and runs it. Prints "failures=N" last.
#include "../../tbraymarcherplugin_amd/csrc/tbrm_morph_plan.h"

#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace tbrm;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
        }                                                                  \
    } while (0)

// the brick range by counting: the bricks that hold a voxel within `reach` of the box (Chebyshev, per axis), inside the volume
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
    const int volumes[][3] = {{40, 24, 19}, {24, 17, 10}, {5, 6, 3}, {16, 16, 16}, {40, 40, 40}, {512, 512, 512}, {1, 1, 1}, {9, 8, 7}};
    const int boxes[][6] = {{11, 5, 3, 13, 9, 7}, {17, 9, 4, 1, 1, 1}, {8, 8, 8, 8, 8, 8}, {0, 0, 0, 1, 1, 1}};
    for (const auto& dims : volumes)
        for (int whole = 0; whole < 2; ++whole)
            for (const auto& bx : boxes) {
                int origin[3], end[3];
                bool fits = true;
                for (int c = 0; c < 3; ++c) {
                    origin[c] = whole ? 0 : bx[c];
                    end[c] = whole ? dims[c] : bx[c] + bx[3 + c];
                    fits = fits && end[c] <= dims[c];
                }
                if (!fits) continue;
                for (int op = MORPH_DILATE; op <= MORPH_CLOSE; ++op)
                    for (int radius : {1, 2, 3, 7, 8, 9, 16, 17, 63, 64})
                        for (int per = 1; per <= 8; ++per) {
                            MorphPlan p;
                            std::memset(&p, 0xff, sizeof(p));
                            CHECK(morph_plan(dims, origin, end, op, radius, per, &p));
                            const bool two = op == MORPH_OPEN || op == MORPH_CLOSE;
                            CHECK(p.reach == (two ? 2 : 1) * radius);
                            const int per_kind = (radius + per - 1) / per;
                            CHECK(p.launches == per_kind * (two ? 2 : 1) && p.launches <= kMorphMaxLaunches);
                            int sum[2] = {0, 0};
                            for (int i = 0; i < p.launches; ++i) {
                                CHECK(p.steps[i] >= 1 && p.steps[i] <= per);
                                CHECK(p.erode[i] <= 1);
                                sum[p.erode[i]] += p.steps[i];
                                if (i > 0 && i != per_kind) CHECK(p.erode[i] == p.erode[i - 1]); // one change of kind at the most, between the sequences
                            }
                            CHECK(sum[0] == (op == MORPH_ERODE ? 0 : radius) && sum[1] == (op == MORPH_DILATE ? 0 : radius));
                            CHECK(p.erode[0] == (op == MORPH_ERODE || op == MORPH_OPEN));
                            if (two) CHECK(p.erode[p.launches - 1] != p.erode[0]);
                            for (int c = 0; c < 3; ++c) {
                                int b0, nb;
                                brick_range_by_counting(dims[c], origin[c], end[c], p.reach, b0, nb);
                                CHECK(p.b0[c] == b0 && p.nb[c] == nb);
                                CHECK(p.b0[c] >= 0 && (p.b0[c] + p.nb[c] - 1) * 8 < dims[c]); // every brick holds a voxel of the volume
                                brick_range_by_counting(dims[c], origin[c], end[c], 0, b0, nb);
                                CHECK(p.wb0[c] == b0 && p.wnb[c] == nb);
                                CHECK(p.wb0[c] >= p.b0[c] && p.wb0[c] + p.wnb[c] <= p.b0[c] + p.nb[c]);
                            }
                        }
            }
    { // morph_steps outside 1 .. 8 is clamped; arguments out of range give no plan and leave *out alone
        const int dims[3] = {40, 24, 19}, o[3] = {0, 0, 0}, e[3] = {40, 24, 19};
        MorphPlan p, q;
        CHECK(morph_plan(dims, o, e, MORPH_DILATE, 17, 0, &p) && p.launches == 17);
        CHECK(morph_plan(dims, o, e, MORPH_DILATE, 17, 100, &p) && p.launches == 3 && p.steps[0] == 8 && p.steps[1] == 8 && p.steps[2] == 1);
        CHECK(morph_plan(dims, o, e, MORPH_CLOSE, 64, 1, &p) && p.launches == 128 && p.erode[63] == 0 && p.erode[64] == 1);
        std::memset(&q, 0x5a, sizeof(q));
        const MorphPlan before = q;
        const int far[3] = {INT_MAX, INT_MAX, INT_MAX}, big[3] = {INT_MAX, INT_MAX, INT_MAX}, last[3] = {INT_MAX - 1, INT_MAX - 1, INT_MAX - 1};
        CHECK(!morph_plan(dims, o, e, 4, 1, 8, &q) && !morph_plan(dims, o, e, -1, 1, 8, &q));
        CHECK(!morph_plan(dims, o, e, MORPH_OPEN, 0, 8, &q) && !morph_plan(dims, o, e, MORPH_OPEN, 65, 8, &q));
        CHECK(!morph_plan(dims, o, far, MORPH_OPEN, 1, 8, &q) && !morph_plan(dims, e, e, MORPH_OPEN, 1, 8, &q));
        CHECK(!morph_plan(nullptr, o, e, MORPH_OPEN, 1, 8, &q) && !morph_plan(dims, o, e, MORPH_OPEN, 1, 8, nullptr));
        CHECK(std::memcmp(&q, &before, sizeof(q)) == 0);
        CHECK(morph_plan(big, last, far, MORPH_CLOSE, 64, 8, &q) && q.reach == 128); // the largest coordinates: no overflow on the way
        CHECK(q.b0[0] == (INT_MAX - 1 - 128) >> 3 && q.b0[0] + q.nb[0] - 1 == (INT_MAX - 1) >> 3);
    }
    std::printf("failures=%d\n", failures);
    return failures != 0;
}
