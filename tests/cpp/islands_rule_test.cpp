// The rule of tbrm_label_islands and the validation of its arguments (tbraymarcherplugin_amd/csrc/tbrm_islands_rule.h) on their own:
// kept / dropped and the label per position and size for the four tools, the sort key's order, and every refusal of the header's
// error table that needs no handle. Pure host code, no device; tests/test_islands_abi.py builds it with
// -fsanitize=address,undefined and runs it. Prints "failures=N" last.
#include "../../tbraymarcherplugin_amd/csrc/tbrm_islands_rule.h"

#include <algorithm>
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

struct Args {
    int dims[3] = {40, 24, 19};
    int32_t origin[3] = {0, 0, 0}, extent[3] = {0, 0, 0};
    int connectivity = 6, max_islands = 0, keep_label = -1, label_step = 0, drop_label = 0, spare_border = 0;
    uint32_t flags = 0, reserved = 0;
};
static const char* validate(const Args& a, int o[3], int e[3])
{
    return islands_validate(a.dims, a.origin, a.extent, a.connectivity, a.max_islands, a.keep_label, a.label_step, a.drop_label, a.spare_border, a.flags,
                            a.reserved, o, e);
}
static bool refused(const Args& a)
{
    int o[3] = {-7, -7, -7}, e[3] = {-7, -7, -7};
    const char* what = validate(a, o, e);
    for (int c = 0; c < 3; ++c) CHECK(what == nullptr || (o[c] == -7 && e[c] == -7)); // a refusal leaves the box alone
    return what != nullptr;
}

int main()
{
    { // keep the largest n: positions below n are kept and left, the others get the erase label
        const IslandsRule r{0, 3, -1, 0, 0};
        for (uint64_t pos = 0; pos < 10; ++pos) {
            CHECK(islands_kept(r, pos, 1) == (pos < 3));
            CHECK(islands_label(r, pos, 1) == (pos < 3 ? kIslandsLeave : 0));
        }
    }
    { // remove the small: no limit by position, by size alone
        const IslandsRule r{5, 0, -1, 0, 9};
        for (uint64_t size = 1; size < 10; ++size) {
            CHECK(islands_kept(r, 1000000, size) == (size >= 5));
            CHECK(islands_label(r, 1000000, size) == (size >= 5 ? kIslandsLeave : 9));
        }
        CHECK(islands_kept(r, (uint64_t) INT_MAX + 5, 5)); // positions beyond int
    }
    { // split: keep_label + position; the last label is 255
        const IslandsRule r{0, 6, 250, 1, -1};
        for (uint64_t pos = 0; pos < 9; ++pos) CHECK(islands_label(r, pos, 7) == (pos < 6 ? 250 + (int) pos : kIslandsLeave));
        const IslandsRule both{3, 6, 250, 1, 4}; // position and size together
        CHECK(islands_label(both, 2, 3) == 252 && islands_label(both, 2, 2) == 4 && islands_label(both, 6, 100) == 4);
    }
    { // fill holes: nothing reaches UINT64_MAX voxels, so everything ordered is dropped; up to n voxels: min_voxels = n + 1
        const IslandsRule any{UINT64_MAX, 0, -1, 0, 2};
        CHECK(!islands_kept(any, 0, 1) && !islands_kept(any, 0, 0xffffffffull) && islands_label(any, 0, 0xffffffffull) == 2);
        const IslandsRule upto{4 + 1, 0, -1, 0, 2};
        CHECK(islands_label(upto, 0, 4) == 2 && islands_label(upto, 0, 5) == kIslandsLeave);
    }
    { // the key: size descending, equal sizes by first voxel ascending; both ends of the 32-bit ranges
        struct Island { uint32_t size, first; };
        std::vector<Island> islands = {{1, 7}, {0xffffffffu, 0xffffffffu}, {5, 3}, {5, 2}, {1, 0}, {0xffffffffu, 0}, {2, 0xffffffffu}, {5, 0xfffffffeu}};
        std::vector<uint64_t> keys;
        for (const Island& i : islands) {
            const uint64_t k = islands_key(i.size, i.first);
            CHECK(islands_key_size(k) == i.size && islands_key_first(k) == i.first);
            keys.push_back(k);
        }
        std::sort(keys.begin(), keys.end());
        std::sort(islands.begin(), islands.end(), [](const Island& a, const Island& b) { return a.size != b.size ? a.size > b.size : a.first < b.first; });
        for (size_t i = 0; i < keys.size(); ++i) CHECK(islands_key_size(keys[i]) == islands[i].size && islands_key_first(keys[i]) == islands[i].first);
        for (size_t i = 1; i < keys.size(); ++i) CHECK(keys[i - 1] < keys[i]);
    }
    { // validation: what passes and the box it gives
        Args a;
        int o[3], e[3];
        CHECK(validate(a, o, e) == nullptr && o[0] == 0 && o[1] == 0 && o[2] == 0 && e[0] == 40 && e[1] == 24 && e[2] == 19);
        a.origin[0] = 5; a.origin[1] = 6; a.origin[2] = 7; // ignored with an all-zero extent
        CHECK(validate(a, o, e) == nullptr && o[0] == 0 && e[2] == 19);
        a.extent[0] = 35; a.extent[1] = 18; a.extent[2] = 12; // up to the far faces
        CHECK(validate(a, o, e) == nullptr && o[0] == 5 && o[1] == 6 && o[2] == 7 && e[0] == 40 && e[1] == 24 && e[2] == 19);
        Args s;
        s.keep_label = 0; s.label_step = 1; s.max_islands = 256; s.connectivity = 26; s.drop_label = -1; s.spare_border = 1; s.flags = kIslandsMeasure;
        CHECK(validate(s, o, e) == nullptr);
        s.keep_label = 255; s.max_islands = 1;
        CHECK(validate(s, o, e) == nullptr);
    }
    { // validation: the refusals
        Args a;
        a.connectivity = 18; CHECK(refused(a)); a.connectivity = 0; CHECK(refused(a)); a = Args();
        a.max_islands = -1; CHECK(refused(a)); a.max_islands = INT_MIN; CHECK(refused(a)); a = Args();
        a.keep_label = 256; CHECK(refused(a)); a.keep_label = -2; CHECK(refused(a)); a = Args();
        a.drop_label = 256; CHECK(refused(a)); a.drop_label = -2; CHECK(refused(a)); a = Args();
        a.label_step = 2; CHECK(refused(a)); a.label_step = -1; CHECK(refused(a)); a = Args();
        a.label_step = 1; a.keep_label = 3; a.max_islands = 0; CHECK(refused(a));       // a step needs a limit
        a.max_islands = 254; CHECK(refused(a)); a.max_islands = 253; CHECK(!refused(a)); // 3 + 253 - 1 = 255
        a.max_islands = INT_MAX; CHECK(refused(a));                                       // (no overflow on the way)
        a.keep_label = -1; a.max_islands = 2; CHECK(refused(a)); a = Args();              // a step needs a first label
        a.spare_border = 2; CHECK(refused(a)); a.spare_border = -1; CHECK(refused(a)); a = Args();
        a.flags = 2; CHECK(refused(a)); a.flags = 0x80000001u; CHECK(refused(a)); a = Args();
        a.reserved = 1; CHECK(refused(a)); a = Args();
        a.extent[0] = 1; CHECK(refused(a));                                               // one axis empty
        a.extent[1] = 1; a.extent[2] = 1; CHECK(!refused(a));
        a.origin[0] = 40; CHECK(refused(a)); a.origin[0] = -1; CHECK(refused(a)); a.origin[0] = 39; CHECK(!refused(a));
        a.extent[0] = 2; CHECK(refused(a)); a.extent[0] = INT_MAX; a.origin[0] = INT_MAX; CHECK(refused(a)); a.extent[0] = -3; a.origin[0] = 3; CHECK(refused(a));
        a = Args();
        a.dims[1] = 0; CHECK(refused(a));
        int o[3], e[3];
        CHECK(islands_validate(nullptr, a.origin, a.extent, 6, 0, -1, 0, 0, 0, 0, 0, o, e) != nullptr);
        CHECK(islands_validate(a.dims, a.origin, a.extent, 6, 0, -1, 0, 0, 0, 0, 0, nullptr, e) != nullptr);
    }
    std::printf("failures=%d\n", failures);
    return failures != 0;
}
