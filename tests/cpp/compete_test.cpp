// Drives ARaymarchVolume::GrowFromSeeds (include/tbrm_plugin.hpp, include/tbrm_compete.h): two painted balls in a two-phase MetaImage
// volume compete for the rest of it; the label volume, the costs and the counts are compared with a restatement below — a heap
// Dijkstra over packed keys on the stored codes as the handle gives them back. The calls request no recompute and count as no frame.
// "nohandle": what an actor without resources answers (no device needed). Otherwise argv[1] is a directory to write the volume to.
// Prints one "key value" line per check; tests/test_compete_facade.py compiles it with g++ and runs it.
#include "tbrm_volume_io.hpp" // includes tbrm_plugin.hpp

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <queue>
#include <string>
#include <utility>
#include <vector>

using namespace tbrm_plugin;

static const int nx = 40, ny = 20, nz = 19;
static size_t at(int x, int y, int z) { return ((size_t) z * ny + y) * nx + x; }

// keys by Dijkstra: seeds are the voxels labelled 1 or 2, every other voxel is claimable
static std::vector<uint32_t> keys_by_dijkstra(const std::vector<uint16_t>& code, const std::vector<uint8_t>& labels, const int step[3], int shift, uint32_t limit)
{
    std::vector<uint32_t> key(code.size(), 0xFFFFFFFFu);
    typedef std::pair<uint32_t, uint32_t> Item;
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    for (size_t i = 0; i < labels.size(); ++i)
        if (labels[i] == 1 || labels[i] == 2) { key[i] = labels[i]; heap.push(Item(key[i], (uint32_t) i)); }
    const int stride[3] = {1, nx, nx * ny}, size[3] = {nx, ny, nz};
    while (!heap.empty()) {
        const Item top = heap.top();
        heap.pop();
        if (top.first != key[top.second]) continue;
        const int i = (int) top.second, pos[3] = {i % nx, (i / nx) % ny, i / (nx * ny)};
        for (int a = 0; a < 3; ++a)
            for (int d = -1; d <= 1; d += 2) {
                if (pos[a] + d < 0 || pos[a] + d >= size[a]) continue;
                const int j = i + d * stride[a];
                if (labels[j] == 1 || labels[j] == 2) continue;
                const int diff = (int) code[i] - (int) code[j];
                const uint64_t cost = (uint64_t) (top.first >> 8) + (uint64_t) step[a] + (uint64_t) ((diff < 0 ? -diff : diff) >> shift);
                if (cost > limit) continue;
                const uint32_t offer = (uint32_t) (cost << 8) | (top.first & 255u);
                if (offer < key[j]) { key[j] = offer; heap.push(Item(offer, (uint32_t) j)); }
            }
    }
    return key;
}

int main(int argc, char** argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "nohandle")) {
        ARaymarchVolume none;
        FCompeteResult m;
        const bool a = none.GrowFromSeeds({1, 2}, FCompeteOptions{}, m);
        int unit[3], aniso[3];
        none.StepCostFromSpacing(16, unit);
        none.VoxelSpacing[0] = 0.7; none.VoxelSpacing[1] = 0.7; none.VoxelSpacing[2] = 2.5;
        none.StepCostFromSpacing(16, aniso);
        std::printf("nohandle grow=%d claimed=%llu recompute=%d abi=%d unit=%d,%d,%d aniso=%d,%d,%d\n", a ? 1 : 0, (unsigned long long) m.Claimed, none.bRequestedRecompute ? 1 : 0,
                    tbrm_compete_abi_version(), unit[0], unit[1], unit[2], aniso[0], aniso[1], aniso[2]);
        return 0;
    }
    if (argc < 2) { std::printf("error: a directory to write the volume to\n"); return 1; }

    // two phases that meet in an oblique plane, with a ripple; a ball of label 1 in one, of label 2 in the other, both off the plane
    std::vector<uint16_t> vol((size_t) nx * ny * nz);
    std::vector<uint8_t> labels(vol.size(), 0);
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const bool dense = 2 * x + y + z > 58;
                vol[at(x, y, z)] = (uint16_t) ((dense ? 50000 : 12000) + 31 * ((x * 7 + y * 3 + z * 5) % 13));
                const int a = (x - 8) * (x - 8) + (y - 9) * (y - 9) + (z - 9) * (z - 9), b = (x - 31) * (x - 31) + (y - 10) * (y - 10) + (z - 8) * (z - 8);
                labels[at(x, y, z)] = a <= 9 ? 1 : (b <= 9 ? 2 : 0);
            }
    const std::string dir = argv[1];
    {
        FILE* raw = std::fopen((dir + "/phases.raw").c_str(), "wb");
        FILE* mhd = std::fopen((dir + "/phases.mhd").c_str(), "w");
        if (!raw || !mhd) { std::printf("error: cannot write to %s\n", dir.c_str()); return 1; }
        std::fwrite(vol.data(), sizeof(uint16_t), vol.size(), raw);
        std::fprintf(mhd, "ObjectType = Image\nNDims = 3\nDimSize = %d %d %d\nElementSpacing = 1 1 2.5\nElementType = MET_USHORT\nElementDataFile = phases.raw\n", nx, ny, nz);
        std::fclose(raw);
        std::fclose(mhd);
    }
    ARaymarchLight l0;
    l0.ForwardVector = FVector{1, .35, -.5}; l0.LightIntensity = 0.5f;
    ARaymarchVolume a;
    a.LightsArray = {&l0};
    if (!LoadMHDFileIntoVolumeNormalized(a, dir + "/phases.mhd")) { std::printf("error %s\n", tbrm_last_error()); return 2; }
    a.Tick(0.016f);
    FCompeteResult m;
    std::printf("nolabels refused=%d\n", a.GrowFromSeeds({1, 2}, FCompeteOptions{}, m) ? 0 : 1); // no label volume yet
    if (!a.SetLabelVolume(labels.data(), labels.size())) { std::printf("error %s\n", tbrm_last_error()); return 3; }
    const int frames = a.Stats.Frames, resets = a.Stats.Resets;

    // the codes as stored
    std::vector<uint16_t> code(vol.size());
    const int32_t origin[3] = {0, 0, 0}, extent[3] = {nx, ny, nz};
    if (tbrm_download_volume_region(a.RaymarchResources.Handle, origin, extent, code.data(), code.size() * sizeof(uint16_t)) != TBRM_OK) { std::printf("error %s\n", tbrm_last_error()); return 4; }

    FCompeteOptions opt;
    opt.SpacingCost = 8;    // spacing 1 : 1 : 2.5 -> 8, 8, 20
    opt.ValueShift = 4;
    const int step[3] = {8, 8, 20};
    struct Call { const char* name; uint32_t limit; bool measure; };
    const Call calls[] = {{"measure", 0u, true}, {"limited", 900u, false}, {"whole", 0u, false}};
    std::vector<uint8_t> want = labels, got(labels.size());
    for (const Call& c : calls) {
        opt.CostLimit = c.limit;
        opt.bMeasureOnly = c.measure;
        const std::vector<uint32_t> key = keys_by_dijkstra(code, want, step, 4, c.limit ? c.limit : 0xFFFFFFu);
        uint64_t claimed = 0, relabelled = 0, per[3] = {0, 0, 0}, seeds = 0;
        uint32_t top = 0;
        std::vector<uint32_t> cost_want(key.size());
        std::vector<uint8_t> next = want;
        for (size_t i = 0; i < key.size(); ++i) {
            const bool seed = want[i] == 1 || want[i] == 2;
            seeds += seed;
            cost_want[i] = seed ? 0u : (key[i] == 0xFFFFFFFFu ? 0xFFFFFFFFu : key[i] >> 8);
            if (seed || key[i] == 0xFFFFFFFFu) continue;
            ++claimed;
            ++per[key[i] & 255u];
            if ((key[i] >> 8) > top) top = key[i] >> 8;
            if (!c.measure) { relabelled += want[i] != (key[i] & 255u); next[i] = (uint8_t) (key[i] & 255u); }
        }
        std::vector<uint32_t> costs;
        if (!a.GrowFromSeeds({1, 2}, opt, m, &costs)) { std::printf("error %s\n", tbrm_last_error()); return 5; }
        if (tbrm_download_label_volume(a.RaymarchResources.Handle, got.data(), got.size()) != TBRM_OK) { std::printf("error %s\n", tbrm_last_error()); return 6; }
        size_t wrong = 0, wrong_costs = costs.size() == cost_want.size() ? 0 : 1;
        for (size_t i = 0; i < got.size(); ++i) wrong += got[i] != next[i];
        for (size_t i = 0; i < costs.size() && i < cost_want.size(); ++i) wrong_costs += costs[i] != cost_want[i];
        // the split: in the unlimited call every voxel is claimed, and both labels took a share
        std::printf("%s wrong=%zu costs=%zu counts=%d both=%d steps=%d,%d,%d\n", c.name, wrong, wrong_costs,
                    (m.SeedVoxels == seeds && m.Claimable == want.size() - seeds && m.Claimed == claimed && m.Relabelled == relabelled && m.ClaimedPerLabel[1] == per[1] &&
                     m.ClaimedPerLabel[2] == per[2] && m.MaxCost == top && m.Passes >= 1) ? 1 : 0,
                    (per[1] > 0 && per[2] > 0 && (c.limit != 0 || claimed == want.size() - seeds) && (c.limit == 0 || claimed < want.size() - seeds)) ? 1 : 0,
                    m.StepCost[0], m.StepCost[1], m.StepCost[2]);
        want = next;
    }
    // where the phases meet: of the voxels of the dense phase label 2's share is the larger, of the other phase label 1's
    uint64_t dense2 = 0, dense = 0, thin1 = 0, thin = 0;
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const bool d = 2 * x + y + z > 58;
                dense += d; thin += !d;
                dense2 += d && got[at(x, y, z)] == 2;
                thin1 += !d && got[at(x, y, z)] == 1;
            }
    std::printf("split dense=%d thin=%d\n", dense2 * 10 > dense * 9 ? 1 : 0, thin1 * 10 > thin * 9 ? 1 : 0);
    // what no call can take
    FCompeteOptions bad = opt;
    bad.ValueShift = 17;
    const bool shift = a.GrowFromSeeds({1, 2}, bad, m);
    bad = opt;
    bad.StepCost[1] = 65536;
    const bool cost = a.GrowFromSeeds({1, 2}, bad, m);
    std::printf("refused none=%d label=%d shift=%d cost=%d\n", a.GrowFromSeeds({}, opt, m) ? 0 : 1, a.GrowFromSeeds({256}, opt, m) ? 0 : 1, shift ? 0 : 1, cost ? 0 : 1);
    std::printf("state frames=%d resets=%d recompute=%d\n", a.Stats.Frames - frames, a.Stats.Resets - resets, a.bRequestedRecompute ? 1 : 0);
    uint64_t c[4] = {0, 0, 0, 0};
    tbrm_compete_counters(a.RaymarchResources.Handle, c);
    std::printf("counters calls=%llu\n", (unsigned long long) c[0]);
    std::printf("OK\n");
    return 0;
}
