// Drives ARaymarchVolume::KeepLargestIslands / RemoveSmallIslands / SplitIslands / FillLabelHoles (include/tbrm_plugin.hpp,
// include/tbrm_islands.h): a block of one label with a cavity three voxels wide in it and specks of the same label around it —
// keep-largest removes the specks and nothing else, closing by radius 1 leaves the cavity open and fill-holes fills it, remove-small
// and split go by size; every label volume is compared with a brute-force restatement below (a flood fill per island). The calls
// request no recompute and count as no frame.
// "nohandle": what an actor without resources answers (no device needed).
// Prints one "key value" line per check; tests/test_islands_facade.py compiles it with g++ and runs it.
#include "tbrm_volume_io.hpp" // includes tbrm_plugin.hpp

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace tbrm_plugin;

static const int nx = 40, ny = 20, nz = 19;
static size_t at(int x, int y, int z) { return ((size_t) z * ny + y) * nx + x; }

struct Island { uint64_t size; size_t first; bool border; std::vector<size_t> voxels; };

// the 6-connected islands of a mask, ordered by size descending and first voxel ascending
static std::vector<Island> islands_of(const std::vector<uint8_t>& m)
{
    std::vector<uint8_t> seen(m.size(), 0);
    std::vector<Island> out;
    for (size_t s = 0; s < m.size(); ++s) {
        if (!m[s] || seen[s]) continue;
        Island isl{0, s, false, {}};
        std::vector<size_t> stack{s};
        seen[s] = 1;
        while (!stack.empty()) {
            const size_t v = stack.back();
            stack.pop_back();
            isl.voxels.push_back(v);
            const int x = (int) (v % nx), y = (int) ((v / nx) % ny), z = (int) (v / ((size_t) nx * ny));
            if (x == 0 || x == nx - 1 || y == 0 || y == ny - 1 || z == 0 || z == nz - 1) isl.border = true;
            const int d[6][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
            for (const auto& o : d) {
                const int X = x + o[0], Y = y + o[1], Z = z + o[2];
                if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) continue;
                const size_t n = at(X, Y, Z);
                if (m[n] && !seen[n]) { seen[n] = 1; stack.push_back(n); }
            }
        }
        isl.size = isl.voxels.size();
        out.push_back(std::move(isl));
    }
    std::sort(out.begin(), out.end(), [](const Island& a, const Island& b) { return a.size != b.size ? a.size > b.size : a.first < b.first; });
    return out;
}

static tbrm_camera example_camera(int width, int height) // examples/render_mhd.cpp's
{
    tbrm_camera cam{};
    cam.position = FVector{-145, -95, 80};
    const double fl = std::sqrt(145.0 * 145 + 95.0 * 95 + 80.0 * 80);
    cam.forward = FVector{145 / fl, 95 / fl, -80 / fl};
    const double rl = std::sqrt(cam.forward.x * cam.forward.x + cam.forward.y * cam.forward.y);
    cam.right = FVector{cam.forward.y / rl, -cam.forward.x / rl, 0};
    cam.up = FVector{cam.right.y * cam.forward.z - cam.right.z * cam.forward.y, cam.right.z * cam.forward.x - cam.right.x * cam.forward.z,
        cam.right.x * cam.forward.y - cam.right.y * cam.forward.x};
    cam.tan_half_fov_y = std::tan(25.0 * 3.14159265358979323846 / 180.0);
    cam.tan_half_fov_x = cam.tan_half_fov_y * width / height;
    cam.width = width;
    cam.height = height;
    return cam;
}

int main(int argc, char** argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "nohandle")) {
        ARaymarchVolume none;
        FIslandsResult r;
        const bool a = none.KeepLargestIslands(1, 1, r), b = none.RemoveSmallIslands(1, 5, r), c = none.SplitIslands(1, 2, 3, r), d = none.FillLabelHoles(1, r);
        std::printf("nohandle keep=%d remove=%d split=%d fill=%d islands=%llu recompute=%d abi=%d\n", a ? 1 : 0, b ? 1 : 0, c ? 1 : 0, d ? 1 : 0,
                    (unsigned long long) r.Islands, none.bRequestedRecompute ? 1 : 0, tbrm_islands_abi_version());
        return 0;
    }

    const int W = 48, H = 40, L = 3;
    std::vector<uint16_t> vol((size_t) nx * ny * nz);
    std::vector<uint8_t> labels(vol.size(), 0);
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const bool block = x >= 4 && x < 30 && y >= 4 && y < 16 && z >= 4 && z < 15;
                const bool cavity = x >= 10 && x < 13 && y >= 9 && y < 12 && z >= 8 && z < 11;         // 3 x 3 x 3 inside the block
                const bool speck = x >= 32 && (x % 3 == 0) && (y % 4 == 1) && (z % 5 == 2);             // single voxels beside it
                const bool pair = x == 34 && (y == 10 || y == 11) && z == 9;                           // and one island of two
                vol[at(x, y, z)] = (uint16_t) (block ? 52000 : 9000 + 37 * x);
                labels[at(x, y, z)] = ((block && !cavity) || speck || pair) ? L : ((x + y + z) % 11 == 0 && !block ? 5 : 0); // a second label scattered around
            }
    ARaymarchLight l0;
    l0.ForwardVector = FVector{1, .35, -.5}; l0.LightIntensity = 0.5f;
    ARaymarchVolume a;
    a.LightsArray = {&l0};
    if (!a.SetVolumeAsset(vol.data(), nx, ny, nz, TBRM_FMT_G16)) { std::printf("error %s\n", tbrm_last_error()); return 2; }
    a.SetWindowCenter(0.55f);
    a.SetWindowWidth(0.5f);
    a.SetRaymarchSteps(72.0f);
    a.Tick(0.016f);
    const tbrm_camera cam = example_camera(W, H);
    std::vector<float> before((size_t) W * H * 4), after(before.size());
    FIslandsResult r;
    std::printf("nolabels refused=%d\n", a.KeepLargestIslands(L, 1, r) ? 0 : 1); // no label volume yet
    if (!a.SetLabelVolume(labels.data(), labels.size())) { std::printf("error %s\n", tbrm_last_error()); return 3; }
    if (!a.RenderLit(cam, before.data())) { std::printf("error %s\n", tbrm_last_error()); return 4; }
    const int frames = a.Stats.Frames, resets = a.Stats.Resets;
    std::vector<uint8_t> got(labels.size());
    auto download = [&]() { return tbrm_download_label_volume(a.RaymarchResources.Handle, got.data(), got.size()) == TBRM_OK; };
    auto mask_of = [&](const std::vector<uint8_t>& l, bool complement) {
        std::vector<uint8_t> m(l.size());
        for (size_t i = 0; i < l.size(); ++i) m[i] = (l[i] == L) != complement;
        return m;
    };
    auto wrong = [&](const std::vector<uint8_t>& want) { size_t n = 0; for (size_t i = 0; i < got.size(); ++i) n += got[i] != want[i]; return n; };

    // closing by radius 1 does not fill a cavity three voxels wide: the dilation does not reach its centre
    FMorphResult m;
    if (!a.CloseLabel(1, L, m) || !download()) { std::printf("error %s\n", tbrm_last_error()); return 5; }
    std::printf("close cavity_open=%d\n", got[at(11, 10, 9)] == 0 ? 1 : 0);
    if (!a.SetLabelVolume(labels.data(), labels.size())) { std::printf("error %s\n", tbrm_last_error()); return 3; }

    // split, measured against the brute force: the three largest get 20, 21, 22 and the rest stays
    std::vector<Island> isl = islands_of(mask_of(labels, false));
    std::vector<uint8_t> want = labels;
    for (size_t i = 0; i < isl.size() && i < 3; ++i)
        for (size_t v : isl[i].voxels) want[v] = (uint8_t) (20 + i);
    if (!a.SplitIslands(L, 20, 3, r) || !download()) { std::printf("error %s\n", tbrm_last_error()); return 6; }
    std::printf("split wrong=%zu counts=%d\n", wrong(want), (r.Islands == isl.size() && r.Kept == 3 && r.Largest == isl[0].size && r.KeptVoxels == isl[0].size + isl[1].size + isl[2].size) ? 1 : 0);
    if (!a.SetLabelVolume(labels.data(), labels.size())) { std::printf("error %s\n", tbrm_last_error()); return 3; }

    // remove the small: single voxels go, the pair and the block stay
    want = labels;
    uint64_t gone = 0;
    for (const Island& i : isl)
        if (i.size < 2) { for (size_t v : i.voxels) want[v] = 0; ++gone; }
    if (!a.RemoveSmallIslands(L, 2, r) || !download()) { std::printf("error %s\n", tbrm_last_error()); return 7; }
    std::printf("remove wrong=%zu counts=%d pair_kept=%d\n", wrong(want), (r.Dropped == gone && r.Relabelled == gone && gone > 0) ? 1 : 0, got[at(34, 10, 9)] == L ? 1 : 0);

    // keep the largest: the pair goes too, nothing else changes
    for (size_t v : isl[1].voxels) want[v] = 0;
    if (!a.KeepLargestIslands(L, 1, r) || !download()) { std::printf("error %s\n", tbrm_last_error()); return 8; }
    size_t label_left = 0, others_same = 0;
    for (size_t i = 0; i < got.size(); ++i) { label_left += got[i] == L; others_same += labels[i] == L || got[i] == labels[i]; } // what was not of the label is as it was
    std::printf("keep wrong=%zu specks_removed=%d nothing_else=%d\n", wrong(want), (r.Islands == 2 && r.Kept == 1 && r.Dropped == 1 && label_left == isl[0].size) ? 1 : 0,
                others_same == got.size() ? 1 : 0);

    // fill the holes: the cavity joins the label; the background outside touches the volume's faces and is spared
    std::vector<Island> holes = islands_of(mask_of(want, true));
    uint64_t enclosed = 0;
    for (const Island& h : holes)
        if (!h.border) { for (size_t v : h.voxels) want[v] = L; enclosed += h.size; }
    if (!a.FillLabelHoles(L, r) || !download()) { std::printf("error %s\n", tbrm_last_error()); return 9; }
    std::printf("fill wrong=%zu counts=%d cavity_filled=%d\n", wrong(want), (r.Relabelled == enclosed && enclosed == 27 && r.Spared >= 1 && r.Kept == 0) ? 1 : 0,
                got[at(10, 9, 8)] == L && got[at(11, 10, 9)] == L && got[at(12, 11, 10)] == L ? 1 : 0);
    // a hole larger than asked for stays: on the first label volume, holes of up to 7 voxels
    if (!a.SetLabelVolume(labels.data(), labels.size()) || !a.FillLabelHoles(L, r, 7) || !download()) { std::printf("error %s\n", tbrm_last_error()); return 10; }
    std::printf("fill_small wrong=%zu kept=%llu\n", wrong(labels), (unsigned long long) r.Kept);

    std::printf("state frames=%d resets=%d recompute=%d\n", a.Stats.Frames - frames, a.Stats.Resets - resets, a.bRequestedRecompute ? 1 : 0);
    if (!a.KeepLargestIslands(L, 1, r) || !a.RenderLit(cam, after.data())) { std::printf("error %s\n", tbrm_last_error()); return 11; }
    std::printf("frame shows_change=%d\n", std::memcmp(before.data(), after.data(), before.size() * sizeof(float)) != 0 ? 1 : 0);
    uint64_t c[6] = {0, 0, 0, 0, 0, 0};
    tbrm_islands_counters(a.RaymarchResources.Handle, c);
    std::printf("counters calls=%llu\n", (unsigned long long) c[0]);
    std::printf("OK\n");
    return 0;
}
