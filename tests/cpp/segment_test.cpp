// Drives ARaymarchVolume::GrowRegion / GrowRegionAt (include/tbrm_plugin.hpp, include/tbrm_segment.h): a click on a blob labels the
// blob under the pixel and nothing else, attaches the label volume it needs, requests no recompute and counts as no frame; a click
// that meets nothing grows nothing.
// "nohandle": what an actor without resources answers (no device needed).
// Prints one "key value" line per check; tests/test_segment_facade.py compiles it with g++ and runs it.
#include "tbrm_volume_io.hpp" // includes tbrm_plugin.hpp

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace tbrm_plugin;

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
        FGrowResult g;
        const int32_t seed[3] = {0, 0, 0};
        const tbrm_camera cam = example_camera(2, 2);
        const bool a = none.GrowRegion(seed, 1, 0.0, 1.0, 1, 6, g), b = none.GrowRegionAt(cam, 0, 0, 0.5f, 10.0, 1, 6, g);
        std::printf("nohandle grow=%d at=%d seeded=%d voxels=%llu recompute=%d abi=%d\n", a ? 1 : 0, b ? 1 : 0, g.bSeeded ? 1 : 0, (unsigned long long) g.Voxels,
                    none.bRequestedRecompute ? 1 : 0, tbrm_segment_abi_version());
        return 0;
    }

    // two balls of the same value in a volume of nothing: the large one in the middle, a small one in a corner, not touching
    const int nx = 40, ny = 36, nz = 28, W = 48, H = 40;
    std::vector<uint16_t> vol((size_t) nx * ny * nz);
    std::vector<uint8_t> ball((size_t) nx * ny * nz);
    size_t in_middle = 0, in_corner = 0;
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const double dx = x - 19.5, dy = y - 17.5, dz = z - 13.5, ex = x - 34.0, ey = y - 30.0, ez = z - 4.0;
                const bool middle = dx * dx + dy * dy + dz * dz <= 81.0, corner = ex * ex + ey * ey + ez * ez <= 9.0;
                vol[((size_t) z * ny + y) * nx + x] = (middle || corner) ? 52000 : 0;
                ball[((size_t) z * ny + y) * nx + x] = middle ? 1 : 0;
                in_middle += middle;
                in_corner += corner;
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
    if (!a.RenderLit(cam, before.data())) { std::printf("error %s\n", tbrm_last_error()); return 3; }
    const int frames = a.Stats.Frames, resets = a.Stats.Resets;

    FGrowResult miss;
    if (!a.GrowRegionAt(cam, 0, 0, 0.5f, 100.0, 7, 6, miss)) { std::printf("error %s\n", tbrm_last_error()); return 4; }
    std::printf("miss seeded=%d voxels=%llu labels=%d\n", miss.bSeeded ? 1 : 0, (unsigned long long) miss.Voxels, tbrm_has_label_volume(a.RaymarchResources.Handle));

    FGrowResult g;
    if (!a.GrowRegionAt(cam, W / 2, H / 2, 0.8f, 100.0, 7, 6, g)) { std::printf("error %s\n", tbrm_last_error()); return 5; }
    std::vector<uint8_t> labels(vol.size(), 255);
    if (tbrm_download_label_volume(a.RaymarchResources.Handle, labels.data(), labels.size()) != TBRM_OK) { std::printf("error %s\n", tbrm_last_error()); return 6; }
    size_t wrong = 0;
    for (size_t i = 0; i < labels.size(); ++i) wrong += labels[i] != (ball[i] ? 7 : 0);
    const size_t seed_at = ((size_t) g.Seed[2] * ny + g.Seed[1]) * nx + g.Seed[0];
    std::printf("grow seeded=%d seed_in_ball=%d voxels_are_the_ball=%d relabelled_all=%d wrong=%zu corner_untouched=%d attached=%d\n", g.bSeeded ? 1 : 0,
                (g.bSeeded && ball[seed_at]) ? 1 : 0, g.Voxels == in_middle ? 1 : 0, g.Relabelled == in_middle ? 1 : 0, wrong, in_corner > 0 ? 1 : 0,
                tbrm_has_label_volume(a.RaymarchResources.Handle));
    std::printf("range lo=%.9g hi=%.9g box=%d,%d,%d..%d,%d,%d\n", g.LoUsed, g.HiUsed, g.BoxMin[0], g.BoxMin[1], g.BoxMin[2], g.BoxMax[0], g.BoxMax[1], g.BoxMax[2]);

    std::vector<tbrm_label_stat> stats;
    a.GetLabelStatistics(stats);
    std::printf("stats count_is_voxels=%d mean=%.9g\n", stats[7].count == g.Voxels ? 1 : 0, stats[7].count ? stats[7].sum / (double) stats[7].count : 0.0);

    // measured only, from the seed itself, 26-connected: the same ball, nothing written
    FGrowResult m;
    if (!a.GrowRegion(g.Seed, 1, 51900.0, 52100.0, -1, 26, m)) { std::printf("error %s\n", tbrm_last_error()); return 7; }
    std::printf("measure voxels_are_the_ball=%d relabelled=%llu\n", m.Voxels == in_middle ? 1 : 0, (unsigned long long) m.Relabelled);

    std::printf("state frames=%d resets=%d recompute=%d\n", a.Stats.Frames - frames, a.Stats.Resets - resets, a.bRequestedRecompute ? 1 : 0);
    if (!a.RenderLit(cam, after.data())) { std::printf("error %s\n", tbrm_last_error()); return 8; }
    std::printf("frame shows_label=%d\n", std::memcmp(before.data(), after.data(), before.size() * sizeof(float)) != 0 ? 1 : 0);
    a.ClearLabelVolume();
    if (!a.RenderLit(cam, after.data())) { std::printf("error %s\n", tbrm_last_error()); return 9; }
    std::printf("cleared identical=%d\n", std::memcmp(before.data(), after.data(), before.size() * sizeof(float)) == 0 ? 1 : 0);
    uint64_t c[4] = {0, 0, 0, 0};
    tbrm_segment_counters(a.RaymarchResources.Handle, c);
    std::printf("counters calls=%llu\n", (unsigned long long) c[0]);
    std::printf("OK\n");
    return 0;
}
