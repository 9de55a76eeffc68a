// Drives ARaymarchVolume::PickVolume / RenderHitDepth (include/tbrm_plugin.hpp, include/tbrm_hit.h): the facade's answers are the
// C-ABI's (tbrm_pick, tbrm_raymarch_hits) for the actor's current window, steps and world parameters, and neither call counts as a
// frame, requests a recompute or changes the next frame.
// "nohandle": what an actor without resources answers (no device needed).
// "mhd FILE W H STEPS X,Y": the pick of examples/render_mhd.cpp --pick X,Y by the C-ABI call, printed in the example's words (the
// example's window and camera restated here; lights do not matter to a hit).
// Prints one "key value" line per check; tests/test_hit_facade.py compiles it with g++ and runs it.
#include "tbrm_volume_io.hpp" // includes tbrm_plugin.hpp

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace tbrm_plugin;

static uint32_t hash32(uint32_t x, uint32_t y, uint32_t z)
{
    uint32_t h = x * 73856093u ^ y * 19349663u ^ z * 83492791u ^ 0x5EED0002u;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
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
        FVolumeHit hit;
        float depth[4] = {-1, -1, -1, -1};
        const tbrm_camera cam = example_camera(2, 2);
        const bool p = none.PickVolume(cam, 0, 0, 0.5f, hit), d = none.RenderHitDepth(cam, depth, 0.5f);
        std::printf("nohandle pick=%d depth=%d hit=%d untouched=%d recompute=%d abi=%d\n", p ? 1 : 0, d ? 1 : 0, hit.bHit ? 1 : 0, depth[0] == -1 ? 1 : 0,
                    none.bRequestedRecompute ? 1 : 0, tbrm_hit_abi_version());
        return 0;
    }
    if (argc > 6 && !std::strcmp(argv[1], "mhd")) {
        int px = 0, py = 0;
        if (std::sscanf(argv[6], "%d,%d", &px, &py) != 2) return 2;
        ARaymarchVolume volume;
        FVolumeInfo info;
        if (!LoadMHDFileIntoVolumeNormalized(volume, argv[2], &info)) { std::printf("error %s\n", tbrm_last_error()); return 2; }
        volume.SetWindowCenter(info.NormalizeValue(info.MinValue + 0.6f * (info.MaxValue - info.MinValue)));
        volume.SetWindowWidth(info.NormalizeRange(0.8f * (info.MaxValue - info.MinValue)));
        volume.SetRaymarchSteps((float) std::atof(argv[5]));
        volume.Tick(0.016f);
        const tbrm_camera cam = example_camera(std::atoi(argv[3]), std::atoi(argv[4]));
        const tbrm_raymarch_params rp{volume.RaymarchingSteps, -1, 1, 0};
        const tbrm_world_params w = volume.WorldParameters.abi();
        tbrm_hit h{};
        double xyz[3], depth = 0;
        if (tbrm_pick(volume.RaymarchResources.Handle, &cam, px, py, &rp, &w, 0.5f, &h, xyz, &depth) != TBRM_OK) { std::printf("error %s\n", tbrm_last_error()); return 3; }
        if (h.sample >= 0) std::printf("pick %d,%d hit sample %d world %.9g %.9g %.9g depth %.9g value %.9g label %d\n", px, py, h.sample, xyz[0], xyz[1], xyz[2], depth,
                                       (double) h.value, h.label);
        else std::printf("pick %d,%d miss\n", px, py);
        return 0;
    }

    const int nx = 40, ny = 36, nz = 28, W = 48, H = 40;
    std::vector<uint16_t> vol((size_t) nx * ny * nz);
    std::vector<uint8_t> labels(vol.size());
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) { // a ball, denser towards its centre, with a little noise; labels: its octants
                const double dx = (x + 0.5) / nx - 0.5, dy = (y + 0.5) / ny - 0.5, dz = (z + 0.5) / nz - 0.5;
                const double v = 0.95 - 1.6 * std::sqrt(dx * dx + dy * dy + dz * dz) + 0.03 * (hash32(x, y, z) % 1000) / 1000.0;
                vol[((size_t) z * ny + y) * nx + x] = (uint16_t) std::lround(65535.0 * std::fmin(std::fmax(v, 0.0), 1.0));
                labels[((size_t) z * ny + y) * nx + x] = (uint8_t) (1 + (dx > 0) + 2 * (dy > 0) + 4 * (dz > 0));
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

    const tbrm_raymarch_params rp{a.RaymarchingSteps, -1, 1, 0};
    const tbrm_world_params w = a.WorldParameters.abi();
    const tbrm_tile tile{0, 0, W, H, 1, 0};
    std::vector<tbrm_hit> map((size_t) W * H);
    std::vector<float> map_depth(map.size()), facade_depth(map.size(), -1.0f);
    if (tbrm_raymarch_hits(a.RaymarchResources.Handle, &cam, &tile, &rp, &w, 0.5f, map.data(), map_depth.data()) != TBRM_OK) { std::printf("error %s\n", tbrm_last_error()); return 4; }
    if (!a.RenderHitDepth(cam, facade_depth.data(), 0.5f)) { std::printf("error %s\n", tbrm_last_error()); return 5; }
    int n_hit = 0, n_miss = 0;
    for (const tbrm_hit& h : map) (h.sample >= 0 ? n_hit : n_miss) += 1;
    std::printf("depth equal=%d hits=%d misses=%d\n", std::memcmp(map_depth.data(), facade_depth.data(), map_depth.size() * sizeof(float)) == 0 ? 1 : 0,
                n_hit >= 100 ? 1 : 0, n_miss >= 100 ? 1 : 0);

    int picks = 0, same = 0, hit_picks = 0, on_depth = 0;
    for (int py = 1; py < H; py += 4)
        for (int px = 2; px < W; px += 5) {
            FVolumeHit f;
            if (!a.PickVolume(cam, px, py, 0.5f, f)) { std::printf("error %s\n", tbrm_last_error()); return 6; }
            const tbrm_hit& h = map[(size_t) py * W + px];
            double xyz[3], depth = 0;
            tbrm_host_hits_to_world(&w, &cam, &h, 1, xyz, &depth);
            ++picks;
            if (f.bHit == (h.sample >= 0) && f.Sample == h.sample && f.Value == h.value && f.Label == h.label && f.WorldPosition.x == xyz[0] &&
                f.WorldPosition.y == xyz[1] && f.WorldPosition.z == xyz[2] && (f.Depth == depth || (std::isinf(f.Depth) && std::isinf(depth)))) ++same;
            if (f.bHit) {
                ++hit_picks;
                if (std::fabs(f.Depth - (double) map_depth[(size_t) py * W + px]) <= 1e-3) ++on_depth; // the kernel's fp32 depth against the host's double
            }
        }
    std::printf("pick same=%d on_depth=%d picks=%d hits=%d\n", same == picks ? 1 : 0, on_depth == hit_picks ? 1 : 0, picks, hit_picks);

    if (!a.SetLabelVolume(labels.data(), labels.size())) { std::printf("error %s\n", tbrm_last_error()); return 7; }
    FVolumeHit centre;
    a.PickVolume(cam, W / 2, H / 2, 0.5f, centre);
    std::printf("labelled hit=%d label_in_range=%d\n", centre.bHit ? 1 : 0, (centre.Label >= 1 && centre.Label <= 8) ? 1 : 0);
    a.ClearLabelVolume();

    std::printf("state frames=%d resets=%d recompute=%d\n", a.Stats.Frames - frames, a.Stats.Resets - resets, a.bRequestedRecompute ? 1 : 0);
    if (!a.RenderLit(cam, after.data())) { std::printf("error %s\n", tbrm_last_error()); return 8; }
    std::printf("frame identical=%d\n", std::memcmp(before.data(), after.data(), before.size() * sizeof(float)) == 0 ? 1 : 0);
    uint64_t c[3] = {0, 0, 0};
    tbrm_hit_counters(a.RaymarchResources.Handle, c);
    std::printf("counters maps=%llu picks=%llu launches=%llu\n", (unsigned long long) c[0], (unsigned long long) c[1], (unsigned long long) c[2]);
    std::printf("OK\n");
    return 0;
}
