// Drives ARaymarchVolume::UpdateVolumeRegion (include/tbrm_plugin.hpp, include/tbrm_volume_region.h): a sub-box written into the
// asset of one actor requests a recompute, and after the next Tick its frame is the frame of a second actor that was given the
// edited volume whole. "nohandle": what an actor without resources answers (no device needed). Prints one "key value" line per
// check; tests/test_volume_region_facade.py compiles it with g++ and runs it.
#include "tbrm_plugin.hpp"

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

static void setup(ARaymarchVolume& v)
{
    FColorCurve tf;
    tf.AddKey(0.0f, 0, 0, 0, 0); tf.AddKey(0.25f, .8f, .4f, .3f, 0); tf.AddKey(0.45f, .9f, .6f, .5f, .02f);
    tf.AddKey(0.70f, 1, 1, .9f, .15f); tf.AddKey(1.0f, 1, 1, 1, .40f);
    v.SetTFCurve(tf);
    v.SetWindowCenter(0.5f); v.SetWindowWidth(0.9f); v.SetHighCutoff(false);
    v.SetRaymarchSteps(64);
}

int main(int argc, char** argv)
{
    const int32_t origin[3] = {5, 11, 3}, extent[3] = {13, 6, 9};
    std::vector<uint16_t> box((size_t) extent[0] * extent[1] * extent[2]);
    if (argc > 1 && !std::strcmp(argv[1], "nohandle")) {
        ARaymarchVolume none;
        const bool refused = !none.UpdateVolumeRegion(origin, extent, box.data(), box.size() * 2);
        std::printf("nohandle %s recompute=%d abi=%d\n", refused ? "refused" : "accepted", none.bRequestedRecompute ? 1 : 0, tbrm_volume_region_abi_version());
        return 0;
    }
    const int nx = 40, ny = 24, nz = 19;
    std::vector<uint16_t> vol((size_t) nx * ny * nz), edited;
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const double px = (x + 0.5) / nx - 0.5, py = (y + 0.5) / ny - 0.5, pz = (z + 0.5) / nz - 0.5;
                const double r = std::sqrt(px * px + py * py + pz * pz);
                double v = (r < 0.42 ? 0.35 : 0.0) + 0.02 * (hash32(x, y, z) / 4294967296.0 - 0.5);
                v = v < 0 ? 0 : (v > 1 ? 1 : v);
                vol[((size_t) z * ny + y) * nx + x] = (uint16_t) (v * 65535.0 + 0.5);
            }
    edited = vol;
    for (int z = 0; z < extent[2]; ++z)
        for (int y = 0; y < extent[1]; ++y)
            for (int x = 0; x < extent[0]; ++x) {
                const uint16_t v = (uint16_t) (40000u + hash32(x, y, z) % 25000u);
                box[((size_t) z * extent[1] + y) * extent[0] + x] = v;
                edited[((size_t) (z + origin[2]) * ny + (y + origin[1])) * nx + (x + origin[0])] = v;
            }

    ARaymarchLight l0, l1;
    l0.ForwardVector = FVector{1, .35, -.5}; l0.LightIntensity = 0.5f;
    l1.ForwardVector = FVector{-.4, 1, -.3}; l1.LightIntensity = 0.4f;
    ARaymarchVolume a, b;
    a.LightsArray = {&l0, &l1};
    b.LightsArray = {&l0, &l1};
    if (!a.SetVolumeAsset(vol.data(), nx, ny, nz, TBRM_FMT_G16) || !b.SetVolumeAsset(edited.data(), nx, ny, nz, TBRM_FMT_G16)) { std::printf("error %s\n", tbrm_last_error()); return 2; }
    setup(a);
    setup(b);
    a.Tick(0.016f);
    b.Tick(0.016f);

    tbrm_camera cam{};
    cam.position = FVector{-145, -95, 80};
    const double fl = std::sqrt(145.0 * 145 + 95.0 * 95 + 80.0 * 80);
    cam.forward = FVector{145 / fl, 95 / fl, -80 / fl};
    const double rl = std::sqrt(cam.forward.y * cam.forward.y + cam.forward.x * cam.forward.x);
    cam.right = FVector{cam.forward.y / rl, -cam.forward.x / rl, 0};
    cam.up = FVector{cam.right.y * cam.forward.z - cam.right.z * cam.forward.y, cam.right.z * cam.forward.x - cam.right.x * cam.forward.z,
        cam.right.x * cam.forward.y - cam.right.y * cam.forward.x};
    cam.tan_half_fov_y = std::tan(30.0 * 3.14159265358979323846 / 180.0);
    cam.tan_half_fov_x = cam.tan_half_fov_y * 64.0 / 48.0;
    cam.width = 64; cam.height = 48;
    std::vector<float> fa((size_t) 64 * 48 * 4), fb(fa.size()), before(fa.size());
    if (!a.RenderLit(cam, before.data(), 3) || !b.RenderLit(cam, fb.data(), 3)) { std::printf("error %s\n", tbrm_last_error()); return 3; }
    std::printf("before_update differs=%d recompute=%d resets=%d\n", std::memcmp(before.data(), fb.data(), fb.size() * 4) != 0, a.bRequestedRecompute ? 1 : 0, a.Stats.Resets);

    const int32_t outside[3] = {30, 11, 3};
    const bool bad = a.UpdateVolumeRegion(outside, extent, box.data(), box.size() * 2);
    std::printf("outside accepted=%d recompute=%d\n", bad ? 1 : 0, a.bRequestedRecompute ? 1 : 0);
    const bool ok = a.UpdateVolumeRegion(origin, extent, box.data(), box.size() * 2);
    std::printf("update accepted=%d recompute=%d octree_rebuild=%d\n", ok ? 1 : 0, a.bRequestedRecompute ? 1 : 0, a.bRequestedOctreeRebuild ? 1 : 0);
    a.Tick(0.016f);
    std::printf("after_tick recompute=%d resets=%d adds=%d\n", a.bRequestedRecompute ? 1 : 0, a.Stats.Resets, a.Stats.LightAdds);
    if (!a.RenderLit(cam, fa.data(), 3)) { std::printf("error %s\n", tbrm_last_error()); return 4; }
    std::printf("frame %s\n", std::memcmp(fa.data(), fb.data(), fb.size() * 4) ? "differs" : "identical");
    std::vector<uint8_t> la((size_t) nx * ny * nz), lb(la.size());
    tbrm_download_light_volume(a.RaymarchResources.Handle, la.data(), la.size());
    tbrm_download_light_volume(b.RaymarchResources.Handle, lb.data(), lb.size());
    std::printf("light_volume %s\n", la == lb ? "identical" : "differs");
    uint64_t c[4] = {0, 0, 0, 0};
    tbrm_volume_region_counters(a.RaymarchResources.Handle, c);
    std::printf("counters updates=%llu voxels=%llu\n", (unsigned long long) c[0], (unsigned long long) c[1]);
    std::printf("OK\n");
    return 0;
}
