// Drives ARaymarchVolume::ComputeHistogram / GetLabelStatistics / AutoWindow (include/tbrm_plugin.hpp, include/tbrm_volume_stats.h):
// on a volume whose values sit in a narrow band AutoWindow sets the window tbrm_host_window_from_histogram proposes from
// ComputeHistogram's bins, through the setters — the recompute is requested and the next Tick resets the lights once.
// "nohandle": what an actor without resources answers (no device needed). Prints one "key value" line per check;
// tests/test_volume_stats_facade.py compiles it with g++ and runs it.
#include "tbrm_plugin.hpp"

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

int main(int argc, char** argv)
{
    std::vector<uint64_t> hist;
    std::vector<tbrm_label_stat> stats;
    if (argc > 1 && !std::strcmp(argv[1], "nohandle")) {
        ARaymarchVolume none;
        const bool h = none.ComputeHistogram(256, hist), s = none.GetLabelStatistics(stats), w = none.AutoWindow();
        std::printf("nohandle histogram=%d statistics=%d window=%d recompute=%d abi=%d\n", h ? 1 : 0, s ? 1 : 0, w ? 1 : 0, none.bRequestedRecompute ? 1 : 0,
                    tbrm_volume_stats_abi_version());
        return 0;
    }
    const int nx = 40, ny = 24, nz = 19;
    const uint32_t band_lo = 20000u, band_hi = 29999u; // the codes the voxels take: a narrow band of the 16-bit range
    std::vector<uint16_t> vol((size_t) nx * ny * nz);
    uint64_t sum = 0;
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const uint16_t v = (uint16_t) (band_lo + hash32(x, y, z) % (band_hi - band_lo + 1));
                vol[((size_t) z * ny + y) * nx + x] = v;
                sum += v;
            }
    ARaymarchLight l0, l1;
    l0.ForwardVector = FVector{1, .35, -.5}; l0.LightIntensity = 0.5f;
    l1.ForwardVector = FVector{-.4, 1, -.3}; l1.LightIntensity = 0.4f;
    ARaymarchVolume a;
    a.LightsArray = {&l0, &l1};
    if (!a.SetVolumeAsset(vol.data(), nx, ny, nz, TBRM_FMT_G16)) { std::printf("error %s\n", tbrm_last_error()); return 2; }
    a.Tick(0.016f);
    std::printf("before recompute=%d resets=%d\n", a.bRequestedRecompute ? 1 : 0, a.Stats.Resets);

    if (!a.ComputeHistogram(1024, hist)) { std::printf("error %s\n", tbrm_last_error()); return 3; }
    uint64_t total = 0, outside = 0;
    for (size_t k = 0; k < hist.size(); ++k) {
        total += hist[k];
        if (k < band_lo / 64 || k > band_hi / 64) outside += hist[k]; // 1024 bins over 65536 codes: bin = code / 64
    }
    std::printf("histogram bins=%zu total=%llu outside_band=%llu recompute=%d\n", hist.size(), (unsigned long long) total, (unsigned long long) outside,
                a.bRequestedRecompute ? 1 : 0);
    if (!a.GetLabelStatistics(stats)) { std::printf("error %s\n", tbrm_last_error()); return 4; }
    std::printf("statistics count=%llu sum_ok=%d min_ok=%d max_ok=%d others=%llu\n", (unsigned long long) stats[0].count, stats[0].sum == (double) sum ? 1 : 0,
                stats[0].min >= band_lo ? 1 : 0, stats[0].max <= band_hi ? 1 : 0, (unsigned long long) (stats[1].count + stats[255].count));

    tbrm_windowing_params want{};
    if (tbrm_host_window_from_histogram(hist.data(), (int32_t) hist.size(), 0.0, 65536.0 / 65535.0, 0.01f, 0.99f, &want) != TBRM_OK) { std::printf("error %s\n", tbrm_last_error()); return 5; }
    const bool ok = a.AutoWindow();
    const FWindowingParameters& w = a.RaymarchResources.WindowingParameters;
    std::printf("auto_window accepted=%d equal=%d cutoffs=%d%d recompute=%d\n", ok ? 1 : 0, (w.Center == want.center && w.Width == want.width) ? 1 : 0,
                w.LowCutoff ? 1 : 0, w.HighCutoff ? 1 : 0, a.bRequestedRecompute ? 1 : 0);
    const double lower = (double) w.Center - (double) w.Width / 2, upper = (double) w.Center + (double) w.Width / 2;
    std::printf("band inside=%d narrow=%d\n", (lower >= (band_lo - 64) / 65535.0 && upper <= (band_hi + 65) / 65535.0) ? 1 : 0, w.Width < 0.2f ? 1 : 0);
    a.Tick(0.016f);
    std::printf("after_tick recompute=%d resets=%d\n", a.bRequestedRecompute ? 1 : 0, a.Stats.Resets);
    a.Tick(0.016f);
    std::printf("second_tick resets=%d\n", a.Stats.Resets);
    const bool again = a.AutoWindow(); // the same window again: the setters see no change
    std::printf("again accepted=%d recompute=%d\n", again ? 1 : 0, a.bRequestedRecompute ? 1 : 0);
    uint64_t c[4] = {0, 0, 0, 0};
    tbrm_volume_stats_counters(a.RaymarchResources.Handle, c);
    std::printf("counters histograms=%llu statistics=%llu\n", (unsigned long long) c[0], (unsigned long long) c[1]);
    std::printf("OK\n");
    return 0;
}
