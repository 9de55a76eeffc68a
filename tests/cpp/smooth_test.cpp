// Drives ARaymarchVolume::SmoothLabel and MedianLabel (include/tbrm_plugin.hpp, include/tbrm_smooth.h): a ball of label voxels with a
// spur, a pit and a speck in a MetaImage volume with ElementSpacing 1 1 2.5, smoothed by world radii; every label volume is compared
// with a brute-force restatement below: the window clipped to the volume, counted by loops. The calls request no recompute and count
// as no frame.
// "nohandle": what an actor without resources answers (no device needed). Otherwise argv[1] is a directory to write the volume to.
// Prints one "key value" line per check; tests/test_smooth_facade.py compiles it with g++ and runs it.
#include "tbrm_volume_io.hpp" // includes tbrm_plugin.hpp

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace tbrm_plugin;

static const int nx = 40, ny = 20, nz = 19;
static size_t at(int x, int y, int z) { return ((size_t) z * ny + y) * nx + x; }

// one pass: set where more than num / den of the voxels of the box [v - r, v + r] that lie inside the volume are set
static std::vector<uint8_t> rank_pass(const std::vector<uint8_t>& m, const int r[3], int num, int den)
{
    std::vector<uint8_t> out(m.size(), 0);
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                long c = 0, n = 0;
                for (int Z = z - r[2]; Z <= z + r[2]; ++Z)
                    for (int Y = y - r[1]; Y <= y + r[1]; ++Y)
                        for (int X = x - r[0]; X <= x + r[0]; ++X) {
                            if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) continue;
                            ++n;
                            c += m[at(X, Y, Z)];
                        }
                out[at(x, y, z)] = c * den > n * num;
            }
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
        FSmoothResult m;
        const bool a = none.SmoothLabel(1, 2.0, 1, m), b = none.MedianLabel(1, 1.0, 2, m);
        std::printf("nohandle smooth=%d median=%d added=%llu recompute=%d abi=%d\n", a ? 1 : 0, b ? 1 : 0, (unsigned long long) m.Added,
                    none.bRequestedRecompute ? 1 : 0, tbrm_smooth_abi_version());
        return 0;
    }
    if (argc < 2) { std::printf("error: a directory to write the volume to\n"); return 1; }

    const int W = 48, H = 40, L = 3;
    const double spacing[3] = {1.0, 1.0, 2.5};
    std::vector<uint16_t> vol((size_t) nx * ny * nz);
    std::vector<uint8_t> labels(vol.size(), 0);
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const double dx = x - 14, dy = y - 10, dz = (z - 9) * 2.5;
                const bool ball = dx * dx + dy * dy + dz * dz <= 64.0;           // a ball of 8 world units
                const bool spur = y == 10 && z == 9 && x > 22 && x <= 28;         // a one-voxel spur on its side
                const bool speck = x == 34 && y == 10 && z == 9;                 // a voxel of its own
                vol[at(x, y, z)] = (uint16_t) (ball ? 52000 : 9000 + 37 * x);
                labels[at(x, y, z)] = (ball || spur || speck) ? L : ((x + y + z) % 11 == 0 ? 5 : 0); // a second label scattered around
            }
    labels[at(14, 10, 9)] = 0; // a pit in the middle
    const std::string dir = argv[1];
    {
        FILE* raw = std::fopen((dir + "/ball.raw").c_str(), "wb");
        FILE* mhd = std::fopen((dir + "/ball.mhd").c_str(), "w");
        if (!raw || !mhd) { std::printf("error: cannot write to %s\n", dir.c_str()); return 1; }
        std::fwrite(vol.data(), sizeof(uint16_t), vol.size(), raw);
        std::fprintf(mhd, "ObjectType = Image\nNDims = 3\nDimSize = %d %d %d\nElementSpacing = 1 1 2.5\nElementType = MET_USHORT\nElementDataFile = ball.raw\n", nx, ny, nz);
        std::fclose(raw);
        std::fclose(mhd);
    }
    ARaymarchLight l0;
    l0.ForwardVector = FVector{1, .35, -.5}; l0.LightIntensity = 0.5f;
    ARaymarchVolume a;
    a.LightsArray = {&l0};
    if (!LoadMHDFileIntoVolumeNormalized(a, dir + "/ball.mhd")) { std::printf("error %s\n", tbrm_last_error()); return 2; }
    std::printf("spacing loaded=%d\n", (a.VoxelSpacing[0] == 1.0 && a.VoxelSpacing[1] == 1.0 && a.VoxelSpacing[2] == 2.5) ? 1 : 0);
    a.SetWindowCenter(0.55f);
    a.SetWindowWidth(0.5f);
    a.SetRaymarchSteps(72.0f);
    a.Tick(0.016f);
    const tbrm_camera cam = example_camera(W, H);
    std::vector<float> before((size_t) W * H * 4), after(before.size());
    FSmoothResult m;
    std::printf("nolabels refused=%d\n", a.MedianLabel(L, 1.0, 1, m) ? 0 : 1); // no label volume yet
    if (!a.SetLabelVolume(labels.data(), labels.size())) { std::printf("error %s\n", tbrm_last_error()); return 3; }
    if (!a.RenderLit(cam, before.data())) { std::printf("error %s\n", tbrm_last_error()); return 4; }
    const int frames = a.Stats.Frames, resets = a.Stats.Resets;

    // each call on the labels the one before left: the expected volume follows along
    std::vector<uint8_t> want = labels, got(labels.size());
    struct Call { const char* name; double radius; int iterations, num, den; bool unit; int r[3]; };
    const Call calls[] = {{"median", 1.0, 1, 1, 2, false, {1, 1, 0}}, {"median3", 3.0, 1, 1, 2, false, {3, 3, 1}}, {"twice", 2.0, 2, 1, 2, false, {2, 2, 1}},
        {"third", 2.0, 1, 1, 3, false, {2, 2, 1}}, {"median_unit", 2.0, 1, 1, 2, true, {2, 2, 2}}};
    for (const Call& c : calls) {
        for (int k = 0; k < 3; ++k) a.VoxelSpacing[k] = c.unit ? 0.0 : spacing[k]; // all zero: unit spacing
        std::vector<uint8_t> S(want.size());
        for (size_t i = 0; i < want.size(); ++i) S[i] = want[i] == L;
        std::vector<uint8_t> R = S;
        for (int i = 0; i < c.iterations; ++i) R = rank_pass(R, c.r, c.num, c.den);
        uint64_t source = 0, result = 0, added = 0, removed = 0;
        for (size_t i = 0; i < want.size(); ++i) {
            source += S[i];
            result += R[i];
            if (R[i] && !S[i]) { ++added; want[i] = L; }
            if (S[i] && !R[i]) { ++removed; want[i] = 0; }
        }
        const bool ok = (c.num == 1 && c.den == 2) ? a.MedianLabel(L, c.radius, c.iterations, m) : a.SmoothLabel(L, c.radius, c.iterations, m, c.num, c.den);
        if (!ok) { std::printf("error %s\n", tbrm_last_error()); return 5; }
        if (tbrm_download_label_volume(a.RaymarchResources.Handle, got.data(), got.size()) != TBRM_OK) { std::printf("error %s\n", tbrm_last_error()); return 6; }
        size_t wrong = 0;
        for (size_t i = 0; i < got.size(); ++i) wrong += got[i] != want[i];
        std::printf("%s wrong=%zu counts=%d moved=%d radius=%d,%d,%d reach=%d,%d,%d launches=%d\n", c.name, wrong,
                    (m.SourceVoxels == source && m.ResultVoxels == result && m.Added == added && m.Removed == removed && m.Relabelled == added + removed) ? 1 : 0,
                    added + removed > 0 ? 1 : 0, m.Radius[0], m.Radius[1], m.Radius[2], m.Reach[0], m.Reach[1], m.Reach[2], m.Launches);
        if (!std::strcmp(c.name, "median"))
            std::printf("features pit_filled=%d spur_cut=%d speck_removed=%d ball_kept=%d\n", got[at(14, 10, 9)] == L ? 1 : 0, got[at(27, 10, 9)] == 0 ? 1 : 0,
                        got[at(34, 10, 9)] == 0 ? 1 : 0, got[at(12, 10, 9)] == L ? 1 : 0);
    }
    for (int k = 0; k < 3; ++k) a.VoxelSpacing[k] = spacing[k];

    // measured only: the counts of a pass at 1 / 4, nothing written
    if (!a.SmoothLabel(L, 2.0, 1, m, 1, 4, 0, true)) { std::printf("error %s\n", tbrm_last_error()); return 7; }
    std::vector<uint8_t> again(got.size());
    tbrm_download_label_volume(a.RaymarchResources.Handle, again.data(), again.size());
    std::printf("measure added=%d relabelled=%llu unchanged=%d\n", m.Added > 0 ? 1 : 0, (unsigned long long) m.Relabelled, again == got ? 1 : 0);
    // what leaves can get a label of its own
    if (!a.SmoothLabel(L, 2.0, 1, m, 3, 4, 9)) { std::printf("error %s\n", tbrm_last_error()); return 8; }
    tbrm_download_label_volume(a.RaymarchResources.Handle, again.data(), again.size());
    uint64_t nines = 0;
    for (uint8_t v : again) nines += v == 9;
    std::printf("erase_label removed_got_it=%d\n", (nines == m.Removed && nines > 0) ? 1 : 0);
    // what no call can take: a radius below half a voxel, above the largest, not a number; no pass, too long a reach, a rank of 1
    std::printf("refused small=%d large=%d nan=%d iterations=%d reach=%d rank=%d\n", a.MedianLabel(L, 0.4, 1, m) ? 0 : 1, a.MedianLabel(L, 17.0, 1, m) ? 0 : 1,
                a.MedianLabel(L, std::nan(""), 1, m) ? 0 : 1, a.MedianLabel(L, 1.0, 0, m) ? 0 : 1, a.MedianLabel(L, 16.0, 5, m) ? 0 : 1, a.SmoothLabel(L, 1.0, 1, m, 2, 2) ? 0 : 1);

    std::printf("state frames=%d resets=%d recompute=%d\n", a.Stats.Frames - frames, a.Stats.Resets - resets, a.bRequestedRecompute ? 1 : 0);
    if (!a.RenderLit(cam, after.data())) { std::printf("error %s\n", tbrm_last_error()); return 9; }
    std::printf("frame shows_change=%d\n", std::memcmp(before.data(), after.data(), before.size() * sizeof(float)) != 0 ? 1 : 0);
    uint64_t c[4] = {0, 0, 0, 0};
    tbrm_smooth_counters(a.RaymarchResources.Handle, c);
    std::printf("counters calls=%llu launches=%llu\n", (unsigned long long) c[0], (unsigned long long) c[1]);
    std::printf("OK\n");
    return 0;
}
