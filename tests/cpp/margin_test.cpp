// Drives ARaymarchVolume::MarginLabel and ExpandLabelBy / ShrinkLabelBy / OpenLabelBy / CloseLabelBy (include/tbrm_plugin.hpp,
// include/tbrm_margin.h): a ball of label voxels in a MetaImage volume with ElementSpacing 1 1 2.5, expanded, shrunk, opened and closed
// by world radii; every label volume is compared with a brute-force restatement below, in world units and doubles (2.5^2 is exact,
// so are the radii's squares). The calls request no recompute and count as no frame.
// "nohandle": what an actor without resources answers (no device needed). Otherwise argv[1] is a directory to write the volume to.
// Prints one "key value" line per check; tests/test_margin_facade.py compiles it with g++ and runs it.
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

// the voxels of the volume within `radius` (world units) of a set voxel; outside the volume counts as unset
static std::vector<uint8_t> expand(const std::vector<uint8_t>& m, const double spacing[3], double radius)
{
    std::vector<uint8_t> out(m.size(), 0);
    const int rx = (int) std::floor(radius / spacing[0]), ry = (int) std::floor(radius / spacing[1]), rz = (int) std::floor(radius / spacing[2]);
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                bool any = false;
                for (int dz = -rz; dz <= rz && !any; ++dz)
                    for (int dy = -ry; dy <= ry && !any; ++dy)
                        for (int dx = -rx; dx <= rx && !any; ++dx) {
                            const int X = x + dx, Y = y + dy, Z = z + dz;
                            if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz || !m[at(X, Y, Z)]) continue;
                            const double wx = dx * spacing[0], wy = dy * spacing[1], wz = dz * spacing[2];
                            any = wx * wx + wy * wy + wz * wz <= radius * radius;
                        }
                out[at(x, y, z)] = any;
            }
    return out;
}

static std::vector<uint8_t> complement(std::vector<uint8_t> m)
{
    for (uint8_t& v : m) v = !v;
    return m;
}

static std::vector<uint8_t> operate(const std::vector<uint8_t>& m, int op, const double spacing[3], double radius)
{
    auto shrink = [&](const std::vector<uint8_t>& s) { return complement(expand(complement(s), spacing, radius)); };
    switch (op) {
        case TBRM_MARGIN_EXPAND: return expand(m, spacing, radius);
        case TBRM_MARGIN_SHRINK: return shrink(m);
        case TBRM_MARGIN_OPEN: return expand(shrink(m), spacing, radius);
        default: return shrink(expand(m, spacing, radius));
    }
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
        FMarginResult m;
        const bool a = none.MarginLabel(TBRM_MARGIN_CLOSE, 2.0, 1, m), b = none.ExpandLabelBy(1.0, 1, m), c = none.ShrinkLabelBy(1.0, 1, m), d = none.OpenLabelBy(1.0, 1, m),
                   e = none.CloseLabelBy(1.0, 1, m);
        std::printf("nohandle margin=%d expand=%d shrink=%d open=%d close=%d added=%llu recompute=%d abi=%d\n", a ? 1 : 0, b ? 1 : 0, c ? 1 : 0, d ? 1 : 0,
                    e ? 1 : 0, (unsigned long long) m.Added, none.bRequestedRecompute ? 1 : 0, tbrm_margin_abi_version());
        return 0;
    }
    if (argc < 2) { std::printf("error: a directory to write the volume to\n"); return 1; }

    const int W = 48, H = 40, L = 3;
    const double spacing[3] = {1.0, 1.0, 2.5}, unit[3] = {1.0, 1.0, 1.0};
    std::vector<uint16_t> vol((size_t) nx * ny * nz);
    std::vector<uint8_t> labels(vol.size(), 0);
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const double dx = x - 14, dy = y - 10, dz = (z - 9) * 2.5;
                const bool ball = dx * dx + dy * dy + dz * dz <= 36.0;           // a ball of 6 world units
                const bool speck = x == 30 && y == 10 && z == 9;                 // a voxel of its own, which an opening removes
                vol[at(x, y, z)] = (uint16_t) (ball ? 52000 : 9000 + 37 * x);
                labels[at(x, y, z)] = (ball || speck) ? L : ((x + y + z) % 11 == 0 ? 5 : 0); // a second label scattered around
            }
    labels[at(14, 10, 9)] = 0; // a pinhole, which a closing fills
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
    a.VoxelSpacing[0] = 7.0; // (a new asset resets it, the loader sets it)
    if (!LoadMHDFileIntoVolumeNormalized(a, dir + "/ball.mhd")) { std::printf("error %s\n", tbrm_last_error()); return 2; }
    std::printf("spacing loaded=%d\n", (a.VoxelSpacing[0] == 1.0 && a.VoxelSpacing[1] == 1.0 && a.VoxelSpacing[2] == 2.5) ? 1 : 0);
    a.SetWindowCenter(0.55f);
    a.SetWindowWidth(0.5f);
    a.SetRaymarchSteps(72.0f);
    a.Tick(0.016f);
    const tbrm_camera cam = example_camera(W, H);
    std::vector<float> before((size_t) W * H * 4), after(before.size());
    FMarginResult m;
    std::printf("nolabels refused=%d\n", a.CloseLabelBy(1.0, L, m) ? 0 : 1); // no label volume yet
    if (!a.SetLabelVolume(labels.data(), labels.size())) { std::printf("error %s\n", tbrm_last_error()); return 3; }
    if (!a.RenderLit(cam, before.data())) { std::printf("error %s\n", tbrm_last_error()); return 4; }
    const int frames = a.Stats.Frames, resets = a.Stats.Resets;

    // each call on the labels the one before left: the expected volume follows along
    std::vector<uint8_t> want = labels, got(labels.size());
    struct Call { const char* name; int op; double radius; bool unit; };
    const Call calls[] = {{"close", TBRM_MARGIN_CLOSE, 1.0, false}, {"open", TBRM_MARGIN_OPEN, 1.5, false}, {"expand", TBRM_MARGIN_EXPAND, 3.0, false},
        {"shrink", TBRM_MARGIN_SHRINK, 2.0, false}, {"expand_unit", TBRM_MARGIN_EXPAND, 2.0, true}};
    for (const Call& c : calls) {
        for (int k = 0; k < 3; ++k) a.VoxelSpacing[k] = c.unit ? 0.0 : spacing[k]; // all zero: unit spacing
        std::vector<uint8_t> S(want.size());
        for (size_t i = 0; i < want.size(); ++i) S[i] = want[i] == L;
        const std::vector<uint8_t> R = operate(S, c.op, c.unit ? unit : spacing, c.radius);
        uint64_t source = 0, result = 0, added = 0, removed = 0;
        for (size_t i = 0; i < want.size(); ++i) {
            source += S[i];
            result += R[i];
            if (R[i] && !S[i]) { ++added; want[i] = L; }
            if (S[i] && !R[i]) { ++removed; want[i] = 0; }
        }
        bool ok;
        switch (c.op) {
            case TBRM_MARGIN_CLOSE: ok = a.CloseLabelBy(c.radius, L, m); break;
            case TBRM_MARGIN_OPEN: ok = a.OpenLabelBy(c.radius, L, m); break;
            case TBRM_MARGIN_EXPAND: ok = a.ExpandLabelBy(c.radius, L, m); break;
            default: ok = a.ShrinkLabelBy(c.radius, L, m); break;
        }
        if (!ok) { std::printf("error %s\n", tbrm_last_error()); return 5; }
        if (tbrm_download_label_volume(a.RaymarchResources.Handle, got.data(), got.size()) != TBRM_OK) { std::printf("error %s\n", tbrm_last_error()); return 6; }
        size_t wrong = 0;
        for (size_t i = 0; i < got.size(); ++i) wrong += got[i] != want[i];
        std::printf("%s wrong=%zu counts=%d moved=%d\n", c.name, wrong,
                    (m.SourceVoxels == source && m.ResultVoxels == result && m.Added == added && m.Removed == removed && m.Relabelled == added + removed) ? 1 : 0,
                    added + removed > 0 ? 1 : 0);
        if (!std::strcmp(c.name, "close")) std::printf("pinhole filled=%d\n", got[at(14, 10, 9)] == L ? 1 : 0);
        if (!std::strcmp(c.name, "open")) std::printf("speck removed=%d ball_kept=%d\n", got[at(30, 10, 9)] == 0 ? 1 : 0, got[at(14, 10, 9)] == L ? 1 : 0);
        if (!std::strcmp(c.name, "expand")) // 3 world units: three voxels along x and y, one slice along z
            std::printf("quantised weights=%u,%u,%u limit=%u reach=%d,%d,%d\n", m.Weights[0], m.Weights[1], m.Weights[2], m.Limit, m.Reach[0], m.Reach[1], m.Reach[2]);
        if (!std::strcmp(c.name, "expand_unit")) std::printf("unit weights=%u,%u,%u limit=%u reach=%d,%d,%d\n", m.Weights[0], m.Weights[1], m.Weights[2], m.Limit, m.Reach[0], m.Reach[1], m.Reach[2]);
    }
    for (int k = 0; k < 3; ++k) a.VoxelSpacing[k] = spacing[k];

    // measured only: the counts of an expansion, nothing written
    if (!a.MarginLabel(TBRM_MARGIN_EXPAND, 1.0, L, m, 0, true)) { std::printf("error %s\n", tbrm_last_error()); return 7; }
    std::vector<uint8_t> again(got.size());
    tbrm_download_label_volume(a.RaymarchResources.Handle, again.data(), again.size());
    std::printf("measure added=%d relabelled=%llu unchanged=%d\n", m.Added > 0 ? 1 : 0, (unsigned long long) m.Relabelled, again == got ? 1 : 0);
    // what leaves can get a label of its own
    if (!a.ShrinkLabelBy(1.0, L, m, 9)) { std::printf("error %s\n", tbrm_last_error()); return 8; }
    tbrm_download_label_volume(a.RaymarchResources.Handle, again.data(), again.size());
    uint64_t nines = 0;
    for (uint8_t v : again) nines += v == 9;
    std::printf("erase_label removed_got_it=%d\n", (nines == m.Removed && nines > 0) ? 1 : 0);
    // radii no call can take: nothing within reach, more than the largest reach, not a number
    std::printf("refused small=%d large=%d nan=%d\n", a.ExpandLabelBy(0.5, L, m) ? 0 : 1, a.ExpandLabelBy(65.0, L, m) ? 0 : 1, a.ExpandLabelBy(std::nan(""), L, m) ? 0 : 1);

    std::printf("state frames=%d resets=%d recompute=%d\n", a.Stats.Frames - frames, a.Stats.Resets - resets, a.bRequestedRecompute ? 1 : 0);
    if (!a.RenderLit(cam, after.data())) { std::printf("error %s\n", tbrm_last_error()); return 9; }
    std::printf("frame shows_change=%d\n", std::memcmp(before.data(), after.data(), before.size() * sizeof(float)) != 0 ? 1 : 0);
    uint64_t c[4] = {0, 0, 0, 0};
    tbrm_margin_counters(a.RaymarchResources.Handle, c);
    std::printf("counters calls=%llu launches=%llu\n", (unsigned long long) c[0], (unsigned long long) c[1]);
    std::printf("OK\n");
    return 0;
}
