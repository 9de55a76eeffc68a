// Drives ARaymarchVolume::MorphLabel and DilateLabel / ErodeLabel / OpenLabel / CloseLabel (include/tbrm_plugin.hpp,
// include/tbrm_morphology.h): two blocks of one label joined by a one-voxel bridge, one of them with a pinhole — closing fills the
// pinhole, opening cuts the bridge, dilating and eroding move the surface; every label volume is compared with a brute-force
// restatement below. The calls request no recompute and count as no frame.
// "nohandle": what an actor without resources answers (no device needed).
// Prints one "key value" line per check; tests/test_morph_facade.py compiles it with g++ and runs it.
#include "tbrm_volume_io.hpp" // includes tbrm_plugin.hpp

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace tbrm_plugin;

static const int nx = 40, ny = 20, nz = 19;
static size_t at(int x, int y, int z) { return ((size_t) z * ny + y) * nx + x; }

// one unit step over the whole volume: a dilation (outside counts as unset) or an erosion (outside counts as set)
static std::vector<uint8_t> step(const std::vector<uint8_t>& m, int connectivity, bool erode)
{
    std::vector<uint8_t> out(m.size());
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                bool any = false, all = true;
                for (int dz = -1; dz <= 1; ++dz)
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) {
                            if (connectivity == 6 && (dx != 0) + (dy != 0) + (dz != 0) > 1) continue;
                            const int X = x + dx, Y = y + dy, Z = z + dz;
                            const bool in = X >= 0 && X < nx && Y >= 0 && Y < ny && Z >= 0 && Z < nz;
                            const bool v = in ? m[at(X, Y, Z)] != 0 : erode;
                            any = any || v;
                            all = all && v;
                        }
                out[at(x, y, z)] = erode ? all : any;
            }
    return out;
}

static std::vector<uint8_t> operate(std::vector<uint8_t> m, int op, int radius, int connectivity)
{
    const bool first_erodes = op == TBRM_MORPH_ERODE || op == TBRM_MORPH_OPEN;
    for (int i = 0; i < radius; ++i) m = step(m, connectivity, first_erodes);
    if (op == TBRM_MORPH_OPEN || op == TBRM_MORPH_CLOSE)
        for (int i = 0; i < radius; ++i) m = step(m, connectivity, !first_erodes);
    return m;
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
        FMorphResult m;
        const bool a = none.MorphLabel(TBRM_MORPH_CLOSE, 2, 1, m), b = none.DilateLabel(1, 1, m), c = none.ErodeLabel(1, 1, m), d = none.OpenLabel(1, 1, m),
                   e = none.CloseLabel(1, 1, m);
        std::printf("nohandle morph=%d dilate=%d erode=%d open=%d close=%d added=%llu recompute=%d abi=%d\n", a ? 1 : 0, b ? 1 : 0, c ? 1 : 0, d ? 1 : 0,
                    e ? 1 : 0, (unsigned long long) m.Added, none.bRequestedRecompute ? 1 : 0, tbrm_morph_abi_version());
        return 0;
    }

    const int W = 48, H = 40, L = 3;
    std::vector<uint16_t> vol((size_t) nx * ny * nz);
    std::vector<uint8_t> labels(vol.size(), 0);
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const bool block = y >= 4 && y < 14 && z >= 4 && z < 14 && ((x >= 4 && x < 14) || (x >= 20 && x < 30));
                const bool bridge = y == 8 && z == 8 && x >= 14 && x < 20;
                vol[at(x, y, z)] = (uint16_t) (block || bridge ? 52000 : 9000 + 37 * x);
                labels[at(x, y, z)] = (block || bridge) ? L : ((x + y + z) % 11 == 0 ? 5 : 0); // a second label scattered around
            }
    labels[at(8, 8, 8)] = 0; // the pinhole
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
    FMorphResult m;
    std::printf("nolabels refused=%d\n", a.CloseLabel(1, L, m) ? 0 : 1); // no label volume yet
    if (!a.SetLabelVolume(labels.data(), labels.size())) { std::printf("error %s\n", tbrm_last_error()); return 3; }
    if (!a.RenderLit(cam, before.data())) { std::printf("error %s\n", tbrm_last_error()); return 4; }
    const int frames = a.Stats.Frames, resets = a.Stats.Resets;

    // each call on the labels the one before left: the expected volume follows along
    std::vector<uint8_t> want = labels, got(labels.size());
    struct Call { const char* name; int op, radius, connectivity; };
    const Call calls[] = {{"close", TBRM_MORPH_CLOSE, 1, 6}, {"open", TBRM_MORPH_OPEN, 1, 6}, {"dilate", TBRM_MORPH_DILATE, 2, 26}, {"erode", TBRM_MORPH_ERODE, 3, 6},
        {"close26", TBRM_MORPH_CLOSE, 2, 26}};
    for (const Call& c : calls) {
        std::vector<uint8_t> S(want.size());
        for (size_t i = 0; i < want.size(); ++i) S[i] = want[i] == L;
        const std::vector<uint8_t> R = operate(S, c.op, c.radius, c.connectivity);
        uint64_t source = 0, result = 0, added = 0, removed = 0;
        for (size_t i = 0; i < want.size(); ++i) {
            source += S[i];
            result += R[i];
            if (R[i] && !S[i]) { ++added; want[i] = L; }
            if (S[i] && !R[i]) { ++removed; want[i] = 0; }
        }
        bool ok;
        switch (c.op) { // the named forms are the 6-connected default; the others go through MorphLabel
            case TBRM_MORPH_CLOSE: ok = c.connectivity == 6 ? a.CloseLabel(c.radius, L, m) : a.CloseLabel(c.radius, L, m, 26); break;
            case TBRM_MORPH_OPEN: ok = a.OpenLabel(c.radius, L, m); break;
            case TBRM_MORPH_DILATE: ok = a.DilateLabel(c.radius, L, m, c.connectivity); break;
            default: ok = a.ErodeLabel(c.radius, L, m); break;
        }
        if (!ok) { std::printf("error %s\n", tbrm_last_error()); return 5; }
        if (tbrm_download_label_volume(a.RaymarchResources.Handle, got.data(), got.size()) != TBRM_OK) { std::printf("error %s\n", tbrm_last_error()); return 6; }
        size_t wrong = 0;
        for (size_t i = 0; i < got.size(); ++i) wrong += got[i] != want[i];
        std::printf("%s wrong=%zu counts=%d moved=%d\n", c.name, wrong,
                    (m.SourceVoxels == source && m.ResultVoxels == result && m.Added == added && m.Removed == removed && m.Relabelled == added + removed) ? 1 : 0,
                    added + removed > 0 ? 1 : 0);
        if (!std::strcmp(c.name, "close")) std::printf("pinhole filled=%d\n", got[at(8, 8, 8)] == L ? 1 : 0);
        if (!std::strcmp(c.name, "open")) std::printf("bridge cut=%d blocks_kept=%d\n", got[at(16, 8, 8)] == 0 ? 1 : 0, (got[at(5, 5, 5)] == L && got[at(25, 9, 9)] == L) ? 1 : 0);
    }

    // measured only: the counts of a dilation, nothing written
    if (!a.MorphLabel(TBRM_MORPH_DILATE, 1, L, m, 6, 0, true)) { std::printf("error %s\n", tbrm_last_error()); return 7; }
    std::vector<uint8_t> again(got.size());
    tbrm_download_label_volume(a.RaymarchResources.Handle, again.data(), again.size());
    std::printf("measure added=%d relabelled=%llu unchanged=%d\n", m.Added > 0 ? 1 : 0, (unsigned long long) m.Relabelled, again == got ? 1 : 0);
    // what leaves can get a label of its own
    if (!a.MorphLabel(TBRM_MORPH_ERODE, 1, L, m, 6, 9)) { std::printf("error %s\n", tbrm_last_error()); return 8; }
    tbrm_download_label_volume(a.RaymarchResources.Handle, again.data(), again.size());
    uint64_t nines = 0;
    for (uint8_t v : again) nines += v == 9;
    std::printf("erase_label removed_got_it=%d\n", (nines == m.Removed && nines > 0) ? 1 : 0);

    std::printf("state frames=%d resets=%d recompute=%d\n", a.Stats.Frames - frames, a.Stats.Resets - resets, a.bRequestedRecompute ? 1 : 0);
    if (!a.RenderLit(cam, after.data())) { std::printf("error %s\n", tbrm_last_error()); return 9; }
    std::printf("frame shows_change=%d\n", std::memcmp(before.data(), after.data(), before.size() * sizeof(float)) != 0 ? 1 : 0);
    uint64_t c[4] = {0, 0, 0, 0};
    tbrm_morph_counters(a.RaymarchResources.Handle, c);
    std::printf("counters calls=%llu launches=%llu\n", (unsigned long long) c[0], (unsigned long long) c[1]);
    std::printf("OK\n");
    return 0;
}
