// Drives ARaymarchVolume::ScissorLabel and EraseInsideLasso / KeepInsideLasso / FillInsideLasso (include/tbrm_plugin.hpp,
// include/tbrm_scissors.h): a slab of label voxels in a MetaImage volume, cut and filled under a concave lasso drawn on the example's
// camera; every label volume is compared with a restatement by loops below: the rows and the mask of the two host functions (which
// tests/test_scissors_abi.py holds to their exact restatements), every voxel by the language's own 64-bit division. The calls request
// no recompute and count as no frame.
// "nohandle": what an actor without resources answers (no device needed). Otherwise argv[1] is a directory to write the volume to.
// Prints one "key value" line per check; tests/test_scissors_facade.py compiles it with g++ and runs it.
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

static int64_t floor_div(int64_t a, int64_t b) // b > 0
{
    int64_t q = a / b;
    if (a % b != 0 && a < 0) --q;
    return q;
}

// M by loops: the voxels whose centre the rows put on a set pixel of the mask, within the depth range
static std::vector<uint8_t> under_lasso(const tbrm_scissors_projection& p, const std::vector<uint32_t>& mask)
{
    std::vector<uint8_t> M((size_t) nx * ny * nz, 0);
    const size_t row_words = (size_t) ((p.width + 31) / 32);
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const int64_t U = p.u[0] * x + p.u[1] * y + p.u[2] * z + p.u[3], V = p.v[0] * x + p.v[1] * y + p.v[2] * z + p.v[3], W = p.w[0] * x + p.w[1] * y + p.w[2] * z + p.w[3];
                if (W <= 0 || W < p.w_min || W > p.w_max) continue;
                const int64_t px = floor_div(U, W), py = floor_div(V, W);
                if (px < 0 || px >= p.width || py < 0 || py >= p.height) continue;
                M[at(x, y, z)] = (mask[(size_t) py * row_words + (size_t) (px >> 5)] >> (px & 31)) & 1u;
            }
    return M;
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
    const std::vector<double> lasso = {10.0, 6.0, 40.5, 9.25, 27.0, 20.0, 42.0, 34.0, 14.0, 31.5, 20.0, 19.0}; // concave
    if (argc > 1 && !std::strcmp(argv[1], "nohandle")) {
        ARaymarchVolume none;
        FScissorsResult m;
        const tbrm_camera cam = example_camera(48, 40);
        const bool a = none.ScissorLabel(cam, lasso, TBRM_SCISSORS_ERASE_INSIDE, 1, 0.0, HUGE_VAL, m), b = none.EraseInsideLasso(cam, lasso, 1, m),
                   c = none.KeepInsideLasso(cam, lasso, 1, m), d = none.FillInsideLasso(cam, lasso, 1, m);
        std::printf("nohandle scissor=%d erase=%d keep=%d fill=%d removed=%llu recompute=%d abi=%d\n", a ? 1 : 0, b ? 1 : 0, c ? 1 : 0, d ? 1 : 0,
                    (unsigned long long) m.Removed, none.bRequestedRecompute ? 1 : 0, tbrm_scissors_abi_version());
        return 0;
    }
    if (argc < 2) { std::printf("error: a directory to write the volume to\n"); return 1; }

    const int W = 48, H = 40, L = 3;
    std::vector<uint16_t> vol((size_t) nx * ny * nz);
    std::vector<uint8_t> labels(vol.size(), 0);
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const bool slab = z >= 5 && z < 14 && x >= 4 && x < 36;
                vol[at(x, y, z)] = (uint16_t) (slab ? 52000 : 9000 + 37 * x);
                labels[at(x, y, z)] = slab ? L : ((x + y + z) % 11 == 0 ? 5 : 0); // a second label scattered around
            }
    const std::string dir = argv[1];
    {
        FILE* raw = std::fopen((dir + "/slab.raw").c_str(), "wb");
        FILE* mhd = std::fopen((dir + "/slab.mhd").c_str(), "w");
        if (!raw || !mhd) { std::printf("error: cannot write to %s\n", dir.c_str()); return 1; }
        std::fwrite(vol.data(), sizeof(uint16_t), vol.size(), raw);
        std::fprintf(mhd, "ObjectType = Image\nNDims = 3\nDimSize = %d %d %d\nElementSpacing = 1 1 2.5\nElementType = MET_USHORT\nElementDataFile = slab.raw\n", nx, ny, nz);
        std::fclose(raw);
        std::fclose(mhd);
    }
    ARaymarchLight l0;
    l0.ForwardVector = FVector{1, .35, -.5}; l0.LightIntensity = 0.5f;
    ARaymarchVolume a;
    a.LightsArray = {&l0};
    if (!LoadMHDFileIntoVolumeNormalized(a, dir + "/slab.mhd")) { std::printf("error %s\n", tbrm_last_error()); return 2; }
    a.SetWindowCenter(0.55f);
    a.SetWindowWidth(0.5f);
    a.SetRaymarchSteps(72.0f);
    a.Tick(0.016f);
    const tbrm_camera cam = example_camera(W, H);
    std::vector<float> before((size_t) W * H * 4), after(before.size());
    FScissorsResult m;
    std::printf("nolabels refused=%d\n", a.EraseInsideLasso(cam, lasso, L, m) ? 0 : 1); // no label volume yet
    if (!a.SetLabelVolume(labels.data(), labels.size())) { std::printf("error %s\n", tbrm_last_error()); return 3; }
    if (!a.RenderLit(cam, before.data())) { std::printf("error %s\n", tbrm_last_error()); return 4; }
    const int frames = a.Stats.Frames, resets = a.Stats.Resets;

    // the rows and the mask the facade must have used
    const tbrm_world_params world = a.WorldParameters.abi();
    const int32_t dims[3] = {nx, ny, nz};
    std::vector<uint32_t> mask((size_t) ((W + 31) / 32) * H);
    if (tbrm_host_scissors_polygon(lasso.data(), lasso.size() / 2, W, H, mask.data(), mask.size()) != TBRM_OK) { std::printf("error %s\n", tbrm_last_error()); return 5; }
    uint64_t pixels = 0;
    for (uint32_t w : mask) pixels += (uint64_t) __builtin_popcount(w);
    tbrm_scissors_projection whole{}, near{};
    const double centre = (world.volume_transform.translation.x - cam.position.x) * cam.forward.x + (world.volume_transform.translation.y - cam.position.y) * cam.forward.y +
                          (world.volume_transform.translation.z - cam.position.z) * cam.forward.z; // the depth of the volume's centre
    if (tbrm_host_scissors_projection(dims, &world, &cam, 0.0, HUGE_VAL, &whole) != TBRM_OK || tbrm_host_scissors_projection(dims, &world, &cam, 0.0, centre, &near) != TBRM_OK) {
        std::printf("error %s\n", tbrm_last_error());
        return 6;
    }

    // each call on the labels the one before left: the expected volume follows along
    std::vector<uint8_t> want = labels, got(labels.size());
    struct Call { const char* name; int op; bool deep; };
    const Call calls[] = {{"erase", TBRM_SCISSORS_ERASE_INSIDE, true}, {"fill", TBRM_SCISSORS_FILL_INSIDE, true}, {"near", TBRM_SCISSORS_ERASE_INSIDE, false},
        {"keep", TBRM_SCISSORS_ERASE_OUTSIDE, true}, {"fill_outside", TBRM_SCISSORS_FILL_OUTSIDE, true}};
    for (const Call& c : calls) {
        const std::vector<uint8_t> M = under_lasso(c.deep ? whole : near, mask);
        uint64_t source = 0, result = 0, added = 0, removed = 0, in_M = 0;
        for (size_t i = 0; i < want.size(); ++i) {
            const bool S = want[i] == L, R = c.op == TBRM_SCISSORS_ERASE_INSIDE ? S && !M[i] : (c.op == TBRM_SCISSORS_ERASE_OUTSIDE ? S && M[i] : (c.op == TBRM_SCISSORS_FILL_INSIDE ? S || M[i] : S || !M[i]));
            source += S; result += R; in_M += M[i];
            if (R && !S) { ++added; want[i] = L; }
            if (S && !R) { ++removed; want[i] = 0; }
        }
        bool ok;
        if (!c.deep) ok = a.ScissorLabel(cam, lasso, c.op, L, 0.0, centre, m);
        else if (c.op == TBRM_SCISSORS_ERASE_INSIDE) ok = a.EraseInsideLasso(cam, lasso, L, m);
        else if (c.op == TBRM_SCISSORS_ERASE_OUTSIDE) ok = a.KeepInsideLasso(cam, lasso, L, m);
        else if (c.op == TBRM_SCISSORS_FILL_INSIDE) ok = a.FillInsideLasso(cam, lasso, L, m);
        else ok = a.ScissorLabel(cam, lasso, c.op, L, 0.0, HUGE_VAL, m);
        if (!ok) { std::printf("error %s\n", tbrm_last_error()); return 7; }
        if (tbrm_download_label_volume(a.RaymarchResources.Handle, got.data(), got.size()) != TBRM_OK) { std::printf("error %s\n", tbrm_last_error()); return 8; }
        size_t wrong = 0;
        for (size_t i = 0; i < got.size(); ++i) wrong += got[i] != want[i];
        std::printf("%s wrong=%zu counts=%d moved=%d cut=%d pixels=%d\n", c.name, wrong,
                    (m.SourceVoxels == source && m.ResultVoxels == result && m.Added == added && m.Removed == removed && m.Relabelled == added + removed) ? 1 : 0,
                    added + removed > 0 ? 1 : 0, (in_M > 0 && in_M < want.size()) ? 1 : 0, m.MaskPixels == pixels ? 1 : 0);
    }

    // measured only: the counts, nothing written
    if (!a.ScissorLabel(cam, lasso, TBRM_SCISSORS_ERASE_INSIDE, L, 0.0, HUGE_VAL, m, 0, true)) { std::printf("error %s\n", tbrm_last_error()); return 9; }
    std::vector<uint8_t> again(got.size());
    tbrm_download_label_volume(a.RaymarchResources.Handle, again.data(), again.size());
    std::printf("measure removed=%d relabelled=%llu unchanged=%d\n", m.Removed > 0 ? 1 : 0, (unsigned long long) m.Relabelled, again == got ? 1 : 0);
    // what leaves can get a label of its own
    if (!a.ScissorLabel(cam, lasso, TBRM_SCISSORS_ERASE_INSIDE, L, 0.0, HUGE_VAL, m, 9)) { std::printf("error %s\n", tbrm_last_error()); return 10; }
    tbrm_download_label_volume(a.RaymarchResources.Handle, again.data(), again.size());
    uint64_t nines = 0;
    for (uint8_t v : again) nines += v == 9;
    std::printf("erase_label removed_got_it=%d\n", (nines == m.Removed && nines > 0) ? 1 : 0);
    // what no call can take: two points, an odd number of coordinates, a label or an operator out of range, depths the wrong way round
    const std::vector<double> two = {1.0, 1.0, 9.0, 9.0}, odd = {1.0, 1.0, 9.0, 9.0, 4.0, 20.0, 7.0};
    std::printf("refused two=%d odd=%d label=%d op=%d depth=%d\n", a.EraseInsideLasso(cam, two, L, m) ? 0 : 1, a.EraseInsideLasso(cam, odd, L, m) ? 0 : 1,
                a.EraseInsideLasso(cam, lasso, 256, m) ? 0 : 1, a.ScissorLabel(cam, lasso, 4, L, 0.0, HUGE_VAL, m) ? 0 : 1, a.ScissorLabel(cam, lasso, 0, L, 9.0, 3.0, m) ? 0 : 1);

    std::printf("state frames=%d resets=%d recompute=%d\n", a.Stats.Frames - frames, a.Stats.Resets - resets, a.bRequestedRecompute ? 1 : 0);
    if (!a.RenderLit(cam, after.data())) { std::printf("error %s\n", tbrm_last_error()); return 11; }
    std::printf("frame shows_change=%d\n", std::memcmp(before.data(), after.data(), before.size() * sizeof(float)) != 0 ? 1 : 0);
    uint64_t c[4] = {0, 0, 0, 0};
    tbrm_scissors_counters(a.RaymarchResources.Handle, c);
    std::printf("counters calls=%llu\n", (unsigned long long) c[0]);
    std::printf("OK\n");
    return 0;
}
