// Drives ARaymarchVolume::PaintLabel, EraseLabel and PaintAlongHits (include/tbrm_plugin.hpp, include/tbrm_paint.h): a MetaImage
// volume with anisotropic spacing, a ball, a stroke and an erasure painted into its labels, a gated stroke, and a stroke along hits;
// every label volume is compared with a restatement by loops below: the weights and the limit of tbrm_host_paint_brush (which
// tests/test_paint_abi.py holds to the margin's), the distance rule of the header voxel by voxel in 64-bit integers. The calls
// request no recompute and count as no frame.
// "nohandle": what an actor without resources answers (no device needed). Otherwise argv[1] is a directory to write the volume to.
// Prints one "key value" line per check; tests/test_paint_facade.py compiles it with g++ and runs it.
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

// the header's rule for one voxel and one segment (values far below the bounds: plain 64-bit products)
static bool within(const int32_t* a, const int32_t* b, const uint32_t w[3], uint32_t limit, int x, int y, int z)
{
    const int64_t v[3] = {8 * x, 8 * y, 8 * z};
    int64_t dd = 0, de = 0, ee = 0, bb = 0;
    for (int c = 0; c < 3; ++c) {
        const int64_t d = b[c] - a[c], e = v[c] - a[c], f = v[c] - b[c];
        dd += w[c] * d * d; de += w[c] * d * e; ee += w[c] * e * e; bb += w[c] * f * f;
    }
    if (de <= 0) return ee <= (int64_t) limit;
    if (de >= dd) return bb <= (int64_t) limit;
    return ee * dd - de * de <= (int64_t) limit * dd;
}

// M by loops: the voxels within some segment of the stroke
static std::vector<uint8_t> stamp(const std::vector<int32_t>& pts, const uint32_t w[3], uint32_t limit)
{
    std::vector<uint8_t> M((size_t) nx * ny * nz, 0);
    const size_t n = pts.size() / 3, segs = n > 1 ? n - 1 : 1;
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x)
                for (size_t k = 0; k < segs && !M[at(x, y, z)]; ++k) M[at(x, y, z)] = within(&pts[3 * k], &pts[3 * (n > 1 ? k + 1 : k)], w, limit, x, y, z);
    return M;
}

int main(int argc, char** argv)
{
    const std::vector<int32_t> ball = {8 * 20, 8 * 10, 8 * 9}, stroke = {30, 20, 40, 150, 100, 60, 290, 120, 110, 350, 60, 130};
    if (argc > 1 && !std::strcmp(argv[1], "nohandle")) {
        ARaymarchVolume none;
        FPaintResult m;
        FVolumeHit h;
        h.bHit = true;
        const bool a = none.PaintLabel(ball, 3.0, 1, m), b = none.EraseLabel(stroke, 3.0, 1, m), c = none.PaintAlongHits({h, h}, 3.0, 1, m), d = none.PaintStroke(TBRM_PAINT_PAINT, ball, 3.0, 1, m);
        std::printf("nohandle paint=%d erase=%d hits=%d stroke=%d added=%llu recompute=%d abi=%d\n", a ? 1 : 0, b ? 1 : 0, c ? 1 : 0, d ? 1 : 0, (unsigned long long) m.Added,
                    none.bRequestedRecompute ? 1 : 0, tbrm_paint_abi_version());
        return 0;
    }
    if (argc < 2) { std::printf("error: a directory to write the volume to\n"); return 1; }

    const int W = 48, H = 40, L = 3;
    std::vector<uint16_t> vol((size_t) nx * ny * nz);
    std::vector<uint8_t> labels(vol.size(), 0);
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                vol[at(x, y, z)] = (uint16_t) (x < 20 ? 52000 : 9000 + 37 * x);
                labels[at(x, y, z)] = (x + y + z) % 11 == 0 ? 5 : 0; // a second label scattered around
            }
    const std::string dir = argv[1];
    {
        FILE* raw = std::fopen((dir + "/paint.raw").c_str(), "wb");
        FILE* mhd = std::fopen((dir + "/paint.mhd").c_str(), "w");
        if (!raw || !mhd) { std::printf("error: cannot write to %s\n", dir.c_str()); return 1; }
        std::fwrite(vol.data(), sizeof(uint16_t), vol.size(), raw);
        std::fprintf(mhd, "ObjectType = Image\nNDims = 3\nDimSize = %d %d %d\nElementSpacing = 1 1 2.5\nElementType = MET_USHORT\nElementDataFile = paint.raw\n", nx, ny, nz);
        std::fclose(raw);
        std::fclose(mhd);
    }
    ARaymarchLight l0;
    l0.ForwardVector = FVector{1, .35, -.5}; l0.LightIntensity = 0.5f;
    ARaymarchVolume a;
    a.LightsArray = {&l0};
    if (!LoadMHDFileIntoVolumeNormalized(a, dir + "/paint.mhd")) { std::printf("error %s\n", tbrm_last_error()); return 2; }
    a.SetWindowCenter(0.55f);
    a.SetWindowWidth(0.5f);
    a.SetRaymarchSteps(72.0f);
    a.Tick(0.016f);
    tbrm_camera cam{};
    {
        cam.position = FVector{-145, -95, 80};
        const double fl = std::sqrt(145.0 * 145 + 95.0 * 95 + 80.0 * 80);
        cam.forward = FVector{145 / fl, 95 / fl, -80 / fl};
        const double rl = std::sqrt(cam.forward.x * cam.forward.x + cam.forward.y * cam.forward.y);
        cam.right = FVector{cam.forward.y / rl, -cam.forward.x / rl, 0};
        cam.up = FVector{cam.right.y * cam.forward.z - cam.right.z * cam.forward.y, cam.right.z * cam.forward.x - cam.right.x * cam.forward.z,
            cam.right.x * cam.forward.y - cam.right.y * cam.forward.x};
        cam.tan_half_fov_y = std::tan(25.0 * 3.14159265358979323846 / 180.0);
        cam.tan_half_fov_x = cam.tan_half_fov_y * W / H;
        cam.width = W;
        cam.height = H;
    }
    std::vector<float> before((size_t) W * H * 4), after(before.size());
    FPaintResult m;
    std::printf("nolabels refused=%d\n", a.PaintLabel(ball, 3.0, L, m) ? 0 : 1); // no label volume yet
    if (!a.SetLabelVolume(labels.data(), labels.size())) { std::printf("error %s\n", tbrm_last_error()); return 3; }
    if (!a.RenderLit(cam, before.data())) { std::printf("error %s\n", tbrm_last_error()); return 4; }
    const int frames = a.Stats.Frames, resets = a.Stats.Resets;

    // the brush the facade must have used: the volume's spacing (1, 1, 2.5) and a radius of 3
    const double spacing[3] = {a.VoxelSpacing[0], a.VoxelSpacing[1], a.VoxelSpacing[2]};
    uint32_t w[3], limit = 0;
    if (tbrm_host_paint_brush(spacing, 3.0, w, &limit) != TBRM_OK) { std::printf("error %s\n", tbrm_last_error()); return 5; }
    std::printf("brush spacing=%d weights=%u,%u,%u limit=%u\n", (spacing[0] == 1.0 && spacing[2] == 2.5) ? 1 : 0, w[0], w[1], w[2], limit);

    // each call on the labels the one before left: the expected volume follows along
    std::vector<uint8_t> want = labels, got(labels.size());
    struct Call { const char* name; bool erase; const std::vector<int32_t>* pts; };
    const Call calls[] = {{"ball", false, &ball}, {"stroke", false, &stroke}, {"erase", true, &ball}};
    for (const Call& c : calls) {
        const std::vector<uint8_t> M = stamp(*c.pts, w, limit);
        uint64_t added = 0, removed = 0, in_M = 0;
        for (size_t i = 0; i < want.size(); ++i) {
            const bool S = want[i] == L, R = c.erase ? S && !M[i] : S || M[i];
            in_M += M[i];
            if (R && !S) { ++added; want[i] = L; }
            if (S && !R) { ++removed; want[i] = 0; }
        }
        if (!(c.erase ? a.EraseLabel(*c.pts, 3.0, L, m) : a.PaintLabel(*c.pts, 3.0, L, m))) { std::printf("error %s\n", tbrm_last_error()); return 7; }
        if (tbrm_download_label_volume(a.RaymarchResources.Handle, got.data(), got.size()) != TBRM_OK) { std::printf("error %s\n", tbrm_last_error()); return 8; }
        size_t wrong = 0;
        for (size_t i = 0; i < got.size(); ++i) wrong += got[i] != want[i];
        std::printf("%s wrong=%zu counts=%d moved=%d brush=%d\n", c.name, wrong,
                    (m.StampVoxels == in_M && m.Added == added && m.Removed == removed && m.Relabelled == added + removed && m.Points == (int) (c.pts->size() / 3) &&
                     m.Segments == (m.Points > 1 ? m.Points - 1 : 1) && m.Launches == 3) ? 1 : 0,
                    added + removed > 0 ? 1 : 0, (m.Weights[0] == w[0] && m.Weights[2] == w[2] && m.Limit == limit) ? 1 : 0);
    }

    // gated, boxed, over label 0 only, measured first: the counts, nothing written
    FPaintOptions o;
    o.bGate = true;
    o.Lo = 40000.0; o.Hi = 65535.0; // the bright half, x < 20, in the loader's codes (it stretches the range: 52000 -> 65535)
    o.Writable = {0};
    o.Origin[1] = 4; o.Extent[0] = nx; o.Extent[1] = 12; o.Extent[2] = nz;
    o.bMeasureOnly = true;
    if (!a.PaintLabel(stroke, 3.0, 7, m, o)) { std::printf("error %s\n", tbrm_last_error()); return 9; }
    std::vector<uint8_t> again(got.size());
    tbrm_download_label_volume(a.RaymarchResources.Handle, again.data(), again.size());
    const uint64_t measured = m.Added;
    std::printf("measure added=%d relabelled=%llu unchanged=%d\n", m.Added > 0 ? 1 : 0, (unsigned long long) m.Relabelled, again == got ? 1 : 0);
    o.bMeasureOnly = false;
    if (!a.PaintLabel(stroke, 3.0, 7, m, o)) { std::printf("error %s\n", tbrm_last_error()); return 10; }
    tbrm_download_label_volume(a.RaymarchResources.Handle, again.data(), again.size());
    {
        const std::vector<uint8_t> M = stamp(stroke, w, limit);
        size_t wrong = 0;
        uint64_t sevens = 0;
        for (int z = 0; z < nz; ++z)
            for (int y = 0; y < ny; ++y)
                for (int x = 0; x < nx; ++x) {
                    const size_t i = at(x, y, z);
                    const bool joins = M[i] && x < 20 && y >= 4 && y < 16 && got[i] == 0;
                    wrong += again[i] != (joins ? 7 : got[i]);
                    sevens += again[i] == 7;
                }
        std::printf("gated wrong=%zu added=%d\n", wrong, (m.Added == sevens && sevens == measured && sevens > 0) ? 1 : 0);
    }

    // along hits: unit-cube positions in their order, records without a hit passed over; the stroke is tbrm_host_paint_stroke's
    {
        std::vector<FVolumeHit> hits(5);
        const float uvw[5][3] = {{0.1f, 0.2f, 0.5f}, {0.9f, 0.9f, 0.9f}, {0.5f, 0.6f, 0.5f}, {0.5f, 0.6f, 0.5f}, {0.8f, 0.3f, 0.2f}};
        for (int i = 0; i < 5; ++i) { hits[i].bHit = i != 1; for (int c = 0; c < 3; ++c) hits[i].Uvw[c] = uvw[i][c]; }
        const int32_t dims[3] = {nx, ny, nz};
        const float kept[9] = {0.1f, 0.2f, 0.5f, 0.5f, 0.6f, 0.5f, 0.8f, 0.3f, 0.2f};
        std::vector<int32_t> pts(9);
        size_t n = 0;
        if (tbrm_host_paint_stroke(dims, kept, 3, w, pts.data(), 3, &n) != TBRM_OK || n != 3) { std::printf("error %s\n", tbrm_last_error()); return 11; }
        const std::vector<uint8_t> M = stamp(pts, w, limit);
        std::vector<uint8_t> base = again;
        if (!a.PaintAlongHits(hits, 3.0, 9, m)) { std::printf("error %s\n", tbrm_last_error()); return 12; }
        tbrm_download_label_volume(a.RaymarchResources.Handle, again.data(), again.size());
        size_t wrong = 0;
        for (size_t i = 0; i < again.size(); ++i) wrong += again[i] != (M[i] ? 9 : base[i]);
        FVolumeHit miss;
        FPaintResult none;
        std::printf("hits wrong=%zu points=%d segments=%d added=%d nohit=%d\n", wrong, m.Points, m.Segments, m.Added > 0 ? 1 : 0, a.PaintAlongHits({miss, miss}, 3.0, 9, none) ? 0 : 1);
        // a picked point of the surface carries its unit-cube position
        FVolumeHit pick;
        if (!a.PickVolume(cam, W / 2, H / 2, 0.3f, pick)) { std::printf("error %s\n", tbrm_last_error()); return 13; }
        bool inside = pick.bHit;
        for (float u : pick.Uvw) inside = inside && u >= 0.0f && u <= 1.0f;
        std::printf("pick hit=%d uvw=%d painted=%d\n", pick.bHit ? 1 : 0, inside ? 1 : 0, (a.PaintAlongHits({pick}, 2.0, 11, m) && m.Added > 0 && m.Segments == 1) ? 1 : 0);
    }
    // what no call can take: no point, a number of coordinates that is no multiple of 3, a label or a radius out of range
    const std::vector<int32_t> nothing, ragged = {1, 2, 3, 4};
    std::printf("refused none=%d ragged=%d label=%d radius=%d op=%d\n", a.PaintLabel(nothing, 3.0, L, m) ? 0 : 1, a.PaintLabel(ragged, 3.0, L, m) ? 0 : 1,
                a.PaintLabel(ball, 3.0, 256, m) ? 0 : 1, a.PaintLabel(ball, 70.0, L, m) ? 0 : 1, a.PaintStroke(2, ball, 3.0, L, m) ? 0 : 1);

    std::printf("state frames=%d resets=%d recompute=%d\n", a.Stats.Frames - frames, a.Stats.Resets - resets, a.bRequestedRecompute ? 1 : 0);
    if (!a.RenderLit(cam, after.data())) { std::printf("error %s\n", tbrm_last_error()); return 14; }
    std::printf("frame shows_change=%d\n", std::memcmp(before.data(), after.data(), before.size() * sizeof(float)) != 0 ? 1 : 0);
    uint64_t c[4] = {0, 0, 0, 0};
    tbrm_paint_counters(a.RaymarchResources.Handle, c);
    std::printf("counters calls=%llu\n", (unsigned long long) c[0]);
    std::printf("OK\n");
    return 0;
}
