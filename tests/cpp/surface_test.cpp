// Drives ARaymarchVolume::ExtractLabelSurface and MeasureLabelSurface (include/tbrm_plugin.hpp, include/tbrm_surface.h): a MetaImage
// volume with anisotropic spacing and a ball and a slab as labels; the mesh is held to what the header promises, in exact arithmetic
// on the records: one vertex per active cell by a count of the cells voxel by voxel, the signed volume at the cells' centres equal
// to the label's voxel count, every edge in two or four triangles' quads, positions in the unit cube equal to the host helper's,
// unit normals. The calls request no recompute and count as no frame.
// "nohandle": what an actor without resources answers (no device needed). Otherwise argv[1] is a directory to write the volume to.
// Prints one "key value" line per check; tests/test_surface_facade.py compiles it with g++ and runs it.
#include "tbrm_volume_io.hpp" // includes tbrm_plugin.hpp

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

using namespace tbrm_plugin;

static const int nx = 40, ny = 20, nz = 19;
static size_t at(int x, int y, int z) { return ((size_t) z * ny + y) * nx + x; }

static bool in_label(const std::vector<uint8_t>& labels, int L, const int o[3], const int e[3], int x, int y, int z)
{
    return x >= o[0] && y >= o[1] && z >= o[2] && x < e[0] && y < e[1] && z < e[2] && labels[at(x, y, z)] == L;
}

// the active cells of the label inside the box [o, e), and its voxels, by loops
static void count_cells(const std::vector<uint8_t>& labels, int L, const int o[3], const int e[3], uint64_t& cells, uint64_t& voxels)
{
    cells = voxels = 0;
    for (int hz = o[2]; hz <= e[2]; ++hz)
        for (int hy = o[1]; hy <= e[1]; ++hy)
            for (int hx = o[0]; hx <= e[0]; ++hx) {
                int n = 0;
                for (int i = 0; i < 8; ++i) n += in_label(labels, L, o, e, hx - 1 + (i & 1), hy - 1 + ((i >> 1) & 1), hz - 1 + ((i >> 2) & 1));
                cells += n != 0 && n != 8;
                voxels += in_label(labels, L, o, e, hx, hy, hz);
            }
}

// what the header promises of a mesh, from the records and the triangles alone
static bool mesh_holds(const FLabelSurface& m, const int dims[3], const double spacing[3], const char* name)
{
    bool ok = m.Records.size() == m.Vertices && m.Triangles.size() == 6 * m.Quads && m.Positions.size() == 3 * m.Vertices && m.Normals.size() == 3 * m.Vertices;
    // six times the signed volume on doubled coordinates, with every vertex at its cell's centre
    long long six = 0;
    std::map<std::pair<uint32_t, uint32_t>, int> uses;
    for (size_t t = 0; ok && t + 5 < m.Triangles.size(); t += 6) {
        const uint32_t* q = &m.Triangles[t];
        ok = ok && q[0] == q[3] && q[2] == q[4]; // (q0, q1, q2), (q0, q2, q3)
        const uint32_t quad[4] = {q[0], q[1], q[2], q[5]};
        for (int i = 0; i < 4; ++i) {
            ok = ok && quad[i] < m.Vertices;
            if (!ok) break;
            const uint32_t a = quad[i], b = quad[(i + 1) % 4];
            ++uses[{a < b ? a : b, a < b ? b : a}];
        }
        for (int tri = 0; ok && tri < 2; ++tri) {
            long long p[3][3];
            for (int k = 0; k < 3; ++k)
                for (int c = 0; c < 3; ++c) p[k][c] = 2LL * m.Records[q[3 * tri + k]].cell[c] + 1;
            six += p[0][0] * (p[1][1] * p[2][2] - p[1][2] * p[2][1]) - p[0][1] * (p[1][0] * p[2][2] - p[1][2] * p[2][0]) + p[0][2] * (p[1][0] * p[2][1] - p[1][1] * p[2][0]);
        }
    }
    const bool volume = six == 48LL * (long long) m.SetVoxels;
    bool edges = true;
    for (const auto& u : uses) edges = edges && (u.second == 2 || u.second == 4);
    // positions: the host helper's, in the unit cube; normals: unit length or zero, pointing the record's way
    int32_t d32[3] = {dims[0], dims[1], dims[2]};
    float scale[3], offset[3];
    tbrm_host_surface_unit_cube(d32, scale, offset);
    std::vector<float> want(m.Positions.size());
    bool positions = tbrm_host_surface_positions(m.Records.data(), m.Records.size(), scale, offset, want.data()) == TBRM_OK && !std::memcmp(want.data(), m.Positions.data(), want.size() * sizeof(float));
    bool normals = true;
    for (size_t i = 0; ok && i < m.Records.size(); ++i) {
        const tbrm_surface_vertex& v = m.Records[i];
        double len = 0, dot = 0, raw = 0;
        for (int c = 0; c < 3; ++c) {
            len += (double) m.Normals[3 * i + c] * m.Normals[3 * i + c];
            dot += m.Normals[3 * i + c] * (v.normal[c] / spacing[c]);
            raw += std::abs((double) v.normal[c]);
            positions = positions && m.Positions[3 * i + c] >= -1.0f / (dims[c] - 1) && m.Positions[3 * i + c] <= 1.0f + 1.0f / (dims[c] - 1);
        }
        normals = normals && (raw == 0 ? len == 0 : (std::abs(len - 1.0) < 1e-5 && dot > 0));
    }
    std::printf("%s ok=%d volume=%d edges=%d positions=%d normals=%d\n", name, ok ? 1 : 0, volume ? 1 : 0, edges ? 1 : 0, positions ? 1 : 0, normals ? 1 : 0);
    return ok && volume && edges && positions && normals;
}

int main(int argc, char** argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "nohandle")) {
        ARaymarchVolume none;
        FLabelSurface m;
        const bool a = none.ExtractLabelSurface(1, m), b = none.MeasureLabelSurface(1, m);
        std::printf("nohandle extract=%d measure=%d vertices=%llu recompute=%d abi=%d\n", a ? 1 : 0, b ? 1 : 0, (unsigned long long) m.Vertices, none.bRequestedRecompute ? 1 : 0,
                    tbrm_surface_abi_version());
        return 0;
    }
    if (argc < 2) { std::printf("error: a directory to write the volume to\n"); return 1; }

    const int L = 3;
    std::vector<uint16_t> vol((size_t) nx * ny * nz);
    std::vector<uint8_t> labels(vol.size(), 0);
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                vol[at(x, y, z)] = (uint16_t) (x < 20 ? 52000 : 9000 + 37 * x);
                const int dx = x - 14, dy = y - 9, dz = z - 8;
                labels[at(x, y, z)] = dx * dx + dy * dy + dz * dz <= 50 ? L : (x >= 30 && z >= 12 ? 5 : 0); // a ball, and a slab that ends on the volume's faces
            }
    const std::string dir = argv[1];
    {
        FILE* raw = std::fopen((dir + "/surface.raw").c_str(), "wb");
        FILE* mhd = std::fopen((dir + "/surface.mhd").c_str(), "w");
        if (!raw || !mhd) { std::printf("error: cannot write to %s\n", dir.c_str()); return 1; }
        std::fwrite(vol.data(), sizeof(uint16_t), vol.size(), raw);
        std::fprintf(mhd, "ObjectType = Image\nNDims = 3\nDimSize = %d %d %d\nElementSpacing = 1 1 2.5\nElementType = MET_USHORT\nElementDataFile = surface.raw\n", nx, ny, nz);
        std::fclose(raw);
        std::fclose(mhd);
    }
    ARaymarchLight l0;
    l0.ForwardVector = FVector{1, .35, -.5}; l0.LightIntensity = 0.5f;
    ARaymarchVolume a;
    a.LightsArray = {&l0};
    if (!LoadMHDFileIntoVolumeNormalized(a, dir + "/surface.mhd")) { std::printf("error %s\n", tbrm_last_error()); return 2; }
    a.Tick(0.016f);
    FLabelSurface m;
    std::printf("nolabels refused=%d\n", a.ExtractLabelSurface(L, m) ? 0 : 1); // no label volume yet
    if (!a.SetLabelVolume(labels.data(), labels.size())) { std::printf("error %s\n", tbrm_last_error()); return 3; }
    const int frames = a.Stats.Frames, resets = a.Stats.Resets;
    a.bRequestedRecompute = false;

    const int dims[3] = {nx, ny, nz}, zero[3] = {0, 0, 0};
    const double spacing[3] = {1, 1, 2.5};
    bool all = true;
    uint64_t cells = 0, voxels = 0;
    {
        if (!a.ExtractLabelSurface(L, m)) { std::printf("error %s\n", tbrm_last_error()); return 5; }
        count_cells(labels, L, zero, dims, cells, voxels);
        std::printf("ball counts=%d\n", m.Vertices == cells && m.SetVoxels == voxels && voxels > 1000 ? 1 : 0);
        all = mesh_holds(m, dims, spacing, "ball_mesh") && m.Vertices == cells && all;
        FLabelSurface n;
        const bool measured = a.MeasureLabelSurface(L, n);
        std::printf("measure same=%d empty=%d\n", measured && n.Vertices == m.Vertices && n.Quads == m.Quads && n.SetVoxels == m.SetVoxels ? 1 : 0, n.Records.empty() && n.Triangles.empty() ? 1 : 0);
    }
    {
        if (!a.ExtractLabelSurface(5, m)) { std::printf("error %s\n", tbrm_last_error()); return 6; }
        count_cells(labels, 5, zero, dims, cells, voxels);
        std::printf("slab counts=%d faces=%d\n", m.Vertices == cells && m.SetVoxels == voxels ? 1 : 0, m.CellMax[0] == nx - 1 && m.CellMax[2] == nz - 1 && m.CellMin[1] == -1 ? 1 : 0);
        all = mesh_holds(m, dims, spacing, "slab_mesh") && all;
    }
    {
        const int o[3] = {9, 3, 5}, ext[3] = {9, 13, 7}, e[3] = {18, 16, 12};
        if (!a.ExtractLabelSurface(L, m, o, ext)) { std::printf("error %s\n", tbrm_last_error()); return 7; }
        count_cells(labels, L, o, e, cells, voxels);
        std::printf("box counts=%d\n", m.Vertices == cells && m.SetVoxels == voxels && voxels > 100 ? 1 : 0);
        all = mesh_holds(m, dims, spacing, "box_mesh") && m.Vertices == cells && all;
    }
    {
        const bool none = a.ExtractLabelSurface(77, m) && m.Vertices == 0 && m.Triangles.empty() && m.CellMax[0] == -1;
        const int o[3] = {30, 0, 0}, ext[3] = {11, 4, 4};
        const bool leaves = !a.ExtractLabelSurface(L, m, o, ext), label = !a.ExtractLabelSurface(256, m) && !a.MeasureLabelSurface(-1, m);
        std::printf("refused none=%d leaves=%d label=%d\n", none ? 1 : 0, leaves ? 1 : 0, label ? 1 : 0);
    }
    std::printf("state frames=%d resets=%d recompute=%d\n", a.Stats.Frames - frames, a.Stats.Resets - resets, a.bRequestedRecompute ? 1 : 0);
    std::vector<uint8_t> down(labels.size());
    const bool same = tbrm_download_label_volume(a.RaymarchResources.Handle, down.data(), down.size()) == TBRM_OK && down == labels;
    uint64_t c[6];
    tbrm_surface_counters(a.RaymarchResources.Handle, c);
    std::printf("labels unchanged=%d\ncounters calls=%llu\n", same ? 1 : 0, (unsigned long long) c[0]);
    std::printf(all ? "OK\n" : "FAILED\n");
    return all ? 0 : 8;
}
