// surface_plan_test.cpp — tbrm_surface_plan.h (what the kernels of tbrm_surface_kernels.hip compute) as a stand-alone host program:
// no device, no handle. Built and run under -fsanitize=address,undefined by tests/test_surface_abi.py.
//
// For every volume of 1, 7, 8, 9 or 17 voxels per axis, sets and boxes: the boards of the set are built as k_morph_load builds them,
// the blocks are counted, scanned and emitted with the plan's functions the way the kernels deal them out (a slice at a time, a cell
// at a time), under skipping and without, and the mesh is held to a voxel-by-voxel extraction that knows no boards and no bits.
#include "../../tbraymarcherplugin_amd/csrc/tbrm_surface_plan.h"

#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>

using namespace tbrm;

static int failures = 0;
#define CHECK(cond, ...)                                                                                                       \
    do {                                                                                                                       \
        if (!(cond)) {                                                                                                         \
            if (++failures <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                                                      \
    } while (0)

struct Volume {
    int dims[3];
    std::vector<uint8_t> set; // dense, x fastest
    bool at(int x, int y, int z) const { return x >= 0 && y >= 0 && z >= 0 && x < dims[0] && y < dims[1] && z < dims[2] && set[((size_t) z * dims[1] + y) * dims[0] + x]; }
};

struct Mesh {
    std::vector<SurfaceVertex> vertices;
    std::vector<uint32_t> indices;
    std::vector<float> positions;
    uint64_t set_voxels = 0, quads_axis[3] = {0, 0, 0};
    int skipped = 0, evaluated = 0;
};

// ---- the answer, voxel by voxel ----------------------------------------------------------------------------------------------------------
static bool in_s(const Volume& v, const VoxelBox& b, int x, int y, int z)
{
    return x >= b.origin[0] && x < b.end[0] && y >= b.origin[1] && y < b.end[1] && z >= b.origin[2] && z < b.end[2] && v.at(x, y, z);
}

static bool cell_record(const Volume& v, const VoxelBox& b, const int h[3], SurfaceVertex& out)
{
    bool in[8];
    int corners = 0;
    for (int i = 0; i < 8; ++i) {
        in[i] = in_s(v, b, h[0] - 1 + (i & 1), h[1] - 1 + ((i >> 1) & 1), h[2] - 1 + ((i >> 2) & 1));
        corners |= (int) in[i] << i;
    }
    if (corners == 0 || corners == 255) return false;
    int edges = 0, sum[3] = {0, 0, 0}, normal[3] = {0, 0, 0};
    for (int i = 0; i < 8; ++i)
        for (int j = i + 1; j < 8; ++j) {
            const int d = i ^ j;
            if (d != 1 && d != 2 && d != 4) continue;
            if (in[i] == in[j]) continue;
            ++edges;
            for (int a = 0; a < 3; ++a) sum[a] += ((i >> a) & 1) + ((j >> a) & 1);
        }
    for (int i = 0; i < 8; ++i)
        for (int a = 0; a < 3; ++a)
            if (in[i]) normal[a] += ((i >> a) & 1) ? -1 : 1;
    memset(&out, 0, sizeof(out));
    for (int a = 0; a < 3; ++a) {
        out.cell[a] = h[a] - 1;
        out.sum[a] = (uint8_t) sum[a];
        out.normal[a] = (int8_t) normal[a];
    }
    out.edges = (uint8_t) edges;
    out.corners = (uint8_t) corners;
    return true;
}

static Mesh answer(const Volume& v, const VoxelBox& b, bool triangles, const float scale[3], const float offset[3])
{
    Mesh m;
    for (int z = b.origin[2]; z < b.end[2]; ++z)
        for (int y = b.origin[1]; y < b.end[1]; ++y)
            for (int x = b.origin[0]; x < b.end[0]; ++x) m.set_voxels += v.at(x, y, z);
    const BrickRange blocks = surface_blocks(b);
    std::map<std::vector<int>, uint32_t> index;
    std::vector<std::vector<int>> order;
    for (uint32_t k = 0; k < (uint32_t) range_bricks(blocks); ++k) {
        int bx, by, bz;
        range_brick(blocks, k, bx, by, bz);
        for (int c = 0; c < 512; ++c) {
            const int h[3] = {bx * 8 + (c & 7), by * 8 + ((c >> 3) & 7), bz * 8 + (c >> 6)};
            SurfaceVertex rec;
            if (!cell_record(v, b, h, rec)) continue;
            index[{h[0], h[1], h[2]}] = (uint32_t) m.vertices.size();
            order.push_back({h[0], h[1], h[2]});
            m.vertices.push_back(rec);
            for (int a = 0; a < 3; ++a) {
                volatile float q = (float) (2 * rec.edges * rec.cell[a] + rec.sum[a]) / (float) (2 * rec.edges);
                volatile float s = scale[a] * q;
                m.positions.push_back(s + offset[a]);
            }
        }
    }
    for (const std::vector<int>& h : order)
        for (int a = 0; a < 3; ++a) {
            int low[3] = {h[0], h[1], h[2]};
            --low[a];
            const bool lo = in_s(v, b, low[0], low[1], low[2]), hi = in_s(v, b, h[0], h[1], h[2]);
            if (lo == hi) continue;
            ++m.quads_axis[a];
            const int bb = (a + 1) % 3, cc = (a + 2) % 3;
            std::vector<int> k1 = h, k2 = h, k3 = h;
            ++k1[bb]; ++k2[bb]; ++k2[cc]; ++k3[cc];
            CHECK(index.count(k1) && index.count(k2) && index.count(k3), "a quad's cell is not active");
            uint32_t q[4] = {index[h], index[k1], index[k2], index[k3]};
            if (!lo) std::swap(q[1], q[3]);
            if (triangles) for (int i : {0, 1, 2, 0, 2, 3}) m.indices.push_back(q[i]);
            else for (int i = 0; i < 4; ++i) m.indices.push_back(q[i]);
        }
    return m;
}

// ---- the plan, dealt out as the kernels deal it ----------------------------------------------------------------------------------------
enum : uint32_t { EMPTY = 0, FULL = 1, MIXED = 2 };

struct Boards {
    int bn[3];
    std::vector<uint64_t> bits;  // 8 words per brick of the volume's grid: the set inside the volume (not cut to a box)
    std::vector<uint32_t> cls;
};

static Boards boards_of(const Volume& v)
{
    Boards b;
    for (int c = 0; c < 3; ++c) b.bn[c] = (v.dims[c] + 7) / 8;
    b.bits.assign((size_t) b.bn[0] * b.bn[1] * b.bn[2] * 8, 0);
    b.cls.assign((size_t) b.bn[0] * b.bn[1] * b.bn[2], EMPTY);
    for (int bz = 0; bz < b.bn[2]; ++bz)
        for (int by = 0; by < b.bn[1]; ++by)
            for (int bx = 0; bx < b.bn[0]; ++bx) {
                const size_t g = grid_index(b.bn[0], b.bn[0] * b.bn[1], bx, by, bz);
                bool any = false, all = true;
                for (int s = 0; s < 8; ++s) {
                    uint64_t w = 0;
                    for (int j = 0; j < 64; ++j)
                        if (v.at(bx * 8 + (j & 7), by * 8 + (j >> 3), bz * 8 + s)) w |= 1ull << j;
                    b.bits[g * 8 + s] = w;
                    any = any || w != 0;
                    all = all && w == slice_in_volume(v.dims, bx, by, bz * 8 + s);
                }
                b.cls[g] = !any ? EMPTY : (all ? FULL : MIXED);
            }
    return b;
}

static Mesh plan(const Boards& B, const VoxelBox& box, bool skip, bool triangles, const float scale[3], const float offset[3])
{
    Mesh m;
    BrickRange bricks{};
    for (int c = 0; c < 3; ++c) axis_bricks(box.origin[c], box.end[c], bricks.b0[c], bricks.nb[c]);
    const BrickRange blocks = surface_blocks(box);
    const uint32_t n = (uint32_t) range_bricks(blocks);
    std::vector<uint64_t> active((size_t) n * 8, 0), before((size_t) n * 8, 0), edges((size_t) n * 8 * 3, 0);
    std::vector<uint32_t> qbefore((size_t) n * 8, 0);
    std::vector<uint64_t> vcount(n, 0), qcount(n, 0), vbase(n, 0), qbase(n, 0);
    const auto fetch_of = [&](int bx, int by, int bz) {
        return [&B, &box, bricks, bx, by, bz](int dx, int dy, int dz, int s) -> uint64_t {
            const int nx = bx + dx, ny = by + dy, nz = bz + dz;
            if (!range_holds(bricks, nx, ny, nz)) return 0ull;
            CHECK(nx >= 0 && ny >= 0 && nz >= 0 && nx < B.bn[0] && ny < B.bn[1] && nz < B.bn[2], "a brick of the box's range outside the grid");
            return B.bits[grid_index(B.bn[0], B.bn[0] * B.bn[1], nx, ny, nz) * 8 + s] & slice_in_box(box, nx, ny, nz * 8 + s);
        };
    };
    // count
    for (uint32_t k = 0; k < n; ++k) {
        int bx, by, bz;
        range_brick(blocks, k, bx, by, bz);
        bool all_empty = true, all_full = true;
        for (int j = 0; j < 8; ++j) {
            const int nx = bx - (j & 1), ny = by - ((j >> 1) & 1), nz = bz - ((j >> 2) & 1);
            bool empty = true, full = false;
            if (range_holds(bricks, nx, ny, nz)) {
                const uint32_t cl = B.cls[grid_index(B.bn[0], B.bn[0] * B.bn[1], nx, ny, nz)];
                empty = cl == EMPTY;
                full = cl == FULL && brick_inside_box(box, nx, ny, nz);
            }
            all_empty = all_empty && empty;
            all_full = all_full && full;
        }
        const bool decided = all_empty || all_full;
        if (decided) ++m.skipped;
        else ++m.evaluated;
        uint64_t vs = 0, qs = 0;
        for (int z = 0; z < 8; ++z) {
            uint64_t c[8];
            surface_corner_words(fetch_of(bx, by, bz), z, c);
            const SurfaceSlice sl = surface_slice(c);
            if (decided) { // the rule of the skip: such a block has no active cell and no quad; its own voxels are none or all
                CHECK(sl.active == 0 && sl.edge[0] == 0 && sl.edge[1] == 0 && sl.edge[2] == 0, "a decided block has an active cell");
                CHECK(c[7] == (all_full ? ~0ull : 0ull), "a decided block's own board");
            }
            if (skip && decided) { m.set_voxels += all_full ? 64 : 0; continue; }
            m.set_voxels += (uint64_t) surface_popc(c[7]);
            active[(size_t) k * 8 + z] = sl.active;
            before[(size_t) k * 8 + z] = vs;
            qbefore[(size_t) k * 8 + z] = (uint32_t) qs;
            for (int a = 0; a < 3; ++a) {
                edges[((size_t) k * 8 + z) * 3 + a] = sl.edge[a];
                m.quads_axis[a] += (uint64_t) surface_popc(sl.edge[a]);
                qs += (uint64_t) surface_popc(sl.edge[a]);
                CHECK((sl.edge[a] & ~sl.active) == 0, "an owned edge of an inactive cell");
            }
            vs += (uint64_t) surface_popc(sl.active);
        }
        vcount[k] = vs;
        qcount[k] = qs;
    }
    // scan
    uint64_t vt = 0, qt = 0;
    for (uint32_t k = 0; k < n; ++k) { vbase[k] = vt; qbase[k] = qt; vt += vcount[k]; qt += qcount[k]; }
    m.vertices.resize(vt);
    m.positions.resize(vt * 3);
    const int per = triangles ? 6 : 4;
    m.indices.assign(qt * per, 0xdeadbeefu);
    const auto look = [&](uint32_t k, int z) { return SurfaceLook{vbase[k] + before[(size_t) k * 8 + z], active[(size_t) k * 8 + z]}; };
    // emit: a vertex at a time, as a lane takes it: its slice from the prefixes, its cell from its rank in the slice
    for (uint32_t k = 0; k < n; ++k) {
        if (!vcount[k]) continue;
        int bx, by, bz;
        range_brick(blocks, k, bx, by, bz);
        for (uint64_t j = 0; j < vcount[k]; ++j) {
            int z = 0;
            for (int s = 1; s < 8; ++s)
                if (before[(size_t) k * 8 + s] <= j) z = s;
            uint64_t c[8];
            surface_corner_words(fetch_of(bx, by, bz), z, c);
            const SurfaceSlice sl = surface_slice(c);
            CHECK(sl.active == active[(size_t) k * 8 + z] && j - before[(size_t) k * 8 + z] < (uint64_t) surface_popc(sl.active), "a vertex outside its slice");
            const int bit = surface_nth_bit(sl.active, (int) (j - before[(size_t) k * 8 + z]));
            const uint64_t below = (1ull << bit) - 1ull;
            const uint64_t vi = vbase[k] + j;
            uint64_t qi = qbase[k] + qbefore[(size_t) k * 8 + z] + (uint64_t) (surface_popc(sl.edge[0] & below) + surface_popc(sl.edge[1] & below) + surface_popc(sl.edge[2] & below));
            const uint64_t low_end[3] = {c[6], c[5], c[3]};
            const int hx = bx * 8 + (bit & 7), hy = by * 8 + (bit >> 3), hz = bz * 8 + z;
            const SurfaceVertex rec = surface_vertex(surface_corners(c, bit), hx, hy, hz);
            uint32_t w[kSurfaceVertexWords];
            surface_vertex_words(rec, w);
            CHECK(vi < vt, "a vertex beyond the count");
            if (vi >= vt) return m;
            memcpy(&m.vertices[vi], w, sizeof(w)); // the record as the dwords the kernel stores
            for (int a = 0; a < 3; ++a) m.positions[vi * 3 + a] = surface_position(rec.cell[a], rec.sum[a], rec.edges, scale[a], offset[a]);
            for (int a = 0; a < 3; ++a) {
                if (!((sl.edge[a] >> bit) & 1ull)) continue;
                uint32_t q[4], out[6];
                surface_quad(blocks, look, hx, hy, hz, a, ((low_end[a] >> bit) & 1ull) != 0, (uint32_t) vi, q);
                const int cnt = surface_quad_indices(q, triangles, out);
                CHECK(cnt == per && qi < qt, "a quad beyond the count");
                if (qi >= qt) return m;
                for (int i = 0; i < per; ++i) m.indices[qi * per + i] = out[i];
                ++qi;
            }
        }
    }
    return m;
}

static void compare(const Volume& v, const VoxelBox& box, const Boards& B, bool triangles, const char* what)
{
    const float scale[3] = {0.7f, 1.0f, 2.5f}, offset[3] = {-3.25f, 0.0f, 100.5f};
    const Mesh want = answer(v, box, triangles, scale, offset);
    for (int skip = 0; skip < 2; ++skip) {
        const Mesh got = plan(B, box, skip != 0, triangles, scale, offset);
        const bool same = got.vertices.size() == want.vertices.size() && got.indices == want.indices && got.set_voxels == want.set_voxels &&
                          (want.vertices.empty() || !memcmp(got.vertices.data(), want.vertices.data(), want.vertices.size() * sizeof(SurfaceVertex))) &&
                          (want.positions.empty() || !memcmp(got.positions.data(), want.positions.data(), want.positions.size() * sizeof(float)));
        CHECK(same, "%s: %d x %d x %d, box [%d,%d,%d)..[%d,%d,%d), skip %d, triangles %d: %zu / %zu vertices, %zu / %zu indices, set %llu / %llu", what, v.dims[0], v.dims[1], v.dims[2],
              box.origin[0], box.origin[1], box.origin[2], box.end[0], box.end[1], box.end[2], skip, (int) triangles, got.vertices.size(), want.vertices.size(), got.indices.size(),
              want.indices.size(), (unsigned long long) got.set_voxels, (unsigned long long) want.set_voxels);
        for (int a = 0; a < 3; ++a) CHECK(got.quads_axis[a] == want.quads_axis[a], "%s: quads along %d", what, a);
    }
}

static void masks()
{
    {
        std::mt19937_64 r64(3);
        for (int t = 0; t < 2000; ++t) {
            const uint64_t w = t == 0 ? ~0ull : (t == 1 ? 1ull << 63 : r64() & r64() & (t & 1 ? r64() : ~0ull));
            int rank = 0;
            for (int b = 0; b < 64; ++b)
                if ((w >> b) & 1ull) {
                    CHECK(surface_nth_bit(w, rank) == b, "surface_nth_bit");
                    ++rank;
                }
        }
    }
    const int widths[5] = {1, 7, 8, 9, 17};
    std::mt19937 rng(7);
    for (int t = 0; t < 200; ++t) {
        VoxelBox b{};
        for (int c = 0; c < 3; ++c) {
            b.origin[c] = (int) (rng() % 20);
            b.end[c] = b.origin[c] + widths[rng() % 5];
        }
        for (int bx = 0; bx < 5; ++bx)
            for (int by = 0; by < 5; ++by) {
                bool every = true;
                for (int z = 0; z < 40; z += 3) {
                    uint64_t w = 0;
                    for (int j = 0; j < 64; ++j) {
                        const int x = bx * 8 + (j & 7), y = by * 8 + (j >> 3);
                        if (x >= b.origin[0] && x < b.end[0] && y >= b.origin[1] && y < b.end[1] && z >= b.origin[2] && z < b.end[2]) w |= 1ull << j;
                    }
                    CHECK(slice_in_box(b, bx, by, z) == w, "slice_in_box");
                }
                for (int bz = 0; bz < 5; ++bz) {
                    every = true;
                    for (int c = 0; c < 3; ++c) {
                        const int at = (c == 0 ? bx : (c == 1 ? by : bz)) * 8;
                        every = every && at >= b.origin[c] && at + 8 <= b.end[c];
                    }
                    CHECK(brick_inside_box(b, bx, by, bz) == every, "brick_inside_box");
                }
            }
    }
}

int main()
{
    masks();
    const int widths[5] = {1, 7, 8, 9, 17};
    std::mt19937 rng(20);
    int cases = 0;
    for (int wx : widths)
        for (int wy : widths)
            for (int wz : widths) {
                Volume v{{wx, wy, wz}, {}};
                const size_t nvox = (size_t) wx * wy * wz;
                const VoxelBox whole{{0, 0, 0}, {wx, wy, wz}};
                for (int kind = 0; kind < 4; ++kind) { // random at 1/2, random at 7/8, full, one voxel
                    v.set.assign(nvox, kind == 2 ? 1 : 0);
                    if (kind < 2) for (size_t i = 0; i < nvox; ++i) v.set[i] = (rng() & 7) < (kind == 0 ? 4u : 7u);
                    if (kind == 3) v.set[rng() % nvox] = 1;
                    const Boards B = boards_of(v);
                    compare(v, whole, B, (cases & 1) != 0, "whole");
                    VoxelBox box{};
                    for (int c = 0; c < 3; ++c) { // a box with its own origin, ending inside a brick where it can
                        box.origin[c] = (int) (rng() % (unsigned) v.dims[c]);
                        box.end[c] = box.origin[c] + 1 + (int) (rng() % (unsigned) (v.dims[c] - box.origin[c]));
                    }
                    compare(v, box, B, (cases & 2) != 0, "box");
                    ++cases;
                }
            }
    { // two bricks' worth of full blocks in every direction: interior blocks are decided, the faces are not
        Volume v{{24, 24, 24}, {}};
        v.set.assign((size_t) 24 * 24 * 24, 1);
        const Boards B = boards_of(v);
        const VoxelBox whole{{0, 0, 0}, {24, 24, 24}};
        const float one[3] = {1, 1, 1}, zero[3] = {0, 0, 0};
        const Mesh m = plan(B, whole, true, false, one, zero);
        // 4^3 blocks of cells; the 2^3 whose eight bricks all exist are decided
        CHECK(m.skipped == 8 && m.evaluated == 64 - 8, "24^3 full: %d skipped, %d evaluated", m.skipped, m.evaluated);
        compare(v, whole, B, false, "24^3 full");
        compare(v, VoxelBox{{3, 8, 0}, {24, 17, 24}}, B, true, "24^3 full, a box");
    }
    std::printf("cases=%d\nfailures=%d\n", cases, failures);
    return failures ? 1 : 0;
}
