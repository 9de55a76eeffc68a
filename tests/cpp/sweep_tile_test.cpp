// The index rules of a tile of the propagation sweep (tbraymarcherplugin_amd/csrc/tbrm_sweep_tile.h) on their own, each against the
// answer found by enumeration: a halo word against the word its neighbour publishes and the halo's cells counted one by one, the LDS
// plane's cells against the plane's size, a brick layer staged through the piece copy and read through the staged offsets against the
// bricked volume, a chained tile's dependency against the tiles and the write-back order of the pass before, brick by brick.
// Pure host code, no device; tests/test_sweep_tile.py builds it with -fsanitize=address,undefined and runs it. Prints "failures=N" last.
#include "../../tbraymarcherplugin_amd/csrc/tbrm_sweep_tile.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <utility>
#include <vector>

using namespace tbrm;

static int failures = 0;
static long checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) {                                                     \
            if (++failures <= 20) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
        }                                                                  \
    } while (0)

static const int T = kSweepTile;
static const int kMaxReach = 14, kMaxChunks = 6; // what the host planner lets through (sweep_fit_reason)

// every (side, reach) of one plane axis: no side exactly when nothing is reached
template <class F>
static void each_side(F&& f)
{
    f(0, 0);
    for (int s = -1; s <= 1; s += 2)
        for (int h = 1; h <= kMaxReach; ++h) f(s, h);
}

// ---- hand-off words ---------------------------------------------------------------------------------------------------------------------
static void check_handoff(const SweepSides& g)
{
    const int chunks = sweep_halo_chunks(g.hx, g.hy), words = sweep_record_words(g.hx, g.hy);
    const int probe = 64 * (kMaxChunks + 1); // word numbers looked at: every lane of every chunk, and one chunk more
    // what the tile publishes: `words` words, the first ones, each a cell of the tile, no cell twice
    std::map<int, std::pair<int, int>> published;
    std::set<std::pair<int, int>> pub_cells;
    for (int w = 0; w < probe; ++w) {
        int cx = -1, cy = -1;
        if (!sweep_published_cell(w, g, T, cx, cy)) continue;
        CHECK(w == (int) published.size());
        CHECK(cx >= 0 && cx < T && cy >= 0 && cy < T);
        published[w] = {cx, cy};
        pub_cells.insert({cx, cy});
    }
    CHECK((int) published.size() == words);
    // (the hx columns and the hy rows overlap in hx x hy cells, which are published twice: once for each neighbour)
    CHECK((int) pub_cells.size() == words - g.hx * g.hy);
    // the halo: the hx columns, hy rows and hx x hy corner on the light's side, cell by cell
    std::map<std::pair<int, int>, int> want;
    const int x0 = g.sx > 0 ? T : -g.hx, y0 = g.sy > 0 ? T : -g.hy;
    for (int kx = 0; kx < g.hx; ++kx)
        for (int y = 0; y < T; ++y) want[{x0 + kx, y}] = 0;
    for (int ky = 0; ky < g.hy; ++ky)
        for (int x = 0; x < T; ++x) want[{x, y0 + ky}] = 0;
    for (int kx = 0; kx < g.hx; ++kx)
        for (int ky = 0; ky < g.hy; ++ky) want[{x0 + kx, y0 + ky}] = 0;
    CHECK((int) want.size() == T * g.hx + T * g.hy + g.hx * g.hy);
    int fetched = 0;
    for (int w = 0; w < probe; ++w) {
        const SweepHaloWord h = sweep_halo_word(w, g, T, 0, 0); // (tile (0, 0): the neighbour's tile is its offset)
        const SweepHaloWord moved = sweep_halo_word(w, g, T, 3, 5);
        CHECK(moved.on == h.on);
        if (!h.on) continue;
        ++fetched;
        CHECK(w < 64 * chunks);
        const int dx = h.ntx, dy = h.nty;
        CHECK(moved.ntx == 3 + dx && moved.nty == 5 + dy && moved.word == h.word && moved.cx == h.cx && moved.cy == h.cy);
        // it comes from an upstream neighbour: towards the light along the axes the cell lies outside the tile on
        CHECK(dx == (h.cx < 0 || h.cx >= T ? g.sx : 0) && dy == (h.cy < 0 || h.cy >= T ? g.sy : 0));
        CHECK(dx != 0 || dy != 0);
        // the neighbour publishes that word, and its cell — in the neighbour's tile, (dx, dy) tiles away — is this halo cell
        const auto it = published.find(h.word);
        CHECK(it != published.end());
        if (it != published.end()) CHECK(h.cx == it->second.first + dx * T && h.cy == it->second.second + dy * T);
        const auto cell = want.find({h.cx, h.cy});
        CHECK(cell != want.end());
        if (cell != want.end()) ++cell->second;
    }
    CHECK(fetched == (int) want.size());
    for (const auto& c : want) CHECK(c.second == 1);
}

// ---- the LDS plane ----------------------------------------------------------------------------------------------------------------------
// One plane axis of a launch: the launch's own streams' side and reach (s, h), those of the stream that comes from records (rs, rh;
// 0, 0: none), the origin, and the tile coordinates in use along it: the tile's pixels and both streams' halo
struct PlaneAxis {
    int s, h, rs, rh, origin;
    std::vector<int> cells;
};
static PlaneAxis plane_axis(int s, int h, int rs, int rh)
{
    PlaneAxis a = {s, h, rs, rh, sweep_plane_origin(s, h, rs, rh), {}};
    std::set<int> cells;
    for (int c = 0; c < T; ++c) cells.insert(c);
    for (int k = 0; k < h; ++k) cells.insert((s > 0 ? T : -h) + k);
    for (int k = 0; k < rh; ++k) cells.insert((rs > 0 ? T : -rh) + k);
    a.cells.assign(cells.begin(), cells.end());
    return a;
}
// every cell in use lies in x.cells x y.cells: own pixels, columns, rows and corners of both streams
static void check_plane(const PlaneAxis& x, const PlaneAxis& y)
{
    static std::vector<int> seen(kSweepPlane, 0);
    static int stamp = 0;
    ++stamp;
    const int ox = x.origin, oy = y.origin;
    for (int cx : x.cells)
        for (int cy : y.cells) {
            const int i = sweep_plane_cell(ox, oy, cx, cy);
            CHECK(i >= 0 && i + kSweepColStride + 1 < kSweepPlane); // the cell and the far tap of a pixel whose first tap it is
            CHECK(oy + cy >= 1 && oy + cy + 1 < kSweepColStride);   // a guard cell on either side, inside the cell's own column
            CHECK(ox + cx >= 1 && ox + cx + 1 < kSweepCols);
            if (i >= 0 && i < kSweepPlane) {
                CHECK(seen[i] != stamp); // no two cells share a word of the plane
                seen[i] = stamp;
            }
        }
}

// ---- light-volume staging ---------------------------------------------------------------------------------------------------------------
// byte of voxel (x, y, z) in a bricked volume of nb bricks per axis: bricks of 8 x 8 x 8 in x-fastest order, voxels inside likewise
static size_t voxel_byte(int x, int y, int z, const int (&nb)[3])
{
    const size_t brick = ((size_t) (z >> 3) * nb[1] + (size_t) (y >> 3)) * nb[0] + (size_t) (x >> 3);
    return brick * 512 + (size_t) (z & 7) * 64 + (size_t) (y & 7) * 8 + (size_t) (x & 7);
}
static uint32_t staged_at(const SweepPiece& pc) { return (uint32_t) (pc.brick * kSweepLvBrick + pc.part * 16); }
template <int AXIS>
static void check_staging(const int (&nb)[3])
{
    const int du = sweep_dim_u(AXIS), dv = sweep_dim_v(AXIS);
    std::vector<uint8_t> vol((size_t) nb[0] * nb[1] * nb[2] * 512);
    for (size_t i = 0; i < vol.size(); ++i) vol[i] = (uint8_t) ((i * 2654435761u) >> 13);
    const int threads = 512; // the compute threads of a tile
    for (int ty = 0; ty * 4 < nb[dv]; ++ty)
        for (int tx = 0; tx * 4 < nb[du]; ++tx) {
            const int base_x = tx * T, base_y = ty * T;
            std::vector<SweepPiece> pieces;
            std::set<uint32_t> src16, dst16;
            for (int i = 0; i < threads; ++i) {
                const SweepPiece pc = sweep_piece<AXIS>(i, base_x, base_y, nb);
                pieces.push_back(pc);
                // the pixels whose voxels are staged in the piece's brick (found through sweep_lv_at): the piece exists exactly when
                // their brick is one of the volume's
                int inside = -1;
                for (int r = 0; r < T; ++r)
                    for (int c = 0; c < T; ++c)
                        if ((int) (sweep_lv_at<AXIS>(c, r) / kSweepLvBrick) == pc.brick) {
                            const int in = ((base_x + c) >> 3) < nb[du] && ((base_y + r) >> 3) < nb[dv];
                            CHECK(inside < 0 || inside == in);
                            inside = in;
                        }
                CHECK(inside >= 0 && pc.exists == (inside == 1));
                CHECK(pc.brick >= 0 && pc.brick < 16 && pc.part >= 0 && pc.part < 32);
                CHECK(dst16.insert(staged_at(pc)).second);
                if (pc.exists) {
                    CHECK(pc.off % 16 == 0);
                    CHECK(src16.insert(pc.off).second);
                }
            }
            for (int L = 0; L < nb[AXIS]; ++L) {
                std::vector<uint8_t> staged(16 * kSweepLvBrick, 0xEE);
                for (const SweepPiece& pc : pieces) {
                    if (!pc.exists) continue;
                    const size_t src = (size_t) pc.off + (size_t) L * pc.layer_stride;
                    CHECK(src + 16 <= vol.size());
                    if (src + 16 <= vol.size()) std::memcpy(staged.data() + staged_at(pc), vol.data() + src, 16);
                }
                for (int r = 0; r < T; ++r)
                    for (int c = 0; c < T; ++c) {
                        const int px = base_x + c, py = base_y + r;
                        if ((px >> 3) >= nb[du] || (py >> 3) >= nb[dv]) continue; // (a brick past the volume: nothing is staged)
                        const uint32_t at = sweep_lv_at<AXIS>(c, r);
                        if ((r & 1) == 0) CHECK(sweep_lv_at<AXIS>(c, r + 1) == at + sweep_lv_row_step(AXIS));
                        for (int k = 0; k < 8; ++k) {
                            int v[3];
                            v[du] = px; v[dv] = py; v[AXIS] = L * 8 + k;
                            const size_t i = (size_t) at + (size_t) k * sweep_lv_step(AXIS);
                            CHECK(i < staged.size());
                            if (i < staged.size()) CHECK(staged[i] == vol[voxel_byte(v[0], v[1], v[2], nb)]);
                        }
                    }
            }
        }
}

// ---- chained launches -------------------------------------------------------------------------------------------------------------------
// axis: this pass's, a: the pass before's, which ran downwards (in_down) from layer in_layer0 over in_G layers. (Which way THIS pass
// runs decides only the order it visits its layers in: every layer is checked.)
static void check_chain(const int (&nb)[3], int axis, int a, int in_down)
{
    const int du = sweep_dim_u(axis), dv = sweep_dim_v(axis), ua = sweep_dim_u(a), va = sweep_dim_v(a);
    const int in_tiles_x = (nb[ua] + 3) / 4, in_G = nb[a], in_layer0 = in_down ? nb[a] - 1 : 0;
    for (int ty = 0; ty * 4 < nb[dv]; ++ty)
        for (int tx = 0; tx * 4 < nb[du]; ++tx) {
            int lo[3];
            lo[du] = tx * 4; lo[dv] = ty * 4; lo[axis] = 0;
            const SweepDep d = sweep_chain_dep(axis, a, in_tiles_x, in_down, in_layer0, lo);
            for (int L = 0; L < nb[axis]; ++L) {
                std::set<int> owners;
                int last = -1; // the last of the layer's bricks in the pass before's write-back order
                for (int ku = 0; ku < 4; ++ku)
                    for (int kv = 0; kv < 4; ++kv) {
                        int b[3];
                        b[du] = lo[du] + ku; b[dv] = lo[dv] + kv; b[axis] = L;
                        if (b[du] >= nb[du] || b[dv] >= nb[dv]) continue;
                        owners.insert((b[va] >> 2) * in_tiles_x + (b[ua] >> 2));
                        for (int g = 0; g < in_G; ++g)
                            if ((in_down ? in_layer0 - g : in_layer0 + g) == b[a]) last = std::max(last, g);
                    }
                CHECK(owners.size() == 1);
                if (owners.size() == 1) CHECK(*owners.begin() == sweep_dep_word(d, L));
                CHECK(last >= 0);
                CHECK(sweep_dep_needed(d, L, in_G) == (uint32_t) std::min(std::max(last + 1, 0), in_G));
            }
        }
}

int main()
{
    // hand-off: every geometry the planner lets through
    int geometries = 0;
    each_side([&](int sx, int hx) {
        each_side([&](int sy, int hy) {
            if (sweep_halo_chunks(hx, hy) > kMaxChunks) return;
            check_handoff(SweepSides{sx, sy, hx, hy});
            ++geometries;
        });
    });
    // the plane: every one-way geometry (no stream from records) and every two-way pair — per axis the low sides' larger reach plus
    // the high sides' is at most 14 —, cell by cell
    std::vector<PlaneAxis> axes;
    each_side([&](int s, int h) {
        each_side([&](int rs, int rh) {
            int lo = 0, hi = 0;
            (s < 0 ? lo : hi) = h;
            (rs < 0 ? lo : hi) = std::max(rs < 0 ? lo : hi, rh);
            if (lo + hi <= kMaxReach) axes.push_back(plane_axis(s, h, rs, rh));
        });
    });
    int pairs = 0;
    for (const PlaneAxis& x : axes)
        for (const PlaneAxis& y : axes) {
            if (sweep_halo_chunks(x.h, y.h) > kMaxChunks || sweep_halo_chunks(x.rh, y.rh) > kMaxChunks) continue;
            check_plane(x, y);
            ++pairs;
        }
    // staging: small ragged light volumes
    const int ragged[3] = {5, 3, 2}, single[3] = {1, 1, 1};
    check_staging<0>(ragged); check_staging<1>(ragged); check_staging<2>(ragged);
    check_staging<0>(single); check_staging<1>(single); check_staging<2>(single);
    // chain: volumes whose last tile is partial along one, two or all axes, and one that is whole tiles
    const int vols[4][3] = {{5, 6, 9}, {4, 8, 3}, {1, 1, 1}, {8, 4, 4}};
    for (const auto& nb : vols)
        for (int axis = 0; axis < 3; ++axis)
            for (int a = 0; a < 3; ++a)
                for (int in_down = 0; in_down < 2; ++in_down) check_chain(nb, axis, a, in_down);
    std::printf("geometries=%d plane_pairs=%d checks=%ld\n", geometries, pairs, checks);
    std::printf("failures=%d\n", failures);
    return failures ? 1 : 0;
}
