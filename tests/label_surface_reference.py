"""Restatement of include/tbrm_surface.h in numpy and Python integers (TEST INFRASTRUCTURE ONLY): the set, the cells, the vertex
records, the quads, the order and the float32 positions, voxel by voxel and cell by cell from the header's definition. Nothing here is
taken from the kernels: no boards, no slice words, no prefixes; the 8^3 blocks appear only as the header's sort key.

Label volumes are indexed [z, y, x]; origins, extents and cells are (x, y, z), as in the C-ABI."""
import numpy as np

VERTEX_DTYPE = np.dtype([("cell", "<i4", 3), ("sum", "u1", 3), ("edges", "u1"), ("normal", "i1", 3), ("corners", "u1")])
assert VERTEX_DTYPE.itemsize == 20
FIELDS = ("set_voxels", "vertices", "quads", "quads_axis", "cell_min", "cell_max")
MAX_DIM = 1 << 19
CORNERS = [((i & 1), (i >> 1) & 1, (i >> 2) & 1) for i in range(8)]
# the 12 edges of a cell as pairs of corners, and the midpoint of each in half voxels from the low corner
EDGES = [(i, j) for i in range(8) for j in range(i + 1, 8) if bin(i ^ j).count("1") == 1]
MIDPOINTS = [tuple(CORNERS[i][a] + CORNERS[j][a] for a in range(3)) for i, j in EDGES]


def resolve_box(dims, origin=None, extent=None):
    if extent is None or tuple(int(v) for v in extent) == (0, 0, 0):
        return (0, 0, 0), tuple(int(d) for d in dims)
    o = tuple(int(v) for v in (origin if origin is not None else (0, 0, 0)))
    return o, tuple(o[c] + int(extent[c]) for c in range(3))


def the_set(labels, source, origin=None, extent=None):
    """bool [z, y, x]: the voxels of the box whose label is in `source`"""
    dims = labels.shape[::-1]
    o, e = resolve_box(dims, origin, extent)
    inside = np.zeros(labels.shape, dtype=bool)
    inside[o[2]:e[2], o[1]:e[1], o[0]:e[0]] = True
    return np.isin(labels, np.asarray(list(source), dtype=labels.dtype)) & inside


def in_set(S, x, y, z):
    nz, ny, nx = S.shape
    return 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and bool(S[z, y, x])


def vertex_of(S, h):
    """the record of the cell with the high corner h as a tuple (cell, sum, edges, normal, corners), or None when it is not active"""
    inside = [in_set(S, h[0] - 1 + c[0], h[1] - 1 + c[1], h[2] - 1 + c[2]) for c in CORNERS]
    corners = sum(1 << i for i in range(8) if inside[i])
    if corners in (0, 255):
        return None
    differing = [k for k, (i, j) in enumerate(EDGES) if inside[i] != inside[j]]
    total = tuple(sum(MIDPOINTS[k][a] for k in differing) for a in range(3))
    normal = tuple(sum(inside[i] for i in range(8) if CORNERS[i][a] == 0) - sum(inside[i] for i in range(8) if CORNERS[i][a] == 1) for a in range(3))
    return (tuple(v - 1 for v in h), total, len(differing), normal, corners)


def order_key(h):
    """the header's total order: blocks of 8^3 by h >> 3, x fastest; inside a block x fastest"""
    return (h[2] >> 3, h[1] >> 3, h[0] >> 3, h[2] & 7, h[1] & 7, h[0] & 7)


def positions_of(vertices, scale=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0)):
    """float32 [n, 3]: one float32 division, one multiplication, one addition"""
    v = np.asarray(vertices, dtype=VERTEX_DTYPE)
    den = (2 * v["edges"].astype(np.int64))[:, None]
    num = den * v["cell"].astype(np.int64) + v["sum"].astype(np.int64)
    assert (np.abs(num) < 2 ** 24).all()
    q = num.astype(np.float32) / den.astype(np.float32)
    assert q.dtype == np.float32
    m = np.asarray(scale, dtype=np.float32)[None, :] * q
    return (m + np.asarray(offset, dtype=np.float32)[None, :]).astype(np.float32)


def unit_cube(dims):
    """(scale, offset) of tbrm_host_surface_unit_cube"""
    return tuple(np.float32(1.0 / (n - 1)) if n > 1 else np.float32(0.0) for n in dims), (np.float32(0.0),) * 3


def surface(labels, source, origin=None, extent=None, triangles=False, scale=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0)):
    """a dict: FIELDS, "vertex" (VERTEX_DTYPE [n]), "indices" (uint32 [quads, 4 or 6]), "positions" (float32 [n, 3])"""
    dims = labels.shape[::-1]
    o, e = resolve_box(dims, origin, extent)
    S = the_set(labels, source, origin, extent)
    # candidates: every cell that has a voxel of S among its corners (all others have corners == 0)
    zs, ys, xs = np.nonzero(S)
    cand = set()
    for x, y, z in zip(xs.tolist(), ys.tolist(), zs.tolist()):
        for c in CORNERS:
            cand.add((x + c[0], y + c[1], z + c[2]))
    cells = {}
    for h in cand:
        assert all(o[a] <= h[a] <= e[a] for a in range(3))
        v = vertex_of(S, h)
        if v is not None:
            cells[h] = v
    ordered = sorted(cells, key=order_key)
    index = {h: i for i, h in enumerate(ordered)}
    vertex = np.zeros(len(ordered), dtype=VERTEX_DTYPE)
    for i, h in enumerate(ordered):
        vertex[i] = cells[h]
    quads, quads_axis = [], [0, 0, 0]
    for h in ordered:
        for a in range(3):
            low = list(h)
            low[a] -= 1
            lo_in, hi_in = in_set(S, *low), in_set(S, *h)
            if lo_in == hi_in:
                continue
            b, c = (a + 1) % 3, (a + 2) % 3
            k = [list(h) for _ in range(4)]
            k[1][b] += 1
            k[2][b] += 1
            k[2][c] += 1
            k[3][c] += 1
            q = [index[tuple(v)] for v in k]
            quads.append(q if lo_in else [q[0], q[3], q[2], q[1]])
            quads_axis[a] += 1
    quad = np.asarray(quads, dtype=np.uint32).reshape(-1, 4)
    indices = quad[:, [0, 1, 2, 0, 2, 3]] if triangles else quad
    res = {"set_voxels": int(S.sum()), "vertices": len(ordered), "quads": len(quads), "quads_axis": tuple(quads_axis)}
    if ordered:
        res["cell_min"] = tuple(int(v) for v in vertex["cell"].min(axis=0))
        res["cell_max"] = tuple(int(v) for v in vertex["cell"].max(axis=0))
    else:
        res["cell_min"], res["cell_max"] = tuple(int(d) for d in dims), (-1, -1, -1)
    res.update(vertex=vertex, indices=np.ascontiguousarray(indices), positions=positions_of(vertex, scale, offset))
    return res


# ---- properties, in exact integer arithmetic -----------------------------------------------------------------------------------------------
def quads_of(indices, triangles):
    idx = np.asarray(indices, dtype=np.int64)
    if not triangles:
        return idx.reshape(-1, 4)
    t = idx.reshape(-1, 6)
    assert (t[:, 0] == t[:, 3]).all() and (t[:, 2] == t[:, 4]).all()
    return t[:, [0, 1, 2, 5]]


def sixfold_volume_doubled(points2, quads):
    """six times the signed volume of the closed quad mesh whose vertices lie at points2 / 2 (integers), times 8: sum over the
    triangles (q0, q1, q2), (q0, q2, q3) of det(p0, p1, p2) on the doubled coordinates"""
    total = 0
    p = [tuple(int(c) for c in row) for row in points2]
    for q in quads:
        for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
            a, b, c = p[t[0]], p[t[1]], p[t[2]]
            total += (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]))
    return total


def edge_uses(quads):
    """{undirected edge: number of quads that have it}"""
    uses = {}
    for q in quads:
        for i in range(4):
            e = (int(min(q[i], q[(i + 1) % 4])), int(max(q[i], q[(i + 1) % 4])))
            uses[e] = uses.get(e, 0) + 1
    return uses


def differing_face_pairs(S):
    """per axis: pairs of face-adjacent positions, one in S and one not, the outside of the volume counting as not in S"""
    P = np.pad(S, 1)
    return tuple(int((np.diff(P.astype(np.int8), axis=ax) != 0).sum()) for ax in (2, 1, 0))


# ---- sets ----------------------------------------------------------------------------------------------------------------------------------
def random_labels(dims, density, seed, labels=(3,)):
    rng = np.random.default_rng(seed)
    out = np.zeros(dims[::-1], dtype=np.uint8)
    pick = rng.random(dims[::-1]) < density
    out[pick] = rng.choice(np.asarray(labels, dtype=np.uint8), size=int(pick.sum()))
    return out


def ball_labels(dims, centre, radius, label=3):
    z, y, x = np.indices(dims[::-1])
    out = np.zeros(dims[::-1], dtype=np.uint8)
    out[(x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius * radius] = label
    return out


def checkerboard_labels(dims, label=3):
    z, y, x = np.indices(dims[::-1])
    return (((x + y + z) & 1) * label).astype(np.uint8)
