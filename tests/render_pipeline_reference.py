"""Random sequences of everything that changes or reads the render state of one handle (TEST INFRASTRUCTURE ONLY): a seeded
generator of step lists and an interpreter that runs a step list on oracle.OracleScene. No algorithm lives here: the interpreter
dispatches to the oracle's operators and frame calls, edits the oracle's data volume in place for the data writes, and keeps what
the handle keeps between calls (data, transfer function, window, present lights, label volume) next to what the caller passes with
every call (world, view).

A step is a plain dict that prints in an assertion message; blocks of voxels, volumes, label volumes and colour tables are rebuilt
from the seeds it carries. The kinds:
    add, remove, change   add_dir_light / change_dir_light (a colour handle: their colour forms); "how" of a change: "small" (a few
                          degrees: the fused path), "across" (another major axis), "back" (to a direction this light had before)
    batch                 add_dir_lights of three lights; the oracle replays the pass order the library reports
    reset                 clear_light_volume, then every present light again
    window                set_windowing; "how": "new", "same" (the window in force, again), "ulp" (the centre one float32 on), "cutoffs"
                          (centre and width as they are, both cut-off flags flipped)
    tf                    set_tf_lut: curve A, curve B or the step curve (alpha > 0 at 0: the volume's shell turns opaque)
    region                update_volume_region(_device) of every box in "boxes": (origin, extent, mode, seed); modes: "empty" (zeros
                          over whole bricks), "fill" (high values), "window" (values inside the window in force)
    upload                upload_volume of another synthetic volume
    world, view           nothing on the handle: the world / the frame view that later calls pass
    cache_clear           light_cache_clear
    frames                k times raymarch_lit_device + flush of the view in force
    modes                 raymarch_intensity, generate_octree + raymarch_octree of one level, raymarch_hits
    labels                upload_label_volume + set_label_colors ("attach"), or release_label_volume

Volumes are indexed [z, y, x]; origins and extents are (x, y, z), as in the C-ABI."""
import copy
import functools

import numpy as np

from tbraymarcherplugin_amd import abi, synthetic as S
import exact_reference as X
import exact_scenes as E
import label_reference as LR

SEEDS = tuple(range(12))
STEPS = 24
CHECKPOINTS = (7, 15, 23)
BRICK = 8
LIGHT_OPS = ("add", "remove", "change", "batch", "reset")
SETTERS = ("window", "tf", "region", "upload")                       # what invalidates cached occlusion and recorded frames
INVALIDATING = SETTERS + ("labels", "world", "view")               # what a relit frame must not be served across
WINDOWS = ((0.5, 0.9, True, False), (0.45, 0.7, True, True), (0.55, 1.1, False, False))
TFS = ("A", "B", "step")
WORLDS = {"default": S.default_world(), "rot": E.ROT_WORLD, "clip": E.CLIP_THROUGH}
# the frame views: tests/test_gpu_view_cache.py's (a 40 x 28 frame, a tile off the origin whose width is no multiple of 8, rows in
# interleaved groups, jittered) and a whole 64 x 48 frame without jitter: (frame size, tile, steps, jitter frame)
VIEWS = (((40, 28), (3, 2, 29, 12, 2), 48.0, 3), ((64, 48), (0, 0, 64, 48, 1), 64.0, -1))
HIT_THRESHOLD = 0.5
MANY_BOXES = 70   # more than the 64 boxes a handle tracks before it falls back to the whole grid

# (dims, data type, float light volume, half resolution, address mode, border mode, colour handle, reserved, the many-boxes seed)
_W, _C, _E8, _XF = abi.ADDRESS_WRAP, abi.ADDRESS_CLAMP, abi.BORDER_ENGINE_8BIT, abi.BORDER_EXACT_FLOAT
SETUPS = [
    ((72, 64, 56), "uint8", False, False, _W, _E8, False, False, False),     # whole brick layers, 3 x 2 sweep tiles
    ((67, 45, 53), "uint16", False, False, _W, _XF, False, False, False),    # ragged pass lengths
    ((45, 40, 37), "float32", False, True, _W, _E8, False, False, False),    # a half-resolution light volume of an odd scan
    ((33, 40, 17), "uint8", False, False, _C, _E8, False, False, False),     # ragged last bricks
    ((40, 40, 5), "uint16", False, False, _W, _E8, False, False, False),     # a downward pass the sweep declines
    ((104, 88, 72), "float32", False, False, _W, _E8, False, False, False),  # several tiles per plane (the one larger seed)
    ((72, 64, 56), "uint8", True, False, _W, _E8, False, False, False),
    ((67, 45, 53), "uint16", False, False, _W, _E8, True, False, False),
    ((45, 40, 37), "float32", False, True, _W, _E8, False, True, False),
    ((33, 40, 17), "uint8", False, False, _W, _E8, False, False, True),
    ((40, 40, 5), "uint16", True, False, _C, _E8, False, False, False),
    ((72, 64, 56), "float32", False, False, _W, _E8, False, False, False),
]


def setup(seed):
    dims, dtype, light32, half, addr, border, rgb, reserve, many = SETUPS[seed]
    return {"seed": seed, "dims": dims, "dtype": dtype, "light32": light32, "half": half, "addr": addr, "border": border, "rgb": rgb,
            "reserve": reserve, "many": many, "vol_seed": 0x5EED0800 + seed, "tf": "A", "window": WINDOWS[0]}


# ---- what a step's seeds stand for ----------------------------------------------------------------------------------------------
def top_of(dtype):
    dtype = np.dtype(dtype)
    return 1.0 if dtype == np.float32 else float(np.iinfo(dtype).max)


def volume_of(dims, dtype, vol_seed):
    return S.make_volume_numpy(dims, np.dtype(dtype), vol_seed)


def box_block(box, dtype, window):
    """the voxels of one box of a region step, [ez, ey, ex]"""
    _, (ex, ey, ez), mode, seed = box
    dtype = np.dtype(dtype)
    if mode == "empty":
        return np.zeros((ez, ey, ex), dtype=dtype)
    r = np.random.default_rng(seed).random((ez, ey, ex))
    if mode == "fill":
        r = 0.6 + 0.4 * r
    else:   # inside the window in force
        lo, hi = max(window[0] - window[1] / 2, 0.0), min(window[0] + window[1] / 2, 1.0)
        r = lo + (hi - lo) * (0.1 + 0.8 * r)
    return r.astype(np.float32) if dtype == np.float32 else np.floor(r * top_of(dtype)).astype(dtype)


def label_volume(dims, seed):
    """two ellipsoids of labels 1 and 2 about the middle of the volume, a fifth to a third of each dimension in radius
    (tests/test_gpu_labels.py sphere_labels is the model; ellipsoids: a flat volume gets more than a voxel's worth)"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    lab = np.zeros((nz, ny, nx), dtype=np.uint8)
    for v in (1, 2):
        c, r = rng.uniform(0.35, 0.65, size=3), rng.uniform(0.2, 0.33, size=3)
        lab[((x - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((z - c[2]) / r[2]) ** 2 <= 1.0] = v
    return lab


def label_colors(seed):
    c = np.zeros((256, 4), dtype=np.float32)
    rng = np.random.default_rng(seed)
    c[1:, :3] = rng.uniform(0.0, 1.0, size=(255, 3))
    c[1:, 3] = rng.uniform(0.3, 0.9, size=255)
    return c


def tf_lut(name):
    return E.tf_lut(name)


def mono_light(l, channel=None):
    """the DirLightParams of a step's light; of channel c of a colour light: intensity x colour, one float32 product
    (tests/test_gpu_color_lights.py channel_light)"""
    if channel is None or len(l) == 2:
        return abi.DirLightParams(l[0], l[1])
    return abi.DirLightParams(l[0], float(np.float32(l[1]) * np.float32(l[2][channel])))


def view_args(index, world_name):
    """(camera, tile, raymarch parameters, world) of a frame call"""
    fb, tile, steps, jitter = VIEWS[index]
    return S.default_camera(*fb), abi.Tile(*tile), abi.RaymarchParams(steps, jitter, True), WORLDS[world_name]


def plain_schedule(lights, world, light_dims, border):
    """the pass order of a batch nobody paired: light by light (what the interpreter replays when it is given no schedule)"""
    return [(i, p, -1, -1) for i, l in enumerate(lights) for p in range(abi.host_light_passes(mono_light(l), world, light_dims, border)[1])]


# ---- the interpreter ------------------------------------------------------------------------------------------------------------
class State:
    """what the handle holds and what the caller passes, on the oracle: one OracleScene (a colour handle: one per channel, on one
    shared data volume)"""

    def __init__(self, su, oracle_mod):
        self.su, self.oracle_mod = su, oracle_mod
        self.vol = np.ascontiguousarray(volume_of(su["dims"], su["dtype"], su["vol_seed"])).copy()
        self.orcs = [oracle_mod.OracleScene(self.vol, su["light32"], su["half"], su["addr"], su["border"]) for _ in range(3 if su["rgb"] else 1)]
        assert all(o.volume is self.vol for o in self.orcs)   # (a data write is an edit of this array: _scene() builds its view per call)
        self.tf, self.window, self.world, self.view = su["tf"], tuple(su["window"]), "default", 0
        self.labels, self.colors = None, None
        for o in self.orcs:
            o.set_tf_lut(tf_lut(self.tf))
            o.set_windowing(abi.WindowingParams(*self.window))

    def fork(self):
        """an independent copy (the data volume and the light volumes copied)"""
        other = copy.copy(self)
        other.vol = self.vol.copy()
        other.orcs = []
        for o in self.orcs:
            n = self.oracle_mod.OracleScene(other.vol, self.su["light32"], self.su["half"], self.su["addr"], self.su["border"])
            n.light[...] = o.light
            n.tf = o.tf
            n.set_windowing(o.windowing)
            other.orcs.append(n)
        return other

    def lights(self):
        return [o.light.copy() for o in self.orcs]

    def frame(self):
        """(the lit frame of the view in force without labels, the nominal sample count); a colour handle: channel c from the
        scene of channel c"""
        cam, tile, rp, world = view_args(self.view, self.world)
        outs = [o.raymarch_lit(cam, tile, rp, world) for o in self.orcs]
        frame = outs[0][0].copy()
        for c in range(1, len(outs)):
            frame[..., c] = outs[c][0][..., c]
        return frame, outs[0][1]

    def labels_shown(self, by):
        """the pixels of the view in force that the attached label volume moves by more than `by`: the float64 restatement of the
        lit march with the label step (tests/label_reference.py) against the one without, lit by the first channel"""
        o = self.orcs[0]
        ex = X.Scene(self.vol, o.tf, abi.WindowingParams(*self.window), o.light_dims, not self.su["light32"], self.su["addr"], self.su["border"])
        ex.set_light(o.light)
        cam, tile, rp, world = view_args(self.view, self.world)
        with_labels, _ = LR.raymarch_lit(ex, self.labels, self.colors, cam, tile, rp.steps, rp.jitter_frame, world)
        without, _ = X.raymarch_lit(ex, cam, tile, rp.steps, rp.jitter_frame, world)
        return int((np.abs(with_labels - without).max(axis=-1) > by).sum())

    def apply(self, step, schedule=None):
        """one step -> its trace entry: {"kind"}, after a light operator "light" (a list: one volume per channel), after frames
        "frame" and "count", after modes "intensity", "octree" and "count" """
        kind, entry = step["kind"], {"kind": step["kind"]}
        world = WORLDS[self.world]
        if kind in ("add", "remove"):
            for c, o in enumerate(self.orcs):
                o.add_dir_light(mono_light(step["light"], c), kind == "add", world)
        elif kind == "change":
            for c, o in enumerate(self.orcs):
                o.change_dir_light(mono_light(step["old"], c), mono_light(step["new"], c), world)
        elif kind == "batch":
            o = self.orcs[0]
            if schedule is None:
                schedule = plain_schedule(step["lights"], world, o.light_dims, self.su["border"])
            for la, pa, lb, pb in schedule:
                o.add_dir_light_pass(mono_light(step["lights"][la]), True, world, pa)
                if lb >= 0:
                    o.add_dir_light_pass(mono_light(step["lights"][lb]), True, world, pb)
        elif kind == "reset":
            for c, o in enumerate(self.orcs):
                o.clear_light_volume(0.0)
                for l in step["lights"]:
                    o.add_dir_light(mono_light(l, c), True, world)
        elif kind == "window":
            self.window = tuple(step["window"])
            for o in self.orcs:
                o.set_windowing(abi.WindowingParams(*self.window))
        elif kind == "tf":
            self.tf = step["tf"]
            for o in self.orcs:
                o.set_tf_lut(tf_lut(self.tf))
        elif kind == "region":
            for box in step["boxes"]:
                (x, y, z), (ex, ey, ez) = box[0], box[1]
                self.vol[z:z + ez, y:y + ey, x:x + ex] = box_block(box, self.vol.dtype, self.window)
        elif kind == "upload":
            self.vol[...] = volume_of(self.su["dims"], self.su["dtype"], step["vol_seed"])
        elif kind == "world":
            self.world = step["world"]
        elif kind == "view":
            self.view = step["view"]
        elif kind == "labels":
            self.labels = label_volume(self.su["dims"], step["seed"]) if step["attach"] else None
            self.colors = label_colors(step["seed"]) if step["attach"] else None
        elif kind == "frames":
            entry["frame"], entry["count"] = self.frame()
        elif kind == "modes":
            cam, tile, rp, world = view_args(self.view, self.world)
            o = self.orcs[0]
            entry["intensity"] = o.raymarch_intensity(cam, tile, rp, world)
            o.generate_octree()
            entry["octree"] = o.raymarch_octree(cam, tile, rp, world, step["mip"])
            entry["count"] = o.raymarch_lit(cam, tile, rp, world, count_only=True)[1]
        elif kind != "cache_clear":
            raise ValueError(step)
        if kind in LIGHT_OPS:
            entry["light"] = self.lights()
        return entry


def run(su, steps, oracle_mod, schedules=None, skip=()):
    """the step list from the set-up's first state -> one trace entry per step (None for a step in `skip`)"""
    st = State(su, oracle_mod)
    return [None if i in skip else st.apply(step, (schedules or {}).get(i)) for i, step in enumerate(steps)]


# ---- the generator --------------------------------------------------------------------------------------------------------------
def pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def major_axis(d):
    return int(np.argmax(np.abs(d)))


def random_light(rng, rgb):
    """the direction families of test_random_light_operator_sequences_against_oracle"""
    family = int(rng.integers(0, 4))
    if family == 0:    # anywhere
        d = rng.normal(size=3)
    elif family == 1:  # nearly along an axis
        d = rng.normal(size=3) * 0.08
        d[rng.integers(0, 3)] = rng.choice([-1.0, 1.0])
    elif family == 2:  # nearly on a face diagonal
        d = rng.normal(size=3) * 0.05
        a, b = rng.choice(3, size=2, replace=False)
        d[a] = rng.choice([-1.0, 1.0])
        d[b] = d[a] * rng.choice([-1.0, 1.0]) * rng.uniform(0.97, 1.03)
    else:              # exactly axis-aligned
        d = np.zeros(3)
        d[rng.integers(0, 3)] = rng.choice([-1.0, 1.0])
    light = (tuple(float(v) for v in d), float(rng.uniform(0.2, 0.7)))
    if rgb:
        light += (tuple(float(v) for v in np.round(rng.uniform(0.1, 1.0, size=3), 3)),)
    return light


def turned(rng, light, how):
    d = light[0]
    if how == "small":
        nd = tuple(float(v) for v in S.rotate_z(d, float(rng.choice([-1.0, 1.0]) * rng.uniform(3.0, 6.0))))
        if major_axis(nd) != major_axis(d) or max(abs(d[0]), abs(d[1])) == 0.0:   # (along z a turn about z is none: tilt it)
            nd = tuple(float(v) for v in np.asarray(d) + 0.06 * np.linalg.norm(d) * np.roll(np.eye(3)[major_axis(d)], 1))
    else:   # another major axis
        nd = tuple(float(v) for v in np.roll(np.asarray(d), 1) + rng.normal(size=3) * 0.05)
    return (nd, float(rng.uniform(0.2, 0.7))) + tuple(light[2:])


class Plan:
    """what the generator knows while it draws: the present lights and where each has been, the setters' running choices"""

    def __init__(self, su, rng):
        self.su, self.rng = su, rng
        self.present, self.history = [], []
        self.window, self.tf, self.world, self.view = tuple(su["window"]), su["tf"], "default", 0
        self.uploads = self.regions = self.label_steps = 0
        self.attached = False
        self.many_left = su["many"]
        self.vol = volume_of(su["dims"], su["dtype"], su["vol_seed"]).copy()   # the data as it stands: where a region step matters

    # light operators
    def swept_faces(self, l):
        """the cube faces of this light's passes under the world in force, if the sweep takes every one of them (the planner's
        word, abi.host_plan_light); else ()"""
        lv = tuple((d + 1) // 2 if self.su["half"] else d for d in self.su["dims"])
        light, world = mono_light(l, 0), WORLDS[self.world]
        passes, n = abi.host_light_passes(light, world, lv, self.su["border"])
        plan = abi.host_plan_light(light, world, lv, self.su["light32"])
        return tuple(passes[k].face for k in range(n)) if len(plan) == n and all(q[0] == 0 for q in plan) else ()

    def add(self):
        l = random_light(self.rng, self.su["rgb"])
        self.present.append(l)
        self.history.append([l])
        return {"kind": "add", "light": l}

    def remove(self):
        i = int(self.rng.integers(len(self.present)))
        self.history.pop(i)
        return {"kind": "remove", "light": self.present.pop(i)}

    def change(self, how=None, index=None):
        i = int(self.rng.integers(len(self.present))) if index is None else index
        old = self.present[i]
        if how is None:
            how = pick(self.rng, ("small", "across", "back") if len(self.history[i]) > 1 else ("small", "across"))
        new = pick(self.rng, self.history[i][:-1]) if how == "back" else turned(self.rng, old, how)
        self.present[i] = new
        self.history[i].append(new)
        return {"kind": "change", "old": old, "new": new, "how": how}

    def light_op(self, on_present=False):
        kinds = ["change", "change"] + (["remove"] if len(self.present) > 1 else []) + ([] if on_present or len(self.present) > 3 else ["add"])
        return getattr(self, pick(self.rng, kinds))()

    def batch(self):
        lights = [random_light(self.rng, False) for _ in range(3)]
        self.present += lights
        self.history += [[l] for l in lights]
        return {"kind": "batch", "lights": lights}

    def reset(self):
        return {"kind": "reset", "lights": list(self.present)}

    # setters
    def window_step(self, how=None):
        how = how or ("same", "ulp", "new")[self.su["seed"] % 3]
        if how == "new":   # (WINDOWS differ in their widths: also from a window an "ulp" step moved)
            self.window = pick(self.rng, [w for w in WINDOWS if w[1] != self.window[1]])
        elif how == "ulp":
            self.window = (float(np.nextafter(np.float32(self.window[0]), np.float32(1.0))),) + self.window[1:]
        elif how == "cutoffs":   # centre and width as they are (and with them the data border): only the two flags
            self.window = self.window[:2] + (not self.window[2], not self.window[3])
        return {"kind": "window", "window": self.window, "how": how}

    def tf_step(self):
        self.tf = pick(self.rng, [t for t in TFS if t != self.tf])
        return {"kind": "tf", "tf": self.tf}

    def brick_sums(self):
        """the sum of every brick's voxels, [bz, by, bx]"""
        v = np.pad(self.vol.astype(np.float64), [(0, -n % BRICK) for n in self.vol.shape])
        return v.reshape(v.shape[0] // BRICK, BRICK, v.shape[1] // BRICK, BRICK, v.shape[2] // BRICK, BRICK).sum(axis=(1, 3, 5))

    def brick_box(self, nb_each, densest):
        """a box of whole bricks, nb_each bricks per axis: one of the three that hold the most (densest) or, in the middle half of
        the volume, the least of the data as it stands — where emptying, and where filling, changes what lights and rays meet"""
        sums = self.brick_sums()
        k = [min(k, n) for k, n in zip(nb_each, sums.shape[::-1])]
        scored = []
        for bz in range(sums.shape[0] - k[2] + 1):
            for by in range(sums.shape[1] - k[1] + 1):
                for bx in range(sums.shape[2] - k[0] + 1):
                    middle = all(n // 4 <= b + kk / 2 <= n - n // 4 for b, kk, n in zip((bx, by, bz), k, sums.shape[::-1]))
                    if densest or middle:
                        total = float(sums[bz:bz + k[2], by:by + k[1], bx:bx + k[0]].sum())
                        scored.append((-total if densest else total, (bx, by, bz)))
        scored.sort()
        b = pick(self.rng, scored[:3])[1]
        origin = tuple(v * BRICK for v in b)
        return origin, tuple(min(kk * BRICK, n - o) for kk, n, o in zip(k, self.su["dims"], origin))

    def region_step(self, size=None, mode=None):
        dims = self.su["dims"]
        self.regions += 1
        seed = lambda: int(self.rng.integers(1 << 30))
        if self.many_left:   # more boxes than a handle tracks between two uses of its skipping metadata
            self.many_left = False
            boxes = []
            for _ in range(MANY_BOXES):
                o = tuple(int(self.rng.integers(0, n - 1)) for n in dims)
                boxes.append((o, tuple(min(2, n - v) for n, v in zip(dims, o)), "fill", seed()))
            step = {"kind": "region", "size": "many", "boxes": boxes, "device": False}
            self.write(step)
            return step
        size, mode = size or pick(self.rng, ("brick", "few", "half")), mode or pick(self.rng, ("empty", "fill", "window"))
        if size == "half":
            axis = int(np.argmax(dims)) if self.rng.random() < 0.5 else int(self.rng.integers(2))   # (an axis of more than one brick)
            half = dims[axis] // 2 // BRICK * BRICK
            lower = self.rng.random() < 0.5
            origin = tuple((0 if lower else half) if a == axis else 0 for a in range(3))
            extent = tuple((half if lower else dims[a] - half) if a == axis else dims[a] for a in range(3))
        else:
            nb = (1, 1, 1) if size == "brick" else (2, 2, int(self.rng.integers(1, 3)))
            origin, extent = self.brick_box(nb, densest=mode != "fill")
            if mode == "window" and size == "few":   # a box that cuts through bricks
                origin = tuple(max(o - 3, 0) for o in origin)
        step = {"kind": "region", "size": size, "boxes": [(origin, extent, mode, seed())], "device": self.regions % 2 == 0}
        self.write(step)
        return step

    def write(self, step):
        for box in step["boxes"]:
            (x, y, z), (ex, ey, ez) = box[0], box[1]
            self.vol[z:z + ez, y:y + ey, x:x + ex] = box_block(box, self.vol.dtype, self.window)

    def upload_step(self):
        self.uploads += 1
        self.vol = volume_of(self.su["dims"], self.su["dtype"], 0x5EED0777 + self.uploads + 16 * self.su["seed"]).copy()
        return {"kind": "upload", "vol_seed": 0x5EED0777 + self.uploads + 16 * self.su["seed"]}

    def setter(self, kind, how=None, size=None, mode=None):
        return {"window": lambda: self.window_step(how or "new"), "tf": self.tf_step, "region": lambda: self.region_step(size, mode), "upload": self.upload_step}[kind]()

    # the rest
    def world_step(self):
        self.world = pick(self.rng, [w for w in WORLDS if w != self.world])
        return {"kind": "world", "world": self.world}

    def view_step(self):
        self.view = 1 - self.view
        return {"kind": "view", "view": self.view}

    def labels_step(self):
        self.attached = not self.attached
        self.label_steps += 1
        return {"kind": "labels", "attach": self.attached, "seed": 0x1ABE1 + 7 * self.su["seed"] + self.label_steps}

    def frames(self, k=None):
        return {"kind": "frames", "k": int(self.rng.integers(1, 6)) if k is None else k}

    def modes(self):
        return {"kind": "modes", "mip": int(self.rng.integers(0, 4))}


L_SETTERS = ("tf", "region", "window")   # (window where the single window step would only be another new one)
# the two singles a mono seed leaves out to make room for L, by seed % 4 (upload: where M23 brings one; reset: never of a float light volume)
LEFT_OUT = (("cache_clear", "modes"), ("reset", "world"), ("upload", "cache_clear"), ("modes", "world"))


def draw(seed, attempt):
    """(the set-up, the step list) of one draw of a seed. Two adds, then in a seeded order the two blocks every seed has and single
    steps of every other kind; frames last. The blocks:
      M1   frames x 4, a light operator, frames x 1 (served relit), a setter, frames x 1 (marched: nothing recorded is of use)
      M23  change A -> B, change B -> A (both sides' occlusion kept), a setter, change A -> B again (everything kept is stale)
      L    (mono handles) a label volume attached, frames x 1 (the overlay's emptiness merged with the data's), a setter (a region:
           empty bricks filled), frames x 2 .. 4 (merged anew, and no frame served from records), the label volume released. (Stale
           merged emptiness shows only where the setter makes empty bricks hold something: the region setter's "fill" does by
           construction, a tf or window setter where the new curve or window happens to.)
    The setters of M1 and M23 go round window, tf, region, upload with the seed (a region of M1: one brick, the smallest refresh),
    the setter of L round tf, region, window. A mono seed leaves out two of cache_clear, modes, reset, upload, world, in turn."""
    su = setup(seed)
    rng = np.random.default_rng([0x2E7DE2, seed, attempt])
    p = Plan(su, rng)
    rgb, float_light = su["rgb"], su["light32"]
    m1_kind, m23_kind, l_kind = SETTERS[seed % 4], SETTERS[(seed + 1) % 4], L_SETTERS[seed % 3]
    singles = ["world", "view", "window", "tf", "region", "region", "upload", "modes", "cache_clear", "reset"]
    singles.remove(m1_kind)
    if rgb:   # (a colour handle takes no labels and no batch)
        singles += ["light_op", "light_op", "frames"]
    else:     # L brings its setter and its frames: the single setter of its kind (or the second region) and one more single make room
        singles.remove(l_kind if l_kind in singles else "region")
        for it in LEFT_OUT[seed % 4]:
            singles.remove(it)
        singles += ["L", "batch"]
    if float_light:
        singles.remove("reset")   # placed below: behind the fourth light operator
    items = ["M1", "M23"] + singles
    items = [items[i] for i in rng.permutation(len(items))]
    if float_light:   # a float light volume restarts from zeros in mid-sequence: no more operators in a row than the project holds one to
        ops, at = 2, len(items)
        for i, it in enumerate(items):
            ops += {"M1": 1, "M23": 3, "batch": 1, "light_op": 1}.get(it, 0)
            if ops >= 4:
                at = i + 1
                break
        items.insert(at, "reset")
    steps = [p.add(), p.add()]
    window_how = ("same", "ulp", "new")[seed % 3]

    def writes(it):
        """what an item sets that a later light operator or frame reads (M1 begins with frames: it reads before it sets)"""
        if it == "window":
            return set() if window_how == "same" else {"window"}
        return {it} if it in SETTERS else {m23_kind} if it == "M23" else {l_kind} if it == "L" else set()

    # a setter whose work the next setter undoes before anything has read it would go untested (a second window, an upload over a
    # region): such a step waits until a light operator or a frame has read the first — a frame, for a window one float32 further,
    # which no UNORM8 light volume notices
    ordered, waiting, unread = [], [], set()
    while items:
        it = items.pop(0)
        if writes(it) & unread or ("upload" in writes(it) and "region" in unread):
            waiting.append(it)
            continue
        ordered.append(it)
        unread |= writes(it)
        if it in ("M1", "M23", "L", "batch", "light_op", "reset", "frames"):
            unread = {"window"} & unread if window_how == "ulp" and it not in ("M1", "L", "frames") else set()
            items, waiting = waiting + items, []
    for it in ordered + waiting:
        if it == "M1":
            steps += [p.frames(4), p.change("small") if rng.random() < 0.6 else p.light_op(), p.frames(1), p.setter(m1_kind, size="brick"), p.frames(1)]
        elif it == "M23":
            # a fused Change keeps the added light's occlusion, per pass, where the sweep runs the pass (a removal keeps nothing, nor
            # does the chain): of a light with two swept passes, if there is one, turned by a few degrees on the same cube faces
            order = [int(i) for i in rng.permutation(len(p.present))]
            i = next((i for i in order if len(p.swept_faces(p.present[i])) == 2), order[0])
            old = p.present[i]
            for _ in range(8):
                there = turned(rng, old, "small")
                if p.swept_faces(there) == p.swept_faces(old):
                    break
            kept = float_light or (len(p.swept_faces(old)) == 2 and p.swept_faces(there) == p.swept_faces(old))   # (a float light volume: not asked for)
            steps += [{"kind": "change", "old": old, "new": there, "how": "small"}, {"kind": "change", "old": there, "new": old, "how": "back", "kept": kept},
                      p.setter(m23_kind, "cutoffs"), {"kind": "change", "old": old, "new": there, "how": "back"}]
            p.present[i] = there
            p.history[i] += [there, old, there]
        elif it == "L":
            steps += [p.labels_step(), p.frames(1), p.setter(l_kind, size="few", mode="fill"), p.frames(int(rng.integers(2, 5))), p.labels_step()]
        elif it in SETTERS:
            steps.append(p.window_step() if it == "window" else p.setter(it))
        else:
            steps.append({"world": p.world_step, "view": p.view_step, "modes": p.modes, "cache_clear": lambda: {"kind": "cache_clear"}, "frames": p.frames,
                          "reset": p.reset, "light_op": p.light_op, "labels": p.labels_step, "batch": p.batch}[it]())
    steps.append(p.frames())
    assert len(steps) == STEPS, len(steps)
    return su, steps


def oracle_module():
    from oracle import oracle

    oracle.build()
    oracle.load()
    return oracle


def same_lights(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def reaches(steps, trace, i, before):
    """does step i reach (the next light operator's result, the next frame)? The trace against a run that skips the step, from
    `before`: the state in front of it (consumed)"""
    light = frame = None
    for j in range(i + 1, len(steps)):
        e = before.apply(steps[j])
        if "light" in e and light is None:
            light = not same_lights(e["light"], trace[j]["light"])
        if "frame" in e and frame is None:
            frame = not np.array_equal(e["frame"], trace[j]["frame"])
        if light is not None and frame is not None:
            break
    return bool(light), bool(frame)


LABELS_SHOW_BY = 1e-3   # of a pixel's colour or opacity: far above the frames' tolerance, far below a label's opacity of 0.3 and more
SHOWN_FLOOR = 24   # pixels with opacity in every frame of a sequence: no frames step compares empty pictures only


def examine(su, steps, oracle_mod, quick=False):
    """the oracle's trace of a step list, and what the tests ask of it -> (trace, facts):
    "moved": per light operator, did the light volume change; "reached": per setter (window, tf, region, upload), does it reach the
    next light operator's result or the next frame; "reached_light": the former; "shown": per frames step, its pixels with opacity; "labels_shown": per frames step under an attached label
    volume, the pixels the labels move (an attach that shows nothing proves nothing); "relit": per pair of frames
    steps with light operators and nothing else in between, do the two frames differ"""
    st = State(su, oracle_mod)
    trace, facts = [], {"moved": {}, "reached": {}, "reached_light": {}, "shown": {}, "labels_shown": {}, "relit": {}}
    befores = {}
    light = st.lights()
    for i, step in enumerate(steps):
        if step["kind"] in SETTERS:
            befores[i] = st.fork()
        e = st.apply(step)
        trace.append(e)
        if "light" in e:
            facts["moved"][i] = not same_lights(light, e["light"])
            light = e["light"]
        if "frame" in e:
            facts["shown"][i] = int((e["frame"][..., 3] > 0).sum())
            if st.labels is not None:
                facts["labels_shown"][i] = st.labels_shown(LABELS_SHOW_BY)
        if quick and (facts["moved"].get(i) is False or facts["shown"].get(i, SHOWN_FLOOR) < SHOWN_FLOOR or facts["labels_shown"].get(i, SHOWN_FLOOR) < SHOWN_FLOOR):
            return trace, None   # (a draw that is turned down already)
    for i, before in befores.items():
        light, frame = reaches(steps, trace, i, before)
        facts["reached"][i] = light or frame
        facts["reached_light"][i] = light
    last = None
    for i, step in enumerate(steps):
        if step["kind"] == "frames":
            if last is not None and all(s["kind"] in LIGHT_OPS for s in steps[last + 1:i]) and i > last + 1:
                facts["relit"][(last, i)] = not np.array_equal(trace[last]["frame"], trace[i]["frame"])
            last = i
    return trace, facts


def every_frame_shows(su, steps, oracle_mod):
    """do all frames steps show SHOWN_FLOOR pixels? Opacity does not depend on the light: asked of a run without the light
    operators, at the cost of the frames alone"""
    st = State(su, oracle_mod)
    for step in steps:
        if step["kind"] in LIGHT_OPS + ("modes",):
            continue
        e = st.apply(step)
        if "frame" in e and int((e["frame"][..., 3] > 0).sum()) < SHOWN_FLOOR:
            return False
    return True


def acceptable(steps, facts):
    """every light operator moves the light volume, every setter but "the same window again" reaches a result and that one reaches
    none, the setter in front of the stale change reaches that change's result, every frame shows something, and a light operator between two frames shows in the second"""
    stale = motifs(steps).get("both_sides", -2) + 1   # the setter of M23: the change behind it must come out differently for it
    return (all(facts["moved"].values()) and all(facts["reached"][i] == (steps[i].get("how") != "same") for i in facts["reached"])
            and facts["reached_light"].get(stale, False)
            and min(facts["shown"].values()) >= SHOWN_FLOOR and all(n >= SHOWN_FLOOR for n in facts["labels_shown"].values()) and all(facts["relit"].values()) and set(motifs(steps)) == motifs_of(steps))


MOTIFS = ("both_sides", "stale", "relit", "marched")


def motifs_of(steps):
    """the motifs a sequence must hold: a handle that takes labels, "labelled" too"""
    return set(MOTIFS) | ({"labelled"} if any(s["kind"] == "labels" for s in steps) else set())
TRIES = 60
# Where each seed's search begins: its first acceptable draw. Starting there spares every process the oracle's seconds on draws
# that acceptable() turns down; tests/test_render_pipeline_reference.py searches from draw 0 and holds the table to what it finds.
FIRST_DRAW = (8, 0, 15, 18, 16, 1, 1, 6, 4, 1, 0, 3)


def generate(seed, oracle_mod=None):
    """(the set-up, the step list, the oracle's trace, the facts) of a seed: the first of up to TRIES draws that is acceptable (the
    last one, if none is: tests/test_render_pipeline_reference.py then fails)"""
    oracle_mod = oracle_mod or oracle_module()
    for attempt in range(FIRST_DRAW[seed], TRIES):
        su, steps = draw(seed, attempt)
        if attempt < TRIES - 1 and (set(motifs(steps)) != motifs_of(steps) or not every_frame_shows(su, steps, oracle_mod)):
            continue   # (turned down before the oracle has run a light operator)
        trace, facts = examine(su, steps, oracle_mod, quick=attempt < TRIES - 1)
        if facts is not None and acceptable(steps, facts):
            break
    return su, steps, trace, dict(facts, attempts=attempt + 1)


@functools.lru_cache(maxsize=None)
def sequence(seed):
    """generate(seed), once a process: the oracle is the cost of every test that walks a sequence"""
    return generate(seed)


# ---- what the tests ask of a step list ------------------------------------------------------------------------------------------
def motifs(steps):
    """where the motifs lie: {"relit": index of the light operator between frames x 4 and frames x 1, "both_sides": index of the
    change back, "stale": index of the light operator behind a setter, "marched": index of the setter between two frames steps
    behind a relit frame, "labelled": index of the frames step behind a setter under an attached label volume} (a missing one:
    absent)"""
    found = {}
    kinds = [s["kind"] for s in steps]
    attached = False
    for i, s in enumerate(steps):
        if s["kind"] == "labels":
            attached = s["attach"]
        if (0 < i < len(steps) - 1 and kinds[i] in LIGHT_OPS and kinds[i - 1] == "frames" and steps[i - 1]["k"] >= 4 and kinds[i + 1] == "frames"
                and not attached and i - 1 not in CHECKPOINTS and i not in CHECKPOINTS):   # (a checkpoint looks at other views in between)
            found.setdefault("relit", i)
        if (i > 0 and kinds[i] == "change" and kinds[i - 1] == "change" and s["old"] == steps[i - 1]["new"] and s["new"] == steps[i - 1]["old"]
                and s.get("kept", True)):   # ("kept": the generator's word that the sweep, whose occlusion is kept, takes both lights)
            found.setdefault("both_sides", i)
        if i > 0 and kinds[i] in ("remove", "change") and kinds[i - 1] in SETTERS and steps[i - 1].get("how") != "same":
            found.setdefault("stale", i)
        if (0 < i < len(steps) - 1 and kinds[i] in SETTERS and s.get("how") != "same" and kinds[i - 1] == "frames" and kinds[i + 1] == "frames"
                and not attached and "relit" in found):
            found.setdefault("marched", i)
        if (2 < i < len(steps) - 1 and kinds[i] == "frames" and s["k"] >= 2 and kinds[i - 1] in ("window", "tf", "region") and steps[i - 1].get("how") != "same"
                and kinds[i - 2] == "frames" and kinds[i - 3] == "labels" and steps[i - 3]["attach"] and kinds[i + 1] == "labels"):
            found.setdefault("labelled", i)
    return found
