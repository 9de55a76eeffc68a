"""ctypes mirror of include/tbrm.h and a thin handle wrapper over libtbrm.so.

This is plumbing for tests and bench.py: every method is one C-ABI call. There is no Python or CPU
implementation of the path here; if libtbrm.so (the HIP extension) is missing, loading raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TBRM_LIB_PATH") or os.path.join(HERE, "lib", "libtbrm.so")  # override: A/B a second build

# enums (include/tbrm.h)
OK, ERR_INVALID_ARG, ERR_NOT_INITIALIZED, ERR_NO_DEVICE, ERR_OUT_OF_MEMORY, ERR_UNSUPPORTED, ERR_AXES_DIFFER = range(7)
FMT_G8, FMT_G16, FMT_R32_FLOAT = 0, 1, 2
ADDRESS_WRAP, ADDRESS_CLAMP = 0, 1
BORDER_ENGINE_8BIT, BORDER_EXACT_FLOAT = 0, 1

FMT_DTYPE = {FMT_G8: np.uint8, FMT_G16: np.uint16, FMT_R32_FLOAT: np.float32}
DTYPE_FMT = {np.dtype(np.uint8): FMT_G8, np.dtype(np.uint16): FMT_G16, np.dtype(np.float32): FMT_R32_FLOAT}


class Vec3d(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]

    def __init__(self, x=0.0, y=0.0, z=0.0):
        super().__init__(float(x), float(y), float(z))


class Quatd(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double), ("w", C.c_double)]

    def __init__(self, x=0.0, y=0.0, z=0.0, w=1.0):
        super().__init__(float(x), float(y), float(z), float(w))


class Transform(C.Structure):  # FTransform
    _fields_ = [("rotation", Quatd), ("translation", Vec3d), ("scale3d", Vec3d)]


class DirLightParams(C.Structure):  # FDirLightParameters
    _fields_ = [("light_direction", Vec3d), ("light_intensity", C.c_float), ("_pad", C.c_int32)]

    def __init__(self, direction=(0.0, 0.0, 0.0), intensity=0.0):
        super().__init__(Vec3d(*direction), float(intensity), 0)


class ColorDirLight(C.Structure):  # tbrm_color_dir_light (include/tbrm_color_lights.h)
    _fields_ = [("light", DirLightParams), ("color", C.c_float * 3), ("_pad", C.c_int32)]

    def __init__(self, direction=(0.0, 0.0, 0.0), intensity=0.0, color=(1.0, 1.0, 1.0)):
        super().__init__(DirLightParams(direction, intensity), (C.c_float * 3)(*[float(c) for c in color]), 0)


class ClippingPlaneParams(C.Structure):  # FClippingPlaneParameters
    _fields_ = [("center", Vec3d), ("direction", Vec3d)]


class WorldParams(C.Structure):  # FRaymarchWorldParameters
    _fields_ = [("volume_transform", Transform), ("clipping_plane", ClippingPlaneParams)]


class WindowingParams(C.Structure):  # FWindowingParameters
    _fields_ = [("center", C.c_float), ("width", C.c_float), ("low_cutoff", C.c_int32), ("high_cutoff", C.c_int32)]

    def __init__(self, center=0.5, width=1.0, low_cutoff=True, high_cutoff=True):
        super().__init__(float(center), float(width), int(bool(low_cutoff)), int(bool(high_cutoff)))


class ResourcesDesc(C.Structure):
    _fields_ = [("dim_x", C.c_int32), ("dim_y", C.c_int32), ("dim_z", C.c_int32), ("data_format", C.c_int32),
                ("light_volume_32bit", C.c_int32), ("light_volume_half_resolution", C.c_int32),
                ("device", C.c_int32), ("data_address_mode", C.c_int32), ("border_mode", C.c_int32),
                ("_reserved", C.c_int32)]


class Camera(C.Structure):
    _fields_ = [("position", Vec3d), ("forward", Vec3d), ("right", Vec3d), ("up", Vec3d),
                ("tan_half_fov_x", C.c_double), ("tan_half_fov_y", C.c_double),
                ("width", C.c_int32), ("height", C.c_int32)]


class Tile(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("row_group_step", C.c_int32), ("_pad", C.c_int32)]

    def __init__(self, x0=0, y0=0, w=0, h=0, row_group_step=1):
        super().__init__(int(x0), int(y0), int(w), int(h), int(row_group_step), 0)


class RaymarchParams(C.Structure):
    _fields_ = [("steps", C.c_float), ("jitter_frame", C.c_int32), ("enable_skipping", C.c_int32), ("_pad", C.c_int32)]

    def __init__(self, steps=150.0, jitter_frame=-1, enable_skipping=True):
        super().__init__(float(steps), int(jitter_frame), int(bool(enable_skipping)), 0)


class LightPass(C.Structure):
    _fields_ = [("face", C.c_int32), ("axis", C.c_int32), ("weight", C.c_float), ("light_alpha", C.c_float),
                ("border_light", C.c_float), ("prev_pixel_offset", C.c_float * 2), ("uvw_offset", C.c_float * 3),
                ("step_size", C.c_float), ("td", C.c_int32 * 3), ("start", C.c_int32), ("stop", C.c_int32),
                ("dir", C.c_int32)]

    def as_dict(self):
        return {"face": self.face, "axis": self.axis, "weight": self.weight, "light_alpha": self.light_alpha,
                "border_light": self.border_light, "prev_pixel_offset": list(self.prev_pixel_offset),
                "uvw_offset": list(self.uvw_offset), "step_size": self.step_size, "td": list(self.td),
                "start": self.start, "stop": self.stop, "dir": self.dir}


class Slab(C.Structure):  # tbrm_slab: the light-volume z range a handle owns
    _fields_ = [("z_begin", C.c_int32), ("z_end", C.c_int32)]


class SlabPass(C.Structure):  # tbrm_slab_pass
    _fields_ = [("axis", C.c_int32), ("dir", C.c_int32), ("lateral", C.c_int32), ("streams", C.c_int32),
                ("plane_w", C.c_int32), ("plane_h", C.c_int32), ("chunk_slices", C.c_int32), ("chunks_of_pass", C.c_int32),
                ("first_chunk", C.c_int32), ("n_chunks", C.c_int32), ("halo_rows", C.c_int32), ("plane_elem_bytes", C.c_int32)]


# every symbol include/tbrm.h declares (tests/test_abi.py checks the header against this list and the .so)
SYMBOLS = [
    "tbrm_abi_version", "tbrm_version", "tbrm_last_error", "tbrm_device_count", "tbrm_set_tunable", "tbrm_get_tunable",
    "tbrm_resources_create", "tbrm_resources_create_slab", "tbrm_resources_destroy", "tbrm_resources_light_volume_dims",
    "tbrm_resources_is_initialized", "tbrm_upload_volume", "tbrm_upload_volume_device",
    "tbrm_set_tf_lut", "tbrm_color_curve_to_lut", "tbrm_make_default_tf_lut", "tbrm_host_bake_tf_lut", "tbrm_set_windowing",
    "tbrm_resources_reserve", "tbrm_add_dir_light", "tbrm_add_dir_lights", "tbrm_change_dir_light", "tbrm_clear_light_volume",
    "tbrm_slab_light_begin", "tbrm_slab_pass_begin", "tbrm_slab_pass_chunk", "tbrm_slab_pass_plane",
    "tbrm_slab_resident_slices", "tbrm_upload_volume_slices", "tbrm_download_light_slices", "tbrm_slab_light_halo",
    "tbrm_raymarch_lit", "tbrm_raymarch_lit_device", "tbrm_raymarch_lit_slab_device", "tbrm_raymarch_intensity", "tbrm_raymarch_intensity_device",
    "tbrm_generate_octree", "tbrm_octree_mip_dims", "tbrm_download_octree_mip", "tbrm_raymarch_octree", "tbrm_raymarch_octree_device",
    "tbrm_count_nominal_samples",
    "tbrm_download_light_volume", "tbrm_upload_light_volume", "tbrm_light_volume_device_ptr",
    "tbrm_selftest_unorm_decode", "tbrm_selftest_unorm8_roundtrip", "tbrm_selftest_window_division", "tbrm_selftest_opacity_correction", "tbrm_launch_counters", "tbrm_sweep_launches", "tbrm_path_counters", "tbrm_light_cache_stats", "tbrm_light_cache_clear", "tbrm_flush", "tbrm_stream", "tbrm_last_gpu_time_ms",
    "tbrm_host_light_passes", "tbrm_host_plan_light", "tbrm_host_local_clipping", "tbrm_host_data_border", "tbrm_host_world_to_local",
]

ABI_VERSION = 5  # TBRM_ABI_VERSION of include/tbrm.h (tests/test_abi.py compares the two)

# every symbol include/tbrm_labels.h declares (the label overlay; tests/test_labels_abi.py checks the header against this list)
LABEL_SYMBOLS = [
    "tbrm_labels_abi_version", "tbrm_make_default_label_colors", "tbrm_upload_label_volume", "tbrm_update_label_region",
    "tbrm_download_label_volume", "tbrm_set_label_colors", "tbrm_release_label_volume", "tbrm_has_label_volume",
]

LABELS_ABI_VERSION = 1  # TBRM_LABELS_ABI_VERSION of include/tbrm_labels.h

# every symbol include/tbrm_color_lights.h declares (coloured lights; tests/test_color_lights_abi.py checks the header against this list)
COLOR_LIGHT_SYMBOLS = [
    "tbrm_color_lights_abi_version", "tbrm_resources_create_rgb", "tbrm_resources_light_channels", "tbrm_add_color_dir_light",
    "tbrm_change_color_dir_light", "tbrm_download_light_channel", "tbrm_upload_light_channel",
]

COLOR_LIGHTS_ABI_VERSION = 1  # TBRM_COLOR_LIGHTS_ABI_VERSION of include/tbrm_color_lights.h

# every symbol include/tbrm_volume_region.h declares (data-volume region updates; tests/test_volume_region_abi.py checks the header against this list)
VOLUME_REGION_SYMBOLS = [
    "tbrm_volume_region_abi_version", "tbrm_update_volume_region", "tbrm_update_volume_region_device", "tbrm_download_volume_region",
    "tbrm_volume_region_counters", "tbrm_volume_skipping_digest",
]

VOLUME_REGION_ABI_VERSION = 1  # TBRM_VOLUME_REGION_ABI_VERSION of include/tbrm_volume_region.h

# every symbol include/tbrm_volume_stats.h declares (volume statistics; tests/test_volume_stats_abi.py checks the header against this list)
VOLUME_STATS_SYMBOLS = [
    "tbrm_volume_stats_abi_version", "tbrm_volume_histogram", "tbrm_volume_histogram_device", "tbrm_label_statistics",
    "tbrm_host_window_from_histogram", "tbrm_volume_stats_counters",
]

VOLUME_STATS_ABI_VERSION = 1  # TBRM_VOLUME_STATS_ABI_VERSION of include/tbrm_volume_stats.h
HISTOGRAM_MAX_BINS = 4096


class HistogramDesc(C.Structure):  # tbrm_histogram_desc
    _fields_ = [("origin", C.c_int32 * 3), ("extent", C.c_int32 * 3), ("n_bins", C.c_int32), ("use_label_mask", C.c_int32),
                ("lo", C.c_double), ("hi", C.c_double), ("label_mask", C.c_uint32 * 8)]


# tbrm_label_stat, as a numpy record
LABEL_STAT_DTYPE = np.dtype([("count", np.uint64), ("nan_count", np.uint64), ("sum", np.float64), ("min", np.float64), ("max", np.float64)])

# every symbol include/tbrm_view_cache.h declares (the view cache; tests/test_gpu_view_cache.py checks the header against this list)
VIEW_CACHE_SYMBOLS = ["tbrm_view_cache_abi_version", "tbrm_view_cache_stats"]

VIEW_CACHE_ABI_VERSION = 1  # TBRM_VIEW_CACHE_ABI_VERSION of include/tbrm_view_cache.h

# every symbol include/tbrm_hit.h declares (hit maps and picking; tests/test_hit_reference.py checks the header against this list)
HIT_SYMBOLS = [
    "tbrm_hit_abi_version", "tbrm_raymarch_hits_device", "tbrm_raymarch_hits", "tbrm_pick", "tbrm_host_hits_to_world", "tbrm_hit_counters",
]

HIT_ABI_VERSION = 1  # TBRM_HIT_ABI_VERSION of include/tbrm_hit.h

# tbrm_hit, as a numpy record
HIT_DTYPE = np.dtype([("uvw", np.float32, (3,)), ("sample", np.int32), ("alpha", np.float32), ("value", np.float32), ("label", np.int32),
                      ("full_steps", np.int32)])

# every symbol include/tbrm_segment.h declares (seeded region growing; tests/test_segment_abi.py checks the header against this list)
SEGMENT_SYMBOLS = [
    "tbrm_segment_abi_version", "tbrm_grow_region", "tbrm_attach_empty_label_volume", "tbrm_host_hit_voxel", "tbrm_segment_counters",
]

SEGMENT_ABI_VERSION = 1  # TBRM_SEGMENT_ABI_VERSION of include/tbrm_segment.h
GROW_MAX_SEEDS = 4096


class GROW_DESC(C.Structure):  # tbrm_grow_desc
    _fields_ = [("origin", C.c_int32 * 3), ("extent", C.c_int32 * 3), ("connectivity", C.c_int32), ("new_label", C.c_int32),
                ("relative_to_seed", C.c_int32), ("reserved", C.c_int32), ("lo", C.c_double), ("hi", C.c_double), ("writable", C.c_uint32 * 8)]


class GROW_RESULT(C.Structure):  # tbrm_grow_result
    _fields_ = [("voxels", C.c_uint64), ("relabelled", C.c_uint64), ("bbox_min", C.c_int32 * 3), ("bbox_max", C.c_int32 * 3),
                ("passes", C.c_int32), ("seeds_taken", C.c_int32), ("lo_used", C.c_double), ("hi_used", C.c_double)]


# every symbol include/tbrm_morphology.h declares (label morphology; tests/test_morph_abi.py checks the header against this list)
MORPH_SYMBOLS = ["tbrm_morph_abi_version", "tbrm_morph_labels", "tbrm_morph_counters"]

MORPH_ABI_VERSION = 1  # TBRM_MORPH_ABI_VERSION of include/tbrm_morphology.h
MORPH_MAX_RADIUS = 64
MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE = range(4)
MORPH_OPS = {"dilate": MORPH_DILATE, "erode": MORPH_ERODE, "open": MORPH_OPEN, "close": MORPH_CLOSE}


class MORPH_DESC(C.Structure):  # tbrm_morph_desc
    _fields_ = [("origin", C.c_int32 * 3), ("extent", C.c_int32 * 3), ("op", C.c_int32), ("radius", C.c_int32), ("connectivity", C.c_int32),
                ("new_label", C.c_int32), ("erase_label", C.c_int32), ("reserved", C.c_int32), ("source", C.c_uint32 * 8), ("writable", C.c_uint32 * 8)]


class MORPH_RESULT(C.Structure):  # tbrm_morph_result
    _fields_ = [("source_voxels", C.c_uint64), ("result_voxels", C.c_uint64), ("added", C.c_uint64), ("removed", C.c_uint64), ("relabelled", C.c_uint64),
                ("bbox_min", C.c_int32 * 3), ("bbox_max", C.c_int32 * 3), ("launches", C.c_int32), ("reserved", C.c_int32)]


# every symbol include/tbrm_islands.h declares (the islands of a label; tests/test_islands_abi.py checks the header against this list)
ISLANDS_SYMBOLS = ["tbrm_islands_abi_version", "tbrm_label_islands", "tbrm_islands_counters"]

ISLANDS_ABI_VERSION = 1  # TBRM_ISLANDS_ABI_VERSION of include/tbrm_islands.h
ISLANDS_MEASURE = 1      # tbrm_islands_desc::flags
ISLAND_KEPT, ISLAND_BORDER = 1, 2  # tbrm_island::flags
ISLANDS_ANY_SIZE = 0xFFFFFFFFFFFFFFFF  # min_voxels of fill_label_holes: holes of any size


class ISLANDS_DESC(C.Structure):  # tbrm_islands_desc
    _fields_ = [("origin", C.c_int32 * 3), ("extent", C.c_int32 * 3), ("connectivity", C.c_int32), ("max_islands", C.c_int32), ("min_voxels", C.c_uint64),
                ("keep_label", C.c_int32), ("label_step", C.c_int32), ("drop_label", C.c_int32), ("spare_border", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32), ("source", C.c_uint32 * 8)]


class ISLANDS_RESULT(C.Structure):  # tbrm_islands_result
    _fields_ = [("set_voxels", C.c_uint64), ("islands", C.c_uint64), ("spared", C.c_uint64), ("kept", C.c_uint64), ("dropped", C.c_uint64),
                ("kept_voxels", C.c_uint64), ("dropped_voxels", C.c_uint64), ("largest", C.c_uint64), ("relabelled", C.c_uint64),
                ("bbox_min", C.c_int32 * 3), ("bbox_max", C.c_int32 * 3), ("table_entries", C.c_int32), ("reserved", C.c_int32)]


# every symbol include/tbrm_margin.h declares (Euclidean margins of labels; tests/test_margin_abi.py checks the header against this list)
MARGIN_SYMBOLS = ["tbrm_margin_abi_version", "tbrm_margin_labels", "tbrm_label_distance", "tbrm_host_margin_weights", "tbrm_margin_counters"]

MARGIN_ABI_VERSION = 1  # TBRM_MARGIN_ABI_VERSION of include/tbrm_margin.h
MARGIN_MAX_REACH = 64
MARGIN_FAR = 0xFFFFFFFF
MARGIN_EXPAND, MARGIN_SHRINK, MARGIN_OPEN, MARGIN_CLOSE = range(4)
MARGIN_OPS = {"expand": MARGIN_EXPAND, "shrink": MARGIN_SHRINK, "open": MARGIN_OPEN, "close": MARGIN_CLOSE}


class MARGIN_DESC(C.Structure):  # tbrm_margin_desc
    _fields_ = [("origin", C.c_int32 * 3), ("extent", C.c_int32 * 3), ("op", C.c_int32), ("new_label", C.c_int32), ("erase_label", C.c_int32),
                ("reserved", C.c_int32), ("weights", C.c_uint32 * 3), ("limit", C.c_uint32), ("source", C.c_uint32 * 8), ("writable", C.c_uint32 * 8)]


class MARGIN_RESULT(C.Structure):  # tbrm_margin_result
    _fields_ = [("source_voxels", C.c_uint64), ("result_voxels", C.c_uint64), ("added", C.c_uint64), ("removed", C.c_uint64), ("relabelled", C.c_uint64),
                ("bbox_min", C.c_int32 * 3), ("bbox_max", C.c_int32 * 3), ("reach", C.c_int32 * 3), ("launches", C.c_int32)]


def margin_weights(spacing, radius):
    """tbrm_host_margin_weights: the voxel spacing (x, y, z) and a radius in the same unit -> ((w_x, w_y, w_z), limit)"""
    s = (C.c_double * 3)(*[float(v) for v in spacing])
    w, limit = (C.c_uint32 * 3)(), C.c_uint32()
    check(load().tbrm_host_margin_weights(s, float(radius), w, C.byref(limit)))
    return tuple(int(v) for v in w), int(limit.value)


# every symbol include/tbrm_smooth.h declares (smoothing of labels; tests/test_smooth_abi.py checks the header against this list)
SMOOTH_SYMBOLS = ["tbrm_smooth_abi_version", "tbrm_smooth_labels", "tbrm_host_smooth_radii", "tbrm_smooth_counters"]

SMOOTH_ABI_VERSION = 1  # TBRM_SMOOTH_ABI_VERSION of include/tbrm_smooth.h
SMOOTH_MAX_RADIUS = 16
SMOOTH_MAX_ITERATIONS = 64
SMOOTH_MAX_REACH = 64
SMOOTH_MAX_RANK_DEN = 256


class SMOOTH_DESC(C.Structure):  # tbrm_smooth_desc
    _fields_ = [("origin", C.c_int32 * 3), ("extent", C.c_int32 * 3), ("radius", C.c_int32 * 3), ("rank_num", C.c_int32), ("rank_den", C.c_int32),
                ("iterations", C.c_int32), ("new_label", C.c_int32), ("erase_label", C.c_int32), ("reserved", C.c_int32),
                ("source", C.c_uint32 * 8), ("writable", C.c_uint32 * 8)]


class SMOOTH_RESULT(C.Structure):  # tbrm_smooth_result
    _fields_ = [("source_voxels", C.c_uint64), ("result_voxels", C.c_uint64), ("added", C.c_uint64), ("removed", C.c_uint64), ("relabelled", C.c_uint64),
                ("bbox_min", C.c_int32 * 3), ("bbox_max", C.c_int32 * 3), ("reach", C.c_int32 * 3), ("launches", C.c_int32)]


def smooth_radii(spacing, radius):
    """tbrm_host_smooth_radii: the voxel spacing (x, y, z) and a radius in the same unit -> (r_x, r_y, r_z)"""
    s = (C.c_double * 3)(*[float(v) for v in spacing])
    r = (C.c_int32 * 3)()
    check(load().tbrm_host_smooth_radii(s, float(radius), r))
    return tuple(int(v) for v in r)


# every symbol include/tbrm_scissors.h declares (view-space scissors; tests/test_scissors_abi.py checks the header against this list)
SCISSORS_SYMBOLS = ["tbrm_scissors_abi_version", "tbrm_scissors_labels", "tbrm_scissors_counters", "tbrm_host_scissors_projection", "tbrm_host_scissors_polygon"]

SCISSORS_ABI_VERSION = 1  # TBRM_SCISSORS_ABI_VERSION of include/tbrm_scissors.h
SCISSORS_MAX_IMAGE = 16384
SCISSORS_COORD_BITS = 46
SCISSORS_ERASE_INSIDE, SCISSORS_ERASE_OUTSIDE, SCISSORS_FILL_INSIDE, SCISSORS_FILL_OUTSIDE = 0, 1, 2, 3
SCISSORS_OPS = {"erase_inside": SCISSORS_ERASE_INSIDE, "erase_outside": SCISSORS_ERASE_OUTSIDE, "fill_inside": SCISSORS_FILL_INSIDE, "fill_outside": SCISSORS_FILL_OUTSIDE}


class SCISSORS_PROJECTION(C.Structure):  # tbrm_scissors_projection
    _fields_ = [("u", C.c_int64 * 4), ("v", C.c_int64 * 4), ("w", C.c_int64 * 4), ("w_min", C.c_int64), ("w_max", C.c_int64),
                ("width", C.c_int32), ("height", C.c_int32), ("scale_log2", C.c_int32), ("reserved", C.c_int32)]


class SCISSORS_DESC(C.Structure):  # tbrm_scissors_desc
    _fields_ = [("origin", C.c_int32 * 3), ("extent", C.c_int32 * 3), ("op", C.c_int32), ("new_label", C.c_int32), ("erase_label", C.c_int32), ("reserved", C.c_int32),
                ("source", C.c_uint32 * 8), ("writable", C.c_uint32 * 8), ("projection", SCISSORS_PROJECTION)]


class SCISSORS_RESULT(C.Structure):  # tbrm_scissors_result
    _fields_ = [("source_voxels", C.c_uint64), ("result_voxels", C.c_uint64), ("added", C.c_uint64), ("removed", C.c_uint64), ("relabelled", C.c_uint64),
                ("bbox_min", C.c_int32 * 3), ("bbox_max", C.c_int32 * 3), ("bricks_inside", C.c_int32), ("bricks_outside", C.c_int32),
                ("bricks_projected", C.c_int32), ("launches", C.c_int32)]


# every symbol include/tbrm_compete.h declares (competitive growing from seed labels; tests/test_compete_abi.py checks the header against this list)
COMPETE_SYMBOLS = ["tbrm_compete_abi_version", "tbrm_compete_labels", "tbrm_host_compete_float_range", "tbrm_compete_counters"]

COMPETE_ABI_VERSION = 1  # TBRM_COMPETE_ABI_VERSION of include/tbrm_compete.h
COMPETE_MAX_COST = 0xFFFFFF
COMPETE_MAX_STEP_COST = 65535
COMPETE_MAX_SHIFT = 16
COMPETE_NO_COST = 0xFFFFFFFF


class COMPETE_DESC(C.Structure):  # tbrm_compete_desc
    _fields_ = [("origin", C.c_int32 * 3), ("extent", C.c_int32 * 3), ("connectivity", C.c_int32), ("measure_only", C.c_int32), ("step_cost", C.c_int32 * 3),
                ("value_shift", C.c_int32), ("cost_limit", C.c_uint32), ("reserved", C.c_int32), ("lo", C.c_double), ("hi", C.c_double),
                ("float_origin", C.c_float), ("float_scale", C.c_float), ("seeds", C.c_uint32 * 8), ("writable", C.c_uint32 * 8)]


class COMPETE_RESULT(C.Structure):  # tbrm_compete_result
    _fields_ = [("seed_voxels", C.c_uint64), ("claimable", C.c_uint64), ("claimed", C.c_uint64), ("relabelled", C.c_uint64), ("claimed_per_label", C.c_uint64 * 256),
                ("max_cost", C.c_uint32), ("passes", C.c_int32), ("bbox_min", C.c_int32 * 3), ("bbox_max", C.c_int32 * 3)]


# every symbol include/tbrm_paint.h declares (the 3D paint brush; tests/test_paint_abi.py checks the header against this list)
PAINT_SYMBOLS = ["tbrm_paint_abi_version", "tbrm_paint_labels", "tbrm_paint_counters", "tbrm_host_paint_brush", "tbrm_host_paint_stroke"]

PAINT_ABI_VERSION = 1  # TBRM_PAINT_ABI_VERSION of include/tbrm_paint.h
PAINT_MAX_POINTS = 4096
PAINT_MAX_COORD = 1 << 18
PAINT_MAX_DIM = 16384
PAINT_MAX_WEIGHT = 65535
PAINT_MAX_LIMIT = (1 << 30) - 1
PAINT_MAX_REACH = 64
PAINT_PAINT, PAINT_ERASE = 0, 1
PAINT_OPS = {"paint": PAINT_PAINT, "erase": PAINT_ERASE}


class PAINT_DESC(C.Structure):  # tbrm_paint_desc
    _fields_ = [("origin", C.c_int32 * 3), ("extent", C.c_int32 * 3), ("op", C.c_int32), ("new_label", C.c_int32), ("erase_label", C.c_int32), ("gate", C.c_int32),
                ("weights", C.c_uint32 * 3), ("limit", C.c_uint32), ("lo", C.c_double), ("hi", C.c_double), ("source", C.c_uint32 * 8), ("writable", C.c_uint32 * 8)]


class PAINT_RESULT(C.Structure):  # tbrm_paint_result
    _fields_ = [("stamp_voxels", C.c_uint64), ("added", C.c_uint64), ("removed", C.c_uint64), ("relabelled", C.c_uint64), ("bbox_min", C.c_int32 * 3),
                ("bbox_max", C.c_int32 * 3), ("segments", C.c_int32), ("bricks_whole", C.c_int32), ("bricks_untouched", C.c_int32), ("bricks_evaluated", C.c_int32),
                ("launches", C.c_int32), ("reserved", C.c_int32)]


# every symbol include/tbrm_surface.h declares (the surface of a label as a mesh; tests/test_surface_abi.py checks the header against this list)
SURFACE_SYMBOLS = ["tbrm_surface_abi_version", "tbrm_label_surface", "tbrm_label_surface_device", "tbrm_surface_counters", "tbrm_host_surface_positions",
                   "tbrm_host_surface_unit_cube"]

SURFACE_ABI_VERSION = 1  # TBRM_SURFACE_ABI_VERSION of include/tbrm_surface.h
SURFACE_MAX_DIM = 1 << 19
SURFACE_TRIANGLES, SURFACE_MEASURE = 1, 2
# tbrm_surface_vertex as a numpy record
SURFACE_VERTEX_DTYPE = np.dtype([("cell", "<i4", 3), ("sum", "u1", 3), ("edges", "u1"), ("normal", "i1", 3), ("corners", "u1")])


class SURFACE_VERTEX(C.Structure):  # tbrm_surface_vertex
    _fields_ = [("cell", C.c_int32 * 3), ("sum", C.c_uint8 * 3), ("edges", C.c_uint8), ("normal", C.c_int8 * 3), ("corners", C.c_uint8)]


class SURFACE_DESC(C.Structure):  # tbrm_surface_desc
    _fields_ = [("origin", C.c_int32 * 3), ("extent", C.c_int32 * 3), ("flags", C.c_uint32), ("reserved", C.c_int32), ("vertex_capacity", C.c_uint64),
                ("quad_capacity", C.c_uint64), ("scale", C.c_float * 3), ("offset", C.c_float * 3), ("source", C.c_uint32 * 8)]


class SURFACE_RESULT(C.Structure):  # tbrm_surface_result
    _fields_ = [("set_voxels", C.c_uint64), ("vertices", C.c_uint64), ("quads", C.c_uint64), ("quads_axis", C.c_uint64 * 3), ("cell_min", C.c_int32 * 3),
                ("cell_max", C.c_int32 * 3), ("blocks_evaluated", C.c_int32), ("blocks_skipped", C.c_int32), ("launches", C.c_int32), ("written", C.c_int32),
                ("reserved", C.c_int32)]


def surface_unit_cube(dims):
    """tbrm_host_surface_unit_cube: (scale, offset) that put voxel i at i / (N - 1), as float32 triples"""
    d = (C.c_int32 * 3)(*[int(v) for v in dims])
    scale, offset = (C.c_float * 3)(), (C.c_float * 3)()
    check(load().tbrm_host_surface_unit_cube(d, scale, offset))
    return tuple(np.float32(v) for v in scale), tuple(np.float32(v) for v in offset)


def surface_positions(vertices, scale=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0)):
    """tbrm_host_surface_positions: the float32 positions [n, 3] of vertex records (SURFACE_VERTEX_DTYPE)"""
    v = np.ascontiguousarray(np.asarray(vertices, dtype=SURFACE_VERTEX_DTYPE).reshape(-1))
    out = np.zeros((v.shape[0], 3), dtype=np.float32)
    sc = (C.c_float * 3)(*[float(x) for x in scale])
    of = (C.c_float * 3)(*[float(x) for x in offset])
    check(load().tbrm_host_surface_positions(v.ctypes.data_as(C.c_void_p), v.shape[0], sc, of, out.ctypes.data_as(C.c_void_p)))
    return out


def paint_brush(spacing, radius):
    """tbrm_host_paint_brush: (weights, limit) of a brush of `radius` on voxels of `spacing` (x, y, z; the same unit)"""
    sp = (C.c_double * 3)(*[float(v) for v in spacing])
    w, limit = (C.c_uint32 * 3)(), C.c_uint32()
    check(load().tbrm_host_paint_brush(sp, float(radius), w, C.byref(limit)))
    return tuple(int(v) for v in w), int(limit.value)


def paint_stroke(dims, uvw, weights, capacity=None):
    """tbrm_host_paint_stroke: unit-cube positions [n, 3] (a hit map's uvw) -> the stroke's points, int32 [m, 3] in eighths of a voxel;
    capacity: the room offered (None: whatever the stroke needs)"""
    d = (C.c_int32 * 3)(*[int(v) for v in dims])
    w = (C.c_uint32 * 3)(*[int(v) for v in weights])
    pos = np.ascontiguousarray(np.asarray(uvw, dtype=np.float32).reshape(-1, 3))
    n_out = C.c_size_t()
    lib = load()
    if capacity is None:
        code = lib.tbrm_host_paint_stroke(d, pos.ctypes.data_as(C.c_void_p), pos.shape[0], w, None, 0, C.byref(n_out))
        if n_out.value == 0:
            check(code)
        capacity = n_out.value
    out = np.zeros((int(capacity), 3), dtype=np.int32)
    check(lib.tbrm_host_paint_stroke(d, pos.ctypes.data_as(C.c_void_p), pos.shape[0], w, out.ctypes.data_as(C.c_void_p), int(capacity), C.byref(n_out)))
    return out[:n_out.value]


def compete_float_range(lo, hi):
    """tbrm_host_compete_float_range: (float_origin, float_scale) that map the values [lo, hi] onto the codes 0 .. 65535"""
    o, s = C.c_float(), C.c_float()
    check(load().tbrm_host_compete_float_range(float(lo), float(hi), C.byref(o), C.byref(s)))
    return o.value, s.value


def scissors_mask_shape(width, height):
    """a mask as numpy: uint32 [height, ceil(width / 32)]; pixel px of row py is bit px & 31 of [py, px >> 5]"""
    return int(height), (int(width) + 31) // 32


def make_scissors_projection(u, v, w, w_min, w_max, width, height):
    """hand-made rows: u, v, w are four integers each"""
    p = SCISSORS_PROJECTION()
    p.u[:], p.v[:], p.w[:] = [int(a) for a in u], [int(a) for a in v], [int(a) for a in w]
    p.w_min, p.w_max, p.width, p.height = int(w_min), int(w_max), int(width), int(height)
    return p


def scissors_projection(dims, world, camera, depth_min=0.0, depth_max=float("inf")):
    """tbrm_host_scissors_projection: the integer rows of `camera` for a volume of dims (x, y, z) under world's volume transform;
    depth_min, depth_max: world units along the camera's forward (a hit map's depth)"""
    d = (C.c_int32 * 3)(*[int(v) for v in dims])
    out = SCISSORS_PROJECTION()
    check(load().tbrm_host_scissors_projection(d, C.byref(world), C.byref(camera), float(depth_min), float(depth_max), C.byref(out)))
    return out


def scissors_polygon(points, width, height):
    """tbrm_host_scissors_polygon: the lasso through `points` ((x, y) in pixels of the view) as a mask (scissors_mask_shape)"""
    xy = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 2))
    mask = np.zeros(scissors_mask_shape(width, height), dtype=np.uint32)
    check(load().tbrm_host_scissors_polygon(xy.ctypes.data_as(C.c_void_p), xy.shape[0], int(width), int(height), mask.ctypes.data_as(C.c_void_p), mask.size))
    return mask


class ISLAND(C.Structure):  # tbrm_island
    _fields_ = [("voxels", C.c_uint64), ("first", C.c_int32 * 3), ("label", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


_lib = None


class TbrmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"tbrm error {code}: {msg}")
        self.code = code


def load():
    """Loads libtbrm.so. Fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension with `python tbraymarcherplugin_amd/build.py` "
            "(__graft_entry__.build()). There is no CPU fallback for this path.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    # include/tbrm.h: a host built against another TBRM_ABI_VERSION must not call in (a stale libtbrm.so that build.py's
    # time-stamp check let through would otherwise be used silently)
    have = lib.tbrm_abi_version() if hasattr(lib, "tbrm_abi_version") else -1
    if have != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI version {have}, this binding is written against {ABI_VERSION}: rebuild it "
                          "(`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_version.restype = C.c_char_p
    lib.tbrm_last_error.restype = C.c_char_p
    lib.tbrm_host_data_border.restype = C.c_float
    lib.tbrm_host_data_border.argtypes = [C.POINTER(WindowingParams), C.c_int]
    P = C.POINTER
    vp = C.c_void_p
    lib.tbrm_device_count.argtypes = [P(C.c_int)]
    lib.tbrm_set_tunable.argtypes = [C.c_char_p, C.c_int32]
    lib.tbrm_get_tunable.argtypes = [C.c_char_p, P(C.c_int32)]
    lib.tbrm_resources_create.argtypes = [P(ResourcesDesc), P(vp)]
    lib.tbrm_resources_create_slab.argtypes = [P(ResourcesDesc), P(Slab), P(vp)]
    lib.tbrm_slab_resident_slices.argtypes = [vp, P(C.c_int32 * 3), P(C.c_int32 * 3)]
    lib.tbrm_upload_volume_slices.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_size_t]
    lib.tbrm_download_light_slices.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_size_t]
    lib.tbrm_slab_light_halo.argtypes = [vp, C.c_int32, P(vp), P(vp), P(C.c_size_t)]
    lib.tbrm_resources_destroy.argtypes = [vp]
    lib.tbrm_resources_light_volume_dims.argtypes = [vp, P(C.c_int32 * 3)]
    lib.tbrm_resources_is_initialized.argtypes = [vp]
    lib.tbrm_upload_volume.argtypes = [vp, vp, C.c_size_t]
    lib.tbrm_upload_volume_device.argtypes = [vp, vp, C.c_size_t]
    lib.tbrm_set_tf_lut.argtypes = [vp, vp]
    lib.tbrm_color_curve_to_lut.argtypes = [P(vp * 4), P(vp * 4), P(C.c_int32 * 4), vp]
    lib.tbrm_make_default_tf_lut.argtypes = [vp]
    lib.tbrm_host_bake_tf_lut.argtypes = [vp, vp]
    lib.tbrm_set_windowing.argtypes = [vp, P(WindowingParams)]
    lib.tbrm_add_dir_light.argtypes = [vp, P(DirLightParams), C.c_int, P(WorldParams), P(C.c_int), C.c_int]
    lib.tbrm_add_dir_lights.argtypes = [vp, vp, C.c_int32, C.c_int, P(WorldParams), vp, P(C.c_int32)]
    lib.tbrm_change_dir_light.argtypes = [vp, P(DirLightParams), P(DirLightParams), P(WorldParams), P(C.c_int), C.c_int]
    lib.tbrm_clear_light_volume.argtypes = [vp, C.c_float]
    lib.tbrm_slab_light_begin.argtypes = [vp, P(DirLightParams), P(DirLightParams), C.c_int, P(WorldParams), P(Slab), P(C.c_int32)]
    lib.tbrm_slab_pass_begin.argtypes = [vp, C.c_int32, P(SlabPass)]
    lib.tbrm_slab_pass_chunk.argtypes = [vp, C.c_int32]
    lib.tbrm_slab_pass_plane.argtypes = [vp, C.c_int32, C.c_int32, P(vp)]
    lib.tbrm_raymarch_lit.argtypes = [vp, P(Camera), P(Tile), P(RaymarchParams), P(WorldParams), vp]
    lib.tbrm_raymarch_lit_device.argtypes = [vp, P(Camera), P(Tile), P(RaymarchParams), P(WorldParams), vp, vp]
    lib.tbrm_raymarch_lit_slab_device.argtypes = [vp, P(Camera), P(Tile), P(RaymarchParams), P(WorldParams), vp, vp, P(Slab), C.c_int]
    lib.tbrm_raymarch_intensity.argtypes = [vp, P(Camera), P(Tile), P(RaymarchParams), P(WorldParams), vp]
    lib.tbrm_raymarch_intensity_device.argtypes = [vp, P(Camera), P(Tile), P(RaymarchParams), P(WorldParams), vp, vp]
    lib.tbrm_generate_octree.argtypes = [vp]
    lib.tbrm_octree_mip_dims.argtypes = [vp, C.c_int, P(C.c_int32 * 3)]
    lib.tbrm_download_octree_mip.argtypes = [vp, C.c_int, vp, C.c_size_t]
    lib.tbrm_raymarch_octree.argtypes = [vp, P(Camera), P(Tile), P(RaymarchParams), P(WorldParams), C.c_int, vp]
    lib.tbrm_raymarch_octree_device.argtypes = [vp, P(Camera), P(Tile), P(RaymarchParams), P(WorldParams), C.c_int, vp, vp]
    lib.tbrm_count_nominal_samples.argtypes = [vp, P(Camera), P(Tile), P(RaymarchParams), P(WorldParams), P(C.c_uint64)]
    lib.tbrm_download_light_volume.argtypes = [vp, vp, C.c_size_t]
    lib.tbrm_upload_light_volume.argtypes = [vp, vp, C.c_size_t]
    lib.tbrm_light_volume_device_ptr.argtypes = [vp, P(vp), P(C.c_size_t)]
    lib.tbrm_launch_counters.argtypes = [vp, P(C.c_uint64 * 3)]
    lib.tbrm_sweep_launches.argtypes = [vp, P(C.c_uint64)]
    lib.tbrm_path_counters.argtypes = [vp, P(C.c_uint64 * 16)]
    lib.tbrm_resources_reserve.argtypes = [vp, C.c_int32, C.c_uint32]
    lib.tbrm_selftest_unorm_decode.argtypes = [C.c_int, vp, vp]
    lib.tbrm_selftest_unorm8_roundtrip.argtypes = [C.c_int, vp, C.c_size_t, vp]
    lib.tbrm_selftest_window_division.argtypes = [C.c_int, C.c_float, C.c_float, P(C.c_uint64), P(C.c_int)]
    lib.tbrm_selftest_opacity_correction.argtypes = [C.c_int, C.c_float, C.c_float, P(C.c_uint64)]
    lib.tbrm_flush.argtypes = [vp]
    lib.tbrm_stream.argtypes = [vp, P(vp)]
    lib.tbrm_last_gpu_time_ms.argtypes = [vp, C.c_int, P(C.c_float)]
    lib.tbrm_host_light_passes.argtypes = [P(DirLightParams), P(WorldParams), P(C.c_int32 * 3), C.c_int, P(LightPass * 2), P(C.c_int)]
    lib.tbrm_host_plan_light.argtypes = [P(DirLightParams), P(WorldParams), P(C.c_int32 * 3), C.c_int, P(C.c_int32 * 8), P(C.c_int)]
    lib.tbrm_host_local_clipping.argtypes = [P(WorldParams), P(C.c_float * 3), P(C.c_float * 3)]
    lib.tbrm_host_world_to_local.argtypes = [P(Transform), P(C.c_float * 12)]
    have = lib.tbrm_labels_abi_version() if hasattr(lib, "tbrm_labels_abi_version") else -1
    if have != LABELS_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has label ABI version {have}, this binding is written against {LABELS_ABI_VERSION}: rebuild it "
                          "(`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_make_default_label_colors.argtypes = [vp]
    lib.tbrm_upload_label_volume.argtypes = [vp, vp, C.c_size_t]
    lib.tbrm_update_label_region.argtypes = [vp, P(C.c_int32 * 3), P(C.c_int32 * 3), vp, C.c_size_t]
    lib.tbrm_download_label_volume.argtypes = [vp, vp, C.c_size_t]
    lib.tbrm_set_label_colors.argtypes = [vp, vp]
    lib.tbrm_release_label_volume.argtypes = [vp]
    lib.tbrm_has_label_volume.argtypes = [vp]
    have = lib.tbrm_color_lights_abi_version() if hasattr(lib, "tbrm_color_lights_abi_version") else -1
    if have != COLOR_LIGHTS_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has colour-light ABI version {have}, this binding is written against {COLOR_LIGHTS_ABI_VERSION}: "
                          "rebuild it (`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_resources_create_rgb.argtypes = [P(ResourcesDesc), P(vp)]
    lib.tbrm_resources_light_channels.argtypes = [vp]
    lib.tbrm_add_color_dir_light.argtypes = [vp, P(ColorDirLight), C.c_int, P(WorldParams), P(C.c_int)]
    lib.tbrm_change_color_dir_light.argtypes = [vp, P(ColorDirLight), P(ColorDirLight), P(WorldParams), P(C.c_int)]
    lib.tbrm_download_light_channel.argtypes = [vp, C.c_int, vp, C.c_size_t]
    lib.tbrm_upload_light_channel.argtypes = [vp, C.c_int, vp, C.c_size_t]
    have = lib.tbrm_volume_region_abi_version() if hasattr(lib, "tbrm_volume_region_abi_version") else -1
    if have != VOLUME_REGION_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has volume-region ABI version {have}, this binding is written against {VOLUME_REGION_ABI_VERSION}: "
                          "rebuild it (`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_update_volume_region.argtypes = [vp, P(C.c_int32 * 3), P(C.c_int32 * 3), vp, C.c_size_t]
    lib.tbrm_update_volume_region_device.argtypes = [vp, P(C.c_int32 * 3), P(C.c_int32 * 3), vp, C.c_size_t]
    lib.tbrm_download_volume_region.argtypes = [vp, P(C.c_int32 * 3), P(C.c_int32 * 3), vp, C.c_size_t]
    lib.tbrm_volume_region_counters.argtypes = [vp, P(C.c_uint64 * 4)]
    lib.tbrm_volume_skipping_digest.argtypes = [vp, P(C.c_uint64 * 4)]
    have = lib.tbrm_volume_stats_abi_version() if hasattr(lib, "tbrm_volume_stats_abi_version") else -1
    if have != VOLUME_STATS_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has volume-statistics ABI version {have}, this binding is written against {VOLUME_STATS_ABI_VERSION}: "
                          "rebuild it (`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_volume_histogram.argtypes = [vp, P(HistogramDesc), vp, P(C.c_uint64 * 4)]
    lib.tbrm_volume_histogram_device.argtypes = [vp, P(HistogramDesc), vp]
    lib.tbrm_label_statistics.argtypes = [vp, P(C.c_int32 * 3), P(C.c_int32 * 3), vp]
    lib.tbrm_host_window_from_histogram.argtypes = [vp, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, P(WindowingParams)]
    lib.tbrm_volume_stats_counters.argtypes = [vp, P(C.c_uint64 * 4)]
    have = lib.tbrm_view_cache_abi_version() if hasattr(lib, "tbrm_view_cache_abi_version") else -1
    if have != VIEW_CACHE_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has view-cache ABI version {have}, this binding is written against {VIEW_CACHE_ABI_VERSION}: "
                          "rebuild it (`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_view_cache_stats.argtypes = [vp, P(C.c_uint64 * 6)]
    have = lib.tbrm_hit_abi_version() if hasattr(lib, "tbrm_hit_abi_version") else -1
    if have != HIT_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has hit ABI version {have}, this binding is written against {HIT_ABI_VERSION}: rebuild it "
                          "(`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_raymarch_hits_device.argtypes = [vp, P(Camera), P(Tile), P(RaymarchParams), P(WorldParams), C.c_float, vp, vp, vp]
    lib.tbrm_raymarch_hits.argtypes = [vp, P(Camera), P(Tile), P(RaymarchParams), P(WorldParams), C.c_float, vp, vp]
    lib.tbrm_pick.argtypes = [vp, P(Camera), C.c_int32, C.c_int32, P(RaymarchParams), P(WorldParams), C.c_float, vp, P(C.c_double * 3), P(C.c_double)]
    lib.tbrm_host_hits_to_world.argtypes = [P(WorldParams), P(Camera), vp, C.c_size_t, vp, vp]
    lib.tbrm_hit_counters.argtypes = [vp, P(C.c_uint64 * 3)]
    have = lib.tbrm_segment_abi_version() if hasattr(lib, "tbrm_segment_abi_version") else -1
    if have != SEGMENT_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has segment ABI version {have}, this binding is written against {SEGMENT_ABI_VERSION}: rebuild it "
                          "(`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_grow_region.argtypes = [vp, P(GROW_DESC), vp, C.c_int32, P(GROW_RESULT)]
    lib.tbrm_attach_empty_label_volume.argtypes = [vp]
    lib.tbrm_host_hit_voxel.argtypes = [P(C.c_int32 * 3), vp, P(C.c_int32 * 3)]
    lib.tbrm_segment_counters.argtypes = [vp, P(C.c_uint64 * 4)]
    have = lib.tbrm_morph_abi_version() if hasattr(lib, "tbrm_morph_abi_version") else -1
    if have != MORPH_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has morphology ABI version {have}, this binding is written against {MORPH_ABI_VERSION}: rebuild it "
                          "(`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_morph_labels.argtypes = [vp, P(MORPH_DESC), P(MORPH_RESULT)]
    lib.tbrm_morph_counters.argtypes = [vp, P(C.c_uint64 * 4)]
    have = lib.tbrm_islands_abi_version() if hasattr(lib, "tbrm_islands_abi_version") else -1
    if have != ISLANDS_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has islands ABI version {have}, this binding is written against {ISLANDS_ABI_VERSION}: rebuild it "
                          "(`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_label_islands.argtypes = [vp, P(ISLANDS_DESC), P(ISLAND), C.c_int32, P(ISLANDS_RESULT)]
    lib.tbrm_islands_counters.argtypes = [vp, P(C.c_uint64 * 6)]
    have = lib.tbrm_margin_abi_version() if hasattr(lib, "tbrm_margin_abi_version") else -1
    if have != MARGIN_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has margin ABI version {have}, this binding is written against {MARGIN_ABI_VERSION}: rebuild it "
                          "(`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_margin_labels.argtypes = [vp, P(MARGIN_DESC), P(MARGIN_RESULT)]
    lib.tbrm_label_distance.argtypes = [vp, P(MARGIN_DESC), C.c_int32, vp, C.c_size_t]
    lib.tbrm_host_margin_weights.argtypes = [P(C.c_double * 3), C.c_double, P(C.c_uint32 * 3), P(C.c_uint32)]
    lib.tbrm_margin_counters.argtypes = [vp, P(C.c_uint64 * 4)]
    have = lib.tbrm_smooth_abi_version() if hasattr(lib, "tbrm_smooth_abi_version") else -1
    if have != SMOOTH_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has smooth ABI version {have}, this binding is written against {SMOOTH_ABI_VERSION}: rebuild it "
                          "(`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_smooth_labels.argtypes = [vp, P(SMOOTH_DESC), P(SMOOTH_RESULT)]
    lib.tbrm_host_smooth_radii.argtypes = [P(C.c_double * 3), C.c_double, P(C.c_int32 * 3)]
    lib.tbrm_smooth_counters.argtypes = [vp, P(C.c_uint64 * 4)]
    have = lib.tbrm_scissors_abi_version() if hasattr(lib, "tbrm_scissors_abi_version") else -1
    if have != SCISSORS_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has scissors ABI version {have}, this binding is written against {SCISSORS_ABI_VERSION}: rebuild it "
                          "(`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_scissors_labels.argtypes = [vp, P(SCISSORS_DESC), vp, C.c_size_t, P(SCISSORS_RESULT)]
    lib.tbrm_scissors_counters.argtypes = [vp, P(C.c_uint64 * 4)]
    lib.tbrm_host_scissors_projection.argtypes = [P(C.c_int32 * 3), P(WorldParams), P(Camera), C.c_double, C.c_double, P(SCISSORS_PROJECTION)]
    lib.tbrm_host_scissors_polygon.argtypes = [vp, C.c_size_t, C.c_int32, C.c_int32, vp, C.c_size_t]
    have = lib.tbrm_compete_abi_version() if hasattr(lib, "tbrm_compete_abi_version") else -1
    if have != COMPETE_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has compete ABI version {have}, this binding is written against {COMPETE_ABI_VERSION}: rebuild it "
                          "(`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_compete_labels.argtypes = [vp, P(COMPETE_DESC), vp, P(COMPETE_RESULT)]
    lib.tbrm_host_compete_float_range.argtypes = [C.c_double, C.c_double, P(C.c_float), P(C.c_float)]
    lib.tbrm_compete_counters.argtypes = [vp, P(C.c_uint64 * 4)]
    have = lib.tbrm_paint_abi_version() if hasattr(lib, "tbrm_paint_abi_version") else -1
    if have != PAINT_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has paint ABI version {have}, this binding is written against {PAINT_ABI_VERSION}: rebuild it "
                          "(`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_paint_labels.argtypes = [vp, P(PAINT_DESC), vp, C.c_size_t, P(PAINT_RESULT)]
    lib.tbrm_paint_counters.argtypes = [vp, P(C.c_uint64 * 4)]
    lib.tbrm_host_paint_brush.argtypes = [P(C.c_double * 3), C.c_double, P(C.c_uint32 * 3), P(C.c_uint32)]
    lib.tbrm_host_paint_stroke.argtypes = [P(C.c_int32 * 3), vp, C.c_size_t, P(C.c_uint32 * 3), vp, C.c_size_t, P(C.c_size_t)]
    have = lib.tbrm_surface_abi_version() if hasattr(lib, "tbrm_surface_abi_version") else -1
    if have != SURFACE_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has surface ABI version {have}, this binding is written against {SURFACE_ABI_VERSION}: rebuild it "
                          "(`python tbraymarcherplugin_amd/build.py --force`)")
    lib.tbrm_label_surface.argtypes = [vp, P(SURFACE_DESC), vp, vp, vp, P(SURFACE_RESULT)]
    lib.tbrm_label_surface_device.argtypes = [vp, P(SURFACE_DESC), vp, vp, vp, P(SURFACE_RESULT)]
    lib.tbrm_surface_counters.argtypes = [vp, P(C.c_uint64 * 6)]
    lib.tbrm_host_surface_positions.argtypes = [vp, C.c_size_t, P(C.c_float * 3), P(C.c_float * 3), vp]
    lib.tbrm_host_surface_unit_cube.argtypes = [P(C.c_int32 * 3), P(C.c_float * 3), P(C.c_float * 3)]
    _lib = lib
    return lib


def check(code):
    if code != OK:
        raise TbrmError(code, load().tbrm_last_error().decode())


def identity_transform(scale=100.0, translation=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.0, 1.0)):
    """The cube mesh component's transform; scale 100 = WorldDimensions/10 of a unit cube (RaymarchVolume.cpp:47)."""
    s = (scale, scale, scale) if np.isscalar(scale) else scale
    return Transform(Quatd(*rotation), Vec3d(*translation), Vec3d(*s))


def make_world(transform=None, clip_center=(0.0, 0.0, 100000.0), clip_direction=(0.0, 0.0, -1.0)):
    """FRaymarchWorldParameters; the defaults are the 'no clipping plane' values of RaymarchVolume.cpp:637-642."""
    return WorldParams(transform if transform is not None else identity_transform(),
                       ClippingPlaneParams(Vec3d(*clip_center), Vec3d(*clip_direction)))


def look_at_camera(eye, target, up, vfov_deg, width, height):
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    thy = np.tan(np.deg2rad(vfov_deg) / 2.0)
    thx = thy * width / height
    return Camera(Vec3d(*eye), Vec3d(*f), Vec3d(*r), Vec3d(*u), thx, thy, int(width), int(height))


def host_light_passes(light, world, lv_dims, border_mode=BORDER_ENGINE_8BIT):
    out = (LightPass * 2)()
    n = C.c_int(0)
    dims = (C.c_int32 * 3)(*lv_dims)
    check(load().tbrm_host_light_passes(C.byref(light), C.byref(world), C.byref(dims), border_mode, C.byref(out), C.byref(n)))
    return [out[0], out[1]], n.value


def host_plan_light(light, world, lv_dims, light_32bit=False):
    """The planner alone (no device): per axis pass of AddDirLight(light) (path, a, b, why) — path 0 sweep / 1 chain / 2 slice."""
    out = (C.c_int32 * 8)()
    n = C.c_int(0)
    dims = (C.c_int32 * 3)(*lv_dims)
    check(load().tbrm_host_plan_light(C.byref(light), C.byref(world), C.byref(dims), int(bool(light_32bit)), C.byref(out), C.byref(n)))
    return [tuple(out[4 * k:4 * k + 4]) for k in range(n.value)]


def host_local_clipping(world):
    c, d = (C.c_float * 3)(), (C.c_float * 3)()
    check(load().tbrm_host_local_clipping(C.byref(world), C.byref(c), C.byref(d)))
    return np.array(c[:], dtype=np.float32), np.array(d[:], dtype=np.float32)


def host_world_to_local(transform):
    m = (C.c_float * 12)()
    check(load().tbrm_host_world_to_local(C.byref(transform), C.byref(m)))
    return np.array(m[:], dtype=np.float32)


def host_data_border(windowing, border_mode=BORDER_ENGINE_8BIT):
    return float(load().tbrm_host_data_border(C.byref(windowing), border_mode))


def color_curve_to_lut(keys):
    """keys: 4 (times, values) pairs, R,G,B,A. Returns the 256x4 float LUT ColorCurveToTexture samples."""
    arrs = [(np.ascontiguousarray(t, dtype=np.float32), np.ascontiguousarray(v, dtype=np.float32)) for t, v in keys]
    times = (C.c_void_p * 4)(*[a[0].ctypes.data for a in arrs])
    vals = (C.c_void_p * 4)(*[a[1].ctypes.data for a in arrs])
    n = (C.c_int32 * 4)(*[len(a[0]) for a in arrs])
    out = np.empty((256, 4), dtype=np.float32)
    check(load().tbrm_color_curve_to_lut(C.byref(times), C.byref(vals), C.byref(n), out.ctypes.data))
    return out


def make_default_tf_lut():
    out = np.empty((256, 4), dtype=np.float32)
    check(load().tbrm_make_default_tf_lut(out.ctypes.data))
    return out


def window_from_histogram(counts, lo_edge, hi_edge, p_low=0.01, p_high=0.99):
    """tbrm_host_window_from_histogram: the percentile window of a histogram whose bins span [lo_edge, hi_edge) in the window's
    units (include/tbrm_volume_stats.h has the rule). Host arithmetic: needs no device."""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    out = WindowingParams()
    check(load().tbrm_host_window_from_histogram(counts.ctypes.data, int(counts.size), float(lo_edge), float(hi_edge), float(p_low), float(p_high),
                                                 C.byref(out)))
    return out


def hits_to_world(world, camera, hits):
    """tbrm_host_hits_to_world: (world positions float64 [..., 3], depths along camera.forward float64 [...]) of HIT_DTYPE records;
    records without a hit give 0, 0, 0 and +inf. Host arithmetic: needs no device."""
    shape = np.shape(hits)
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE).reshape(-1)
    xyz = np.empty((hits.size, 3), dtype=np.float64)
    depth = np.empty(hits.size, dtype=np.float64)
    check(load().tbrm_host_hits_to_world(C.byref(world), C.byref(camera), hits.ctypes.data, hits.size, xyz.ctypes.data, depth.ctypes.data))
    return xyz.reshape(shape + (3,)), depth.reshape(shape)


def hit_voxel(dims, hit):
    """tbrm_host_hit_voxel: the voxel (x, y, z) the label step reads at a hit record (a HIT_DTYPE scalar) of a volume `dims` (x, y, z)"""
    rec = np.array([hit], dtype=HIT_DTYPE)
    d = (C.c_int32 * 3)(*[int(v) for v in dims])
    out = (C.c_int32 * 3)()
    check(load().tbrm_host_hit_voxel(C.byref(d), rec.ctypes.data, C.byref(out)))
    return tuple(out[:])


def make_default_label_colors():
    """The reference's GetColorFromLabelValue as a 256 x RGBA table (include/tbrm_labels.h)."""
    out = np.empty((256, 4), dtype=np.float32)
    check(load().tbrm_make_default_label_colors(out.ctypes.data))
    return out


def host_bake_tf_lut(lut):
    lut = np.ascontiguousarray(lut, dtype=np.float32).reshape(256, 4)
    out = np.empty_like(lut)
    check(load().tbrm_host_bake_tf_lut(lut.ctypes.data, out.ctypes.data))
    return out


def selftest_unorm_decode(device=0):
    u8, u16 = np.empty(256, dtype=np.float32), np.empty(65536, dtype=np.float32)
    check(load().tbrm_selftest_unorm_decode(device, u8.ctypes.data, u16.ctypes.data))
    return u8, u16


def selftest_unorm8_roundtrip(values, device=0):
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.empty_like(v)
    check(load().tbrm_selftest_unorm8_roundtrip(device, v.ctypes.data, v.size, out.ctypes.data))
    return out


def device_count():
    n = C.c_int(0)
    code = load().tbrm_device_count(C.byref(n))
    return n.value if code == OK else 0


def set_tunable(name, value):
    """Process-wide A/B switch of the library (include/tbrm.h tbrm_set_tunable)."""
    check(load().tbrm_set_tunable(name.encode(), int(value)))


def get_tunable(name):
    v = C.c_int32(0)
    check(load().tbrm_get_tunable(name.encode(), C.byref(v)))
    return v.value


class Resources:
    """Owns one tbrm_resources handle (FBasicRaymarchRenderingResources)."""

    def __init__(self, dims, data_format, light_32bit=False, half_res=False, device=0,
                 data_address_mode=ADDRESS_WRAP, border_mode=BORDER_ENGINE_8BIT, owned=None, rgb=False):
        """owned: a Slab -> a slab-resident handle (tbrm_resources_create_slab) that holds only its part of the volumes;
        rgb: a colour handle (tbrm_resources_create_rgb, include/tbrm_color_lights.h): a light volume of three channels"""
        self.lib = load()
        self.desc = ResourcesDesc(int(dims[0]), int(dims[1]), int(dims[2]), int(data_format), int(bool(light_32bit)),
                                  int(bool(half_res)), int(device), int(data_address_mode), int(border_mode), 0)
        self.handle = C.c_void_p()
        self.owned = owned
        if rgb:
            if owned is not None:
                raise TbrmError(ERR_UNSUPPORTED, "there is no colour form of a slab-resident handle")
            check(self.lib.tbrm_resources_create_rgb(C.byref(self.desc), C.byref(self.handle)))
        elif owned is None:
            check(self.lib.tbrm_resources_create(C.byref(self.desc), C.byref(self.handle)))
        else:
            check(self.lib.tbrm_resources_create_slab(C.byref(self.desc), C.byref(owned), C.byref(self.handle)))
        d = (C.c_int32 * 3)()
        check(self.lib.tbrm_resources_light_volume_dims(self.handle, C.byref(d)))
        self.light_dims = tuple(d[:])
        self.light_dtype = np.float32 if light_32bit else np.uint8
        self.device = int(device)

    def close(self):
        if self.handle:
            self.lib.tbrm_resources_destroy(self.handle)
            self.handle = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # volume arrays are indexed [z, y, x] (x fastest), like the dense UVolumeTexture mip
    def upload_volume(self, vol):
        vol = np.ascontiguousarray(vol)
        assert DTYPE_FMT[vol.dtype] == self.desc.data_format
        assert vol.shape == (self.desc.dim_z, self.desc.dim_y, self.desc.dim_x)
        check(self.lib.tbrm_upload_volume(self.handle, vol.ctypes.data, vol.nbytes))

    def upload_volume_device(self, ptr, nbytes):
        check(self.lib.tbrm_upload_volume_device(self.handle, C.c_void_p(ptr), nbytes))

    def set_tf_lut(self, lut):
        lut = np.ascontiguousarray(lut, dtype=np.float32)
        assert lut.shape == (256, 4)
        check(self.lib.tbrm_set_tf_lut(self.handle, lut.ctypes.data))

    def set_windowing(self, w):
        check(self.lib.tbrm_set_windowing(self.handle, C.byref(w)))

    # label overlay (include/tbrm_labels.h): uint8 [z, y, x] on the data volume's grid
    def upload_label_volume(self, labels):
        labels = np.ascontiguousarray(labels)
        assert labels.dtype == np.uint8 and labels.shape == (self.desc.dim_z, self.desc.dim_y, self.desc.dim_x)
        check(self.lib.tbrm_upload_label_volume(self.handle, labels.ctypes.data, labels.nbytes))

    def update_label_region(self, origin, block):
        """writes `block` (uint8 [ez, ey, ex]) at voxel `origin` (x, y, z) of the attached label volume"""
        block = np.ascontiguousarray(block)
        assert block.dtype == np.uint8 and block.ndim == 3
        o = (C.c_int32 * 3)(*[int(v) for v in origin])
        e = (C.c_int32 * 3)(block.shape[2], block.shape[1], block.shape[0])
        check(self.lib.tbrm_update_label_region(self.handle, C.byref(o), C.byref(e), block.ctypes.data, block.nbytes))

    def download_label_volume(self):
        out = np.empty((self.desc.dim_z, self.desc.dim_y, self.desc.dim_x), dtype=np.uint8)
        check(self.lib.tbrm_download_label_volume(self.handle, out.ctypes.data, out.nbytes))
        return out

    def set_label_colors(self, lut):
        lut = np.ascontiguousarray(lut, dtype=np.float32)
        assert lut.shape == (256, 4)
        check(self.lib.tbrm_set_label_colors(self.handle, lut.ctypes.data))

    def release_label_volume(self):
        check(self.lib.tbrm_release_label_volume(self.handle))

    def has_label_volume(self):
        return bool(self.lib.tbrm_has_label_volume(self.handle))

    # data-volume region updates (include/tbrm_volume_region.h): boxes are [ez, ey, ex] in the handle's data format
    def update_volume_region(self, origin, block):
        """writes `block` ([ez, ey, ex], the volume's dtype) at voxel `origin` (x, y, z) of the uploaded data volume"""
        block = np.ascontiguousarray(block)
        assert DTYPE_FMT[block.dtype] == self.desc.data_format and block.ndim == 3
        o = (C.c_int32 * 3)(*[int(v) for v in origin])
        e = (C.c_int32 * 3)(block.shape[2], block.shape[1], block.shape[0])
        check(self.lib.tbrm_update_volume_region(self.handle, C.byref(o), C.byref(e), block.ctypes.data, block.nbytes))

    def update_volume_region_device(self, origin, extent, ptr, nbytes):
        """the same from device memory: `extent` (ex, ey, ez) voxels, dense and x fastest, at address `ptr`"""
        o = (C.c_int32 * 3)(*[int(v) for v in origin])
        e = (C.c_int32 * 3)(*[int(v) for v in extent])
        check(self.lib.tbrm_update_volume_region_device(self.handle, C.byref(o), C.byref(e), C.c_void_p(ptr), nbytes))

    def download_volume_region(self, origin, extent):
        """the box `extent` (ex, ey, ez) at voxel `origin` (x, y, z) of the data volume, as an [ez, ey, ex] array"""
        o = (C.c_int32 * 3)(*[int(v) for v in origin])
        e = (C.c_int32 * 3)(*[int(v) for v in extent])
        out = np.empty((int(extent[2]), int(extent[1]), int(extent[0])), dtype=FMT_DTYPE[self.desc.data_format])
        check(self.lib.tbrm_download_volume_region(self.handle, C.byref(o), C.byref(e), out.ctypes.data, out.nbytes))
        return out

    VOLUME_REGION_COUNTERS = ("updates", "voxels_written", "bricks_refreshed", "minmax_rebuilds")

    def volume_region_counters(self):
        out = (C.c_uint64 * 4)()
        check(self.lib.tbrm_volume_region_counters(self.handle, C.byref(out)))
        return {k: int(out[i]) for i, k in enumerate(self.VOLUME_REGION_COUNTERS)}

    def skipping_digest(self):
        """tbrm_volume_skipping_digest (a test hook): (bricks, empty bricks, hash of the value ranges, hash of the distance field)"""
        out = (C.c_uint64 * 4)()
        check(self.lib.tbrm_volume_skipping_digest(self.handle, C.byref(out)))
        return tuple(int(v) for v in out)

    # volume statistics (include/tbrm_volume_stats.h): stored units — codes for the UNORM formats, the float itself for float data
    HISTOGRAM_TALLY = ("below", "above", "nan", "visited")

    def histogram_desc(self, n_bins, lo, hi, origin=None, extent=None, labels=None):
        """origin / extent (x, y, z): a box, both None: the whole volume; labels: the label values that count (None: no mask)"""
        d = HistogramDesc()
        if extent is not None:
            d.origin[:] = [int(v) for v in (origin if origin is not None else (0, 0, 0))]
            d.extent[:] = [int(v) for v in extent]
        d.n_bins, d.lo, d.hi = int(n_bins), float(lo), float(hi)
        if labels is not None:
            d.use_label_mask = 1
            for l in labels:
                d.label_mask[int(l) >> 5] |= 1 << (int(l) & 31)
        return d

    def volume_histogram(self, n_bins, lo, hi, origin=None, extent=None, labels=None):
        """(counts uint64[n_bins], {"below", "above", "nan", "visited"})"""
        d = self.histogram_desc(n_bins, lo, hi, origin, extent, labels)
        counts = np.zeros(max(int(n_bins), 1), dtype=np.uint64)
        tally = (C.c_uint64 * 4)()
        check(self.lib.tbrm_volume_histogram(self.handle, C.byref(d), counts.ctypes.data, C.byref(tally)))
        return counts, {k: int(tally[i]) for i, k in enumerate(self.HISTOGRAM_TALLY)}

    def volume_histogram_device(self, ptr, n_bins, lo, hi, origin=None, extent=None, labels=None):
        """adds the bins and the four tallies to the n_bins + 4 uint32 words at device address `ptr`; returns once enqueued"""
        d = self.histogram_desc(n_bins, lo, hi, origin, extent, labels)
        check(self.lib.tbrm_volume_histogram_device(self.handle, C.byref(d), C.c_void_p(ptr)))

    def label_statistics(self, origin=None, extent=None):
        """a record array of 256 (LABEL_STAT_DTYPE): per label count, nan_count, sum, min, max over the box / the whole volume"""
        out = np.zeros(256, dtype=LABEL_STAT_DTYPE)
        if extent is None:
            check(self.lib.tbrm_label_statistics(self.handle, None, None, out.ctypes.data))
        else:
            o = (C.c_int32 * 3)(*[int(v) for v in (origin if origin is not None else (0, 0, 0))])
            e = (C.c_int32 * 3)(*[int(v) for v in extent])
            check(self.lib.tbrm_label_statistics(self.handle, C.byref(o), C.byref(e), out.ctypes.data))
        return out

    VOLUME_STATS_COUNTERS = ("histograms", "label_statistics", "whole_bricks", "cut_bricks")

    def volume_stats_counters(self):
        out = (C.c_uint64 * 4)()
        check(self.lib.tbrm_volume_stats_counters(self.handle, C.byref(out)))
        return {k: int(out[i]) for i, k in enumerate(self.VOLUME_STATS_COUNTERS)}

    # hit maps and picking (include/tbrm_hit.h)
    def raymarch_hits(self, camera, tile, params, world, threshold, scene_depth=None, depth=False):
        """the tile's hit records (HIT_DTYPE [h, w]); depth=True: (records, float32 [h, w] depths along camera.forward, +inf without a
        hit). scene_depth: a float32 framebuffer-sized array the rays stop at (goes through device memory: needs torch)"""
        hits = np.empty((tile.h, tile.w), dtype=HIT_DTYPE)
        dep = np.empty((tile.h, tile.w), dtype=np.float32) if depth else None
        if scene_depth is None:
            check(self.lib.tbrm_raymarch_hits(self.handle, C.byref(camera), C.byref(tile), C.byref(params), C.byref(world), float(threshold),
                                              hits.ctypes.data, dep.ctypes.data if depth else None))
        else:
            import torch
            dev = torch.device("cuda", self.device)
            d_scene = torch.from_numpy(np.ascontiguousarray(scene_depth, dtype=np.float32)).to(dev)
            d_hits = torch.empty(max(hits.nbytes, 1), dtype=torch.uint8, device=dev)
            d_dep = torch.empty(max(hits.size, 1), dtype=torch.float32, device=dev)
            self.raymarch_hits_device(camera, tile, params, world, threshold, d_hits.data_ptr(), d_dep.data_ptr() if depth else None,
                                      d_scene.data_ptr())
            self.flush()
            hits = d_hits.cpu().numpy()[:hits.nbytes].view(HIT_DTYPE).reshape(tile.h, tile.w)
            dep = d_dep.cpu().numpy()[:hits.size].reshape(tile.h, tile.w) if depth else None
        return (hits, dep) if depth else hits

    def raymarch_hits_device(self, camera, tile, params, world, threshold, hits_ptr, depth_ptr=None, scene_depth_ptr=None):
        """enqueues the hit map into device memory: tile.h * tile.w records of 32 bytes at hits_ptr, floats at depth_ptr (or None)"""
        check(self.lib.tbrm_raymarch_hits_device(self.handle, C.byref(camera), C.byref(tile), C.byref(params), C.byref(world), float(threshold),
                                                 C.c_void_p(scene_depth_ptr), C.c_void_p(hits_ptr), C.c_void_p(depth_ptr)))

    def pick(self, camera, px, py, params, world, threshold):
        """tbrm_pick: (the pixel's record as a HIT_DTYPE scalar, world position float64 [3], depth)"""
        hit = np.zeros(1, dtype=HIT_DTYPE)
        xyz, depth = (C.c_double * 3)(), C.c_double()
        check(self.lib.tbrm_pick(self.handle, C.byref(camera), int(px), int(py), C.byref(params), C.byref(world), float(threshold),
                                 hit.ctypes.data, C.byref(xyz), C.byref(depth)))
        return hit[0], np.array(xyz[:], dtype=np.float64), float(depth.value)

    HIT_COUNTERS = ("hit_maps", "picks", "launches")

    def hit_counters(self):
        out = (C.c_uint64 * 3)()
        check(self.lib.tbrm_hit_counters(self.handle, C.byref(out)))
        return {k: int(out[i]) for i, k in enumerate(self.HIT_COUNTERS)}

    # seeded region growing (include/tbrm_segment.h): lo / hi in stored units, seeds and boxes as (x, y, z)
    def grow_desc(self, lo, hi, label, connectivity=6, origin=None, extent=None, writable=None, relative=False):
        """writable: the label values that may be grown over (None: every label); label -1: measure only"""
        d = GROW_DESC()
        if extent is not None:
            d.origin[:] = [int(v) for v in (origin if origin is not None else (0, 0, 0))]
            d.extent[:] = [int(v) for v in extent]
        d.connectivity, d.new_label, d.relative_to_seed = int(connectivity), int(label), int(bool(relative))
        d.lo, d.hi = float(lo), float(hi)
        if writable is None:
            d.writable[:] = [0xFFFFFFFF] * 8
        else:
            for l in writable:
                d.writable[int(l) >> 5] |= 1 << (int(l) & 31)
        return d

    def grow_region(self, seeds, lo, hi, label, connectivity=6, origin=None, extent=None, writable=None, relative=False):
        """tbrm_grow_region from `seeds` ([n, 3] voxels, or empty / None: plain thresholding): {"voxels", "relabelled", "bbox_min",
        "bbox_max", "passes", "seeds_taken", "lo_used", "hi_used"}"""
        d = self.grow_desc(lo, hi, label, connectivity, origin, extent, writable, relative)
        s = np.ascontiguousarray(np.asarray(seeds if seeds is not None else [], dtype=np.int32).reshape(-1, 3))
        out = GROW_RESULT()
        check(self.lib.tbrm_grow_region(self.handle, C.byref(d), s.ctypes.data if len(s) else None, len(s), C.byref(out)))
        return {"voxels": int(out.voxels), "relabelled": int(out.relabelled), "bbox_min": tuple(out.bbox_min[:]), "bbox_max": tuple(out.bbox_max[:]),
                "passes": int(out.passes), "seeds_taken": int(out.seeds_taken), "lo_used": float(out.lo_used), "hi_used": float(out.hi_used)}

    def attach_empty_labels(self):
        check(self.lib.tbrm_attach_empty_label_volume(self.handle))

    SEGMENT_COUNTERS = ("grow_calls", "passes", "brick_visits", "bricks_written")

    def segment_counters(self):
        out = (C.c_uint64 * 4)()
        check(self.lib.tbrm_segment_counters(self.handle, C.byref(out)))
        return {k: int(out[i]) for i, k in enumerate(self.SEGMENT_COUNTERS)}

    # label morphology (include/tbrm_morphology.h): boxes as (x, y, z)
    def morph_desc(self, op, radius, source, new_label, connectivity=6, origin=None, extent=None, writable=None, erase_label=0):
        """op: MORPH_DILATE .. MORPH_CLOSE or its name; source: the label values of the set; writable: the label values a joining voxel
        may overwrite (None: every label); new_label -1: measure only"""
        d = MORPH_DESC()
        if extent is not None:
            d.origin[:] = [int(v) for v in (origin if origin is not None else (0, 0, 0))]
            d.extent[:] = [int(v) for v in extent]
        d.op, d.radius, d.connectivity = int(MORPH_OPS.get(op, op)), int(radius), int(connectivity)
        d.new_label, d.erase_label = int(new_label), int(erase_label)
        for l in source:
            d.source[int(l) >> 5] |= 1 << (int(l) & 31)
        if writable is None:
            d.writable[:] = [0xFFFFFFFF] * 8
        else:
            for l in writable:
                d.writable[int(l) >> 5] |= 1 << (int(l) & 31)
        return d

    def morph_labels(self, op, radius, source, new_label, connectivity=6, origin=None, extent=None, writable=None, erase_label=0):
        """tbrm_morph_labels: {"source_voxels", "result_voxels", "added", "removed", "relabelled", "bbox_min", "bbox_max", "launches"}"""
        d = self.morph_desc(op, radius, source, new_label, connectivity, origin, extent, writable, erase_label)
        out = MORPH_RESULT()
        check(self.lib.tbrm_morph_labels(self.handle, C.byref(d), C.byref(out)))
        return {"source_voxels": int(out.source_voxels), "result_voxels": int(out.result_voxels), "added": int(out.added), "removed": int(out.removed),
                "relabelled": int(out.relabelled), "bbox_min": tuple(out.bbox_min[:]), "bbox_max": tuple(out.bbox_max[:]), "launches": int(out.launches)}

    MORPH_COUNTERS = ("morph_calls", "step_launches", "windows", "bricks_written")

    def morph_counters(self):
        out = (C.c_uint64 * 4)()
        check(self.lib.tbrm_morph_counters(self.handle, C.byref(out)))
        return {k: int(out[i]) for i, k in enumerate(self.MORPH_COUNTERS)}

    # Euclidean margins of labels (include/tbrm_margin.h): boxes, weights and reaches as (x, y, z)
    def margin_desc(self, op, weights, limit, source, new_label, origin=None, extent=None, writable=None, erase_label=0):
        """op: MARGIN_EXPAND .. MARGIN_CLOSE or its name; weights, limit: the squared distance's (margin_weights turns a spacing and a
        radius into them); source, writable, new_label: as in morph_desc"""
        d = MARGIN_DESC()
        if extent is not None:
            d.origin[:] = [int(v) for v in (origin if origin is not None else (0, 0, 0))]
            d.extent[:] = [int(v) for v in extent]
        d.op, d.new_label, d.erase_label = int(MARGIN_OPS.get(op, op)), int(new_label), int(erase_label)
        d.weights[:] = [int(v) for v in weights]
        d.limit = int(limit)
        for l in source:
            d.source[int(l) >> 5] |= 1 << (int(l) & 31)
        if writable is None:
            d.writable[:] = [0xFFFFFFFF] * 8
        else:
            for l in writable:
                d.writable[int(l) >> 5] |= 1 << (int(l) & 31)
        return d

    def margin_labels(self, op, weights, limit, source, new_label, origin=None, extent=None, writable=None, erase_label=0):
        """tbrm_margin_labels: {"source_voxels", "result_voxels", "added", "removed", "relabelled", "bbox_min", "bbox_max", "reach", "launches"}"""
        d = self.margin_desc(op, weights, limit, source, new_label, origin, extent, writable, erase_label)
        out = MARGIN_RESULT()
        check(self.lib.tbrm_margin_labels(self.handle, C.byref(d), C.byref(out)))
        return {"source_voxels": int(out.source_voxels), "result_voxels": int(out.result_voxels), "added": int(out.added), "removed": int(out.removed),
                "relabelled": int(out.relabelled), "bbox_min": tuple(out.bbox_min[:]), "bbox_max": tuple(out.bbox_max[:]), "reach": tuple(out.reach[:]),
                "launches": int(out.launches)}

    def label_distance(self, source, weights, limit, origin=None, extent=None, inside=False):
        """tbrm_label_distance: the weighted squared distance to the source set (inside: to its complement inside the volume) of the
        box's voxels, uint32 [ez, ey, ex]; MARGIN_FAR above `limit`"""
        d = self.margin_desc(MARGIN_EXPAND, weights, limit, source, -1, origin, extent)
        whole = extent is None or tuple(int(v) for v in extent) == (0, 0, 0)
        ex, ey, ez = (self.desc.dim_x, self.desc.dim_y, self.desc.dim_z) if whole else (int(v) for v in extent)
        out = np.empty((max(ez, 0), max(ey, 0), max(ex, 0)), dtype=np.uint32)
        check(self.lib.tbrm_label_distance(self.handle, C.byref(d), int(bool(inside)), out.ctypes.data, out.nbytes))
        return out

    MARGIN_COUNTERS = ("margin_calls", "launches", "bricks_computed", "bricks_written")

    def margin_counters(self):
        out = (C.c_uint64 * 4)()
        check(self.lib.tbrm_margin_counters(self.handle, C.byref(out)))
        return {k: int(out[i]) for i, k in enumerate(self.MARGIN_COUNTERS)}

    # smoothing of labels (include/tbrm_smooth.h): boxes, radii and reaches as (x, y, z)
    def smooth_desc(self, radius, source, new_label, rank=(1, 2), iterations=1, origin=None, extent=None, writable=None, erase_label=0):
        """radius: (r_x, r_y, r_z) in voxels, or one number for all three (smooth_radii turns a spacing and a radius into them);
        rank: (rank_num, rank_den), the median by default; source, writable, new_label: as in morph_desc"""
        d = SMOOTH_DESC()
        if extent is not None:
            d.origin[:] = [int(v) for v in (origin if origin is not None else (0, 0, 0))]
            d.extent[:] = [int(v) for v in extent]
        d.radius[:] = [int(radius)] * 3 if np.isscalar(radius) else [int(v) for v in radius]
        d.rank_num, d.rank_den, d.iterations = int(rank[0]), int(rank[1]), int(iterations)
        d.new_label, d.erase_label = int(new_label), int(erase_label)
        for l in source:
            d.source[int(l) >> 5] |= 1 << (int(l) & 31)
        if writable is None:
            d.writable[:] = [0xFFFFFFFF] * 8
        else:
            for l in writable:
                d.writable[int(l) >> 5] |= 1 << (int(l) & 31)
        return d

    def smooth_labels(self, radius, source, new_label, rank=(1, 2), iterations=1, origin=None, extent=None, writable=None, erase_label=0):
        """tbrm_smooth_labels: {"source_voxels", "result_voxels", "added", "removed", "relabelled", "bbox_min", "bbox_max", "reach", "launches"}"""
        d = self.smooth_desc(radius, source, new_label, rank, iterations, origin, extent, writable, erase_label)
        out = SMOOTH_RESULT()
        check(self.lib.tbrm_smooth_labels(self.handle, C.byref(d), C.byref(out)))
        return {"source_voxels": int(out.source_voxels), "result_voxels": int(out.result_voxels), "added": int(out.added), "removed": int(out.removed),
                "relabelled": int(out.relabelled), "bbox_min": tuple(out.bbox_min[:]), "bbox_max": tuple(out.bbox_max[:]), "reach": tuple(out.reach[:]),
                "launches": int(out.launches)}

    SMOOTH_COUNTERS = ("smooth_calls", "launches", "bricks_computed", "bricks_written")

    def smooth_counters(self):
        out = (C.c_uint64 * 4)()
        check(self.lib.tbrm_smooth_counters(self.handle, C.byref(out)))
        return {k: int(out[i]) for i, k in enumerate(self.SMOOTH_COUNTERS)}

    # view-space scissors (include/tbrm_scissors.h): boxes as (x, y, z)
    def scissors_desc(self, projection, op, source, new_label, origin=None, extent=None, writable=None, erase_label=0):
        """projection: a SCISSORS_PROJECTION (scissors_projection, make_scissors_projection); op: SCISSORS_* or its name;
        source, writable, new_label: as in morph_desc"""
        d = SCISSORS_DESC()
        if extent is not None:
            d.origin[:] = [int(v) for v in (origin if origin is not None else (0, 0, 0))]
            d.extent[:] = [int(v) for v in extent]
        d.op = SCISSORS_OPS[op] if isinstance(op, str) else int(op)
        d.new_label, d.erase_label = int(new_label), int(erase_label)
        for l in source:
            d.source[int(l) >> 5] |= 1 << (int(l) & 31)
        if writable is None:
            d.writable[:] = [0xFFFFFFFF] * 8
        else:
            for l in writable:
                d.writable[int(l) >> 5] |= 1 << (int(l) & 31)
        C.memmove(C.byref(d.projection), C.byref(projection), C.sizeof(SCISSORS_PROJECTION))
        return d

    def scissor_labels(self, projection, mask, op, source, new_label, origin=None, extent=None, writable=None, erase_label=0):
        """tbrm_scissors_labels; mask: uint32 [height, ceil(width / 32)] (scissors_polygon makes one): {"source_voxels", "result_voxels",
        "added", "removed", "relabelled", "bbox_min", "bbox_max", "bricks_inside", "bricks_outside", "bricks_projected", "launches"}"""
        d = self.scissors_desc(projection, op, source, new_label, origin, extent, writable, erase_label)
        m = np.ascontiguousarray(mask, dtype=np.uint32)
        out = SCISSORS_RESULT()
        check(self.lib.tbrm_scissors_labels(self.handle, C.byref(d), m.ctypes.data_as(C.c_void_p), m.size, C.byref(out)))
        return {"source_voxels": int(out.source_voxels), "result_voxels": int(out.result_voxels), "added": int(out.added), "removed": int(out.removed),
                "relabelled": int(out.relabelled), "bbox_min": tuple(out.bbox_min[:]), "bbox_max": tuple(out.bbox_max[:]), "bricks_inside": int(out.bricks_inside),
                "bricks_outside": int(out.bricks_outside), "bricks_projected": int(out.bricks_projected), "launches": int(out.launches)}

    SCISSORS_COUNTERS = ("scissors_calls", "launches", "bricks_projected", "bricks_written")

    def scissors_counters(self):
        out = (C.c_uint64 * 4)()
        check(self.lib.tbrm_scissors_counters(self.handle, C.byref(out)))
        return {k: int(out[i]) for i, k in enumerate(self.SCISSORS_COUNTERS)}

    # competitive growing from seed labels (include/tbrm_compete.h): lo / hi in stored units, boxes as (x, y, z)
    def compete_desc(self, seeds, lo, hi, step_cost=(1, 1, 1), value_shift=0, cost_limit=0, origin=None, extent=None, writable=None, measure_only=False,
                     float_range=None, connectivity=6):
        """seeds: the label values that grow; writable: the label values that may be claimed (None: every label); float_range:
        (float_origin, float_scale) of an R32_FLOAT handle (compete_float_range makes one)"""
        d = COMPETE_DESC()
        if extent is not None:
            d.origin[:] = [int(v) for v in (origin if origin is not None else (0, 0, 0))]
            d.extent[:] = [int(v) for v in extent]
        d.connectivity, d.measure_only, d.value_shift, d.cost_limit = int(connectivity), int(measure_only), int(value_shift), int(cost_limit)
        d.step_cost[:] = [int(v) for v in step_cost]
        d.lo, d.hi = float(lo), float(hi)
        if float_range is not None:
            d.float_origin, d.float_scale = float(float_range[0]), float(float_range[1])
        for l in seeds:
            d.seeds[int(l) >> 5] |= 1 << (int(l) & 31)
        if writable is None:
            d.writable[:] = [0xFFFFFFFF] * 8
        else:
            for l in writable:
                d.writable[int(l) >> 5] |= 1 << (int(l) & 31)
        return d

    def compete_labels(self, seeds, lo, hi, step_cost=(1, 1, 1), value_shift=0, cost_limit=0, origin=None, extent=None, writable=None, measure_only=False,
                       float_range=None, connectivity=6, costs=False):
        """tbrm_compete_labels: {"seed_voxels", "claimable", "claimed", "relabelled", "claimed_per_label" ({label: voxels}, the labels that
        claimed any), "max_cost", "passes", "bbox_min", "bbox_max"}; with costs=True (that, the costs of the box as uint32 [ez, ey, ex])"""
        d = self.compete_desc(seeds, lo, hi, step_cost, value_shift, cost_limit, origin, extent, writable, measure_only, float_range, connectivity)
        box = None
        if costs:
            whole = extent is None or tuple(int(v) for v in extent) == (0, 0, 0)
            e = (self.desc.dim_x, self.desc.dim_y, self.desc.dim_z) if whole else tuple(int(v) for v in extent)
            box = np.empty((max(e[2], 0), max(e[1], 0), max(e[0], 0)), dtype=np.uint32)
        out = COMPETE_RESULT()
        check(self.lib.tbrm_compete_labels(self.handle, C.byref(d), box.ctypes.data_as(C.c_void_p) if box is not None and box.size else None, C.byref(out)))
        res = {"seed_voxels": int(out.seed_voxels), "claimable": int(out.claimable), "claimed": int(out.claimed), "relabelled": int(out.relabelled),
               "claimed_per_label": {l: int(n) for l, n in enumerate(out.claimed_per_label) if n}, "max_cost": int(out.max_cost), "passes": int(out.passes),
               "bbox_min": tuple(out.bbox_min[:]), "bbox_max": tuple(out.bbox_max[:])}
        return (res, box) if costs else res

    COMPETE_COUNTERS = ("compete_calls", "passes", "brick_visits", "bricks_written")

    def compete_counters(self):
        out = (C.c_uint64 * 4)()
        check(self.lib.tbrm_compete_counters(self.handle, C.byref(out)))
        return {k: int(out[i]) for i, k in enumerate(self.COMPETE_COUNTERS)}

    # the 3D paint brush (include/tbrm_paint.h): points in eighths of a voxel, boxes as (x, y, z)
    def paint_desc(self, weights, limit, op, source, new_label, gate=None, origin=None, extent=None, writable=None, erase_label=0):
        """weights, limit: the brush (paint_brush makes them); op: PAINT_* or its name; gate: None or (lo, hi) in stored units;
        source, writable, new_label: as in morph_desc"""
        d = PAINT_DESC()
        if extent is not None:
            d.origin[:] = [int(v) for v in (origin if origin is not None else (0, 0, 0))]
            d.extent[:] = [int(v) for v in extent]
        d.op = PAINT_OPS[op] if isinstance(op, str) else int(op)
        d.new_label, d.erase_label = int(new_label), int(erase_label)
        d.weights[:] = [int(v) for v in weights]
        d.limit = int(limit)
        if gate is not None:
            d.gate, d.lo, d.hi = 1, float(gate[0]), float(gate[1])
        for l in source:
            d.source[int(l) >> 5] |= 1 << (int(l) & 31)
        if writable is None:
            d.writable[:] = [0xFFFFFFFF] * 8
        else:
            for l in writable:
                d.writable[int(l) >> 5] |= 1 << (int(l) & 31)
        return d

    PAINT_FIELDS = ("stamp_voxels", "added", "removed", "relabelled", "segments", "bricks_whole", "bricks_untouched", "bricks_evaluated", "launches")

    def paint_labels(self, points, weights, limit, op, source, new_label, gate=None, origin=None, extent=None, writable=None, erase_label=0):
        """tbrm_paint_labels; points: int32 [n, 3] in eighths of a voxel (paint_stroke makes them from unit-cube positions):
        PAINT_FIELDS, "bbox_min" and "bbox_max" as a dict"""
        d = self.paint_desc(weights, limit, op, source, new_label, gate, origin, extent, writable, erase_label)
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.int32).reshape(-1, 3))
        out = PAINT_RESULT()
        check(self.lib.tbrm_paint_labels(self.handle, C.byref(d), pts.ctypes.data_as(C.c_void_p), pts.shape[0], C.byref(out)))
        res = {k: int(getattr(out, k)) for k in self.PAINT_FIELDS}
        res.update(bbox_min=tuple(out.bbox_min[:]), bbox_max=tuple(out.bbox_max[:]))
        return res

    PAINT_COUNTERS = ("paint_calls", "launches", "bricks_evaluated", "bricks_written")

    def paint_counters(self):
        out = (C.c_uint64 * 4)()
        check(self.lib.tbrm_paint_counters(self.handle, C.byref(out)))
        return {k: int(out[i]) for i, k in enumerate(self.PAINT_COUNTERS)}

    # the surface of a set of labels as an indexed mesh (include/tbrm_surface.h): boxes as (x, y, z)
    def surface_desc(self, source, origin=None, extent=None, triangles=False, measure=False, scale=None, offset=None, vertex_capacity=0, quad_capacity=0):
        """source: the label values of the set; scale, offset: of the positions (None: voxel-index coordinates)"""
        d = SURFACE_DESC()
        if extent is not None:
            d.origin[:] = [int(v) for v in (origin if origin is not None else (0, 0, 0))]
            d.extent[:] = [int(v) for v in extent]
        d.flags = (SURFACE_TRIANGLES if triangles else 0) | (SURFACE_MEASURE if measure else 0)
        d.vertex_capacity, d.quad_capacity = int(vertex_capacity), int(quad_capacity)
        d.scale[:] = [float(v) for v in (scale if scale is not None else (1.0, 1.0, 1.0))]
        d.offset[:] = [float(v) for v in (offset if offset is not None else (0.0, 0.0, 0.0))]
        for l in source:
            d.source[int(l) >> 5] |= 1 << (int(l) & 31)
        return d

    SURFACE_FIELDS = ("set_voxels", "vertices", "quads", "blocks_evaluated", "blocks_skipped", "launches", "written")

    @classmethod
    def surface_result(cls, out):
        res = {k: int(getattr(out, k)) for k in cls.SURFACE_FIELDS}
        res.update(quads_axis=tuple(int(v) for v in out.quads_axis), cell_min=tuple(out.cell_min[:]), cell_max=tuple(out.cell_max[:]))
        return res

    def measure_label_surface(self, source, origin=None, extent=None):
        """tbrm_label_surface with TBRM_SURFACE_MEASURE: the result fields, nothing written"""
        d = self.surface_desc(source, origin, extent, measure=True)
        out = SURFACE_RESULT()
        check(self.lib.tbrm_label_surface(self.handle, C.byref(d), None, None, None, C.byref(out)))
        return self.surface_result(out)

    def label_surface(self, source, origin=None, extent=None, triangles=False, positions=True, scale=None, offset=None):
        """measures, allocates, extracts: the result fields and "vertex" (SURFACE_VERTEX_DTYPE [n]), "indices" (uint32 [quads, 4 or 6]),
        "positions" (float32 [n, 3], or None) as numpy arrays"""
        n = self.measure_label_surface(source, origin, extent)
        d = self.surface_desc(source, origin, extent, triangles, False, scale, offset, n["vertices"], n["quads"])
        vertex = np.zeros(n["vertices"], dtype=SURFACE_VERTEX_DTYPE)
        indices = np.zeros((n["quads"], 6 if triangles else 4), dtype=np.uint32)
        pos = np.zeros((n["vertices"], 3), dtype=np.float32) if positions else None
        out = SURFACE_RESULT()
        check(self.lib.tbrm_label_surface(self.handle, C.byref(d), vertex.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p),
                                          pos.ctypes.data_as(C.c_void_p) if positions else None, C.byref(out)))
        res = self.surface_result(out)
        res.update(vertex=vertex, indices=indices, positions=pos)
        return res

    def label_surface_device(self, source, vertices, indices, positions=None, origin=None, extent=None, triangles=False, scale=None, offset=None):
        """tbrm_label_surface_device onto the caller's torch tensors on the handle's device: vertices (uint8 [capacity, 20] or int32
        [capacity, 5]), indices (int32 / uint32-sized [capacity, 4 or 6]), positions (float32 [capacity, 3]) or None; the capacities
        are the tensors' first dimensions. Returns the result fields"""
        per = 6 if triangles else 4
        assert vertices.is_contiguous() and indices.is_contiguous() and vertices.element_size() * vertices[0].numel() == 20 and indices.element_size() * indices[0].numel() == 4 * per
        assert positions is None or (positions.is_contiguous() and positions.shape[0] >= vertices.shape[0] and positions.element_size() * positions[0].numel() == 12)
        d = self.surface_desc(source, origin, extent, triangles, False, scale, offset, vertices.shape[0], indices.shape[0])
        out = SURFACE_RESULT()
        check(self.lib.tbrm_label_surface_device(self.handle, C.byref(d), vertices.data_ptr(), indices.data_ptr(), positions.data_ptr() if positions is not None else None,
                                                 C.byref(out)))
        return self.surface_result(out)

    SURFACE_COUNTERS = ("surface_calls", "vertices_written", "quads_written", "blocks_evaluated", "scratch_bytes", "scratch_allocations")

    def surface_counters(self):
        out = (C.c_uint64 * 6)()
        check(self.lib.tbrm_surface_counters(self.handle, C.byref(out)))
        return {k: int(out[i]) for i, k in enumerate(self.SURFACE_COUNTERS)}

    # the islands of a label (include/tbrm_islands.h): boxes and first voxels as (x, y, z)
    def islands_desc(self, source, connectivity=6, max_islands=0, min_voxels=0, keep_label=-1, label_step=0, drop_label=-1, spare_border=False,
                     measure=False, origin=None, extent=None):
        """source: the label values of the set, or a ready 8-word mask (a tuple of 8 ints)"""
        d = ISLANDS_DESC()
        if extent is not None:
            d.origin[:] = [int(v) for v in (origin if origin is not None else (0, 0, 0))]
            d.extent[:] = [int(v) for v in extent]
        d.connectivity, d.max_islands, d.min_voxels = int(connectivity), int(max_islands), int(min_voxels)
        d.keep_label, d.label_step, d.drop_label = int(keep_label), int(label_step), int(drop_label)
        d.spare_border, d.flags = int(spare_border), ISLANDS_MEASURE if measure else 0
        for l in source:
            d.source[int(l) >> 5] |= 1 << (int(l) & 31)
        return d

    ISLANDS_FIELDS = ("set_voxels", "islands", "spared", "kept", "dropped", "kept_voxels", "dropped_voxels", "largest", "relabelled")

    def label_islands(self, source, connectivity=6, max_islands=0, min_voxels=0, keep_label=-1, label_step=0, drop_label=-1, spare_border=False,
                      measure=False, origin=None, extent=None, table=0):
        """tbrm_label_islands: the result's fields, "bbox_min", "bbox_max", "table_entries" and "table": the first `table` islands of the
        order as dicts {"voxels", "first", "label", "kept", "border"}"""
        d = self.islands_desc(source, connectivity, max_islands, min_voxels, keep_label, label_step, drop_label, spare_border, measure, origin, extent)
        out = ISLANDS_RESULT()
        entries = (ISLAND * int(table))() if table > 0 else None
        check(self.lib.tbrm_label_islands(self.handle, C.byref(d), entries, int(table), C.byref(out)))
        res = {k: int(getattr(out, k)) for k in self.ISLANDS_FIELDS}
        res.update(bbox_min=tuple(out.bbox_min[:]), bbox_max=tuple(out.bbox_max[:]), table_entries=int(out.table_entries))
        res["table"] = [{"voxels": int(e.voxels), "first": tuple(e.first[:]), "label": int(e.label), "kept": bool(e.flags & ISLAND_KEPT),
                         "border": bool(e.flags & ISLAND_BORDER)} for e in (entries[:out.table_entries] if entries is not None else [])]
        return res

    # the four tools: parameter sets of the one rule
    def keep_largest_islands(self, label, n=1, erase_label=0, connectivity=6, **kw):
        """the n largest islands of `label` stay, the others get erase_label"""
        return self.label_islands([label], connectivity, max_islands=n, keep_label=-1, drop_label=erase_label, **kw)

    def remove_small_islands(self, label, min_voxels, erase_label=0, connectivity=6, **kw):
        """islands of `label` with fewer than min_voxels voxels get erase_label"""
        return self.label_islands([label], connectivity, max_islands=0, min_voxels=min_voxels, keep_label=-1, drop_label=erase_label, **kw)

    def split_islands(self, label, first_label, max_islands, drop_label=-1, connectivity=6, **kw):
        """the max_islands largest islands of `label` get first_label, first_label + 1, ..; the others drop_label (-1: they stay)"""
        return self.label_islands([label], connectivity, max_islands=max_islands, keep_label=first_label, label_step=1, drop_label=drop_label, **kw)

    def fill_label_holes(self, label, max_voxels=None, connectivity=6, **kw):
        """the islands of everything but `label` that touch no face of the box and have at most max_voxels voxels (None: any size)
        get `label`; connectivity is the background's"""
        others = [l for l in range(256) if l != label]
        return self.label_islands(others, connectivity, max_islands=0, min_voxels=ISLANDS_ANY_SIZE if max_voxels is None else int(max_voxels) + 1,
                                  keep_label=-1, drop_label=label, spare_border=True, **kw)

    ISLANDS_COUNTERS = ("islands_calls", "islands_found", "bricks_written", "local_components", "scratch_bytes", "scratch_allocations")

    def islands_counters(self):
        out = (C.c_uint64 * 6)()
        check(self.lib.tbrm_islands_counters(self.handle, C.byref(out)))
        return {k: int(out[i]) for i, k in enumerate(self.ISLANDS_COUNTERS)}

    def is_initialized(self):
        return bool(self.lib.tbrm_resources_is_initialized(self.handle))

    def reserve(self, n_lights, flags=0):
        """tbrm_resources_reserve: allocate now what the light operators of a scene with n_lights lights will need."""
        check(self.lib.tbrm_resources_reserve(self.handle, int(n_lights), int(flags)))

    def add_dir_light(self, light, added, world, gpu_sync=False):
        flag = C.c_int(0)
        check(self.lib.tbrm_add_dir_light(self.handle, C.byref(light), int(bool(added)), C.byref(world), C.byref(flag), int(gpu_sync)))
        return bool(flag.value)

    def add_dir_lights(self, lights, added, world):
        """Several AddDirLight calls as one (passes of different lights that share a cube face run two at a time). Returns
        the order the passes ran in: [(light a, pass a, light b, pass b)], b = (-1, -1) for an unpaired pass."""
        n = len(lights)
        arr = (DirLightParams * max(n, 1))(*lights)
        sched = (C.c_int32 * (8 * max(n, 1)))()
        n_entries = C.c_int32(0)
        check(self.lib.tbrm_add_dir_lights(self.handle, arr, n, int(bool(added)), C.byref(world), sched, C.byref(n_entries)))
        return [tuple(sched[4 * e:4 * e + 4]) for e in range(n_entries.value)]

    def change_dir_light(self, old, new, world, gpu_sync=False):
        flag = C.c_int(0)
        check(self.lib.tbrm_change_dir_light(self.handle, C.byref(old), C.byref(new), C.byref(world), C.byref(flag), int(gpu_sync)))
        return bool(flag.value)

    # coloured lights (include/tbrm_color_lights.h)
    def light_channels(self):
        return int(self.lib.tbrm_resources_light_channels(self.handle))

    def add_color_dir_light(self, light, added, world):
        flag = C.c_int(0)
        check(self.lib.tbrm_add_color_dir_light(self.handle, C.byref(light), int(bool(added)), C.byref(world), C.byref(flag)))
        return bool(flag.value)

    def change_color_dir_light(self, old, new, world):
        flag = C.c_int(0)
        check(self.lib.tbrm_change_color_dir_light(self.handle, C.byref(old), C.byref(new), C.byref(world), C.byref(flag)))
        return bool(flag.value)

    def download_light_channel(self, channel):
        out = np.empty(self.light_dims[::-1], dtype=self.light_dtype)
        check(self.lib.tbrm_download_light_channel(self.handle, int(channel), out.ctypes.data, out.nbytes))
        return out

    def upload_light_channel(self, channel, lv):
        lv = np.ascontiguousarray(lv, dtype=self.light_dtype)
        assert lv.shape == self.light_dims[::-1]
        check(self.lib.tbrm_upload_light_channel(self.handle, int(channel), lv.ctypes.data, lv.nbytes))

    def clear_light_volume(self, value=0.0):
        check(self.lib.tbrm_clear_light_volume(self.handle, float(value)))

    # slab-resident handles
    def resident_slices(self):
        """({first, end, wrap copy's first or -1} of the data volume, the same of the light volume), in slices"""
        d, l = (C.c_int32 * 3)(), (C.c_int32 * 3)()
        check(self.lib.tbrm_slab_resident_slices(self.handle, C.byref(d), C.byref(l)))
        return tuple(d[:]), tuple(l[:])

    def upload_volume_slices(self, z_begin, slices):
        slices = np.ascontiguousarray(slices)
        assert DTYPE_FMT[slices.dtype] == self.desc.data_format and slices.shape[1:] == (self.desc.dim_y, self.desc.dim_x)
        check(self.lib.tbrm_upload_volume_slices(self.handle, int(z_begin), int(slices.shape[0]), slices.ctypes.data, slices.nbytes))

    def upload_resident_part(self, vol):
        """uploads, from the whole volume `vol` [z, y, x], the layers this slab-resident handle holds"""
        (lo, hi, wrap), _ = self.resident_slices()
        self.upload_volume_slices(lo, vol[lo:hi])
        if wrap >= 0:
            self.upload_volume_slices(wrap, vol[wrap:wrap + 8])

    def download_light_slices(self, z_begin, z_count):
        out = np.empty((int(z_count), self.light_dims[1], self.light_dims[0]), dtype=self.light_dtype)
        check(self.lib.tbrm_download_light_slices(self.handle, int(z_begin), int(z_count), out.ctypes.data, out.nbytes))
        return out

    def slab_light_halo(self, side):
        """(device address of the layer to send, of the layer to receive into or None, bytes) for the neighbour on `side`"""
        snd, rcv, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        check(self.lib.tbrm_slab_light_halo(self.handle, int(side), C.byref(snd), C.byref(rcv), C.byref(n)))
        return snd.value, rcv.value, n.value

    # slab-partitioned illumination (tbrm.h "slabs"; driver: slabs.py)
    def slab_light_begin(self, removed, light, added, world, slab):
        n = C.c_int32(0)
        check(self.lib.tbrm_slab_light_begin(self.handle, C.byref(removed) if removed is not None else None, C.byref(light),
                                             int(bool(added)), C.byref(world), C.byref(slab), C.byref(n)))
        return int(n.value)

    def slab_pass_begin(self, index):
        out = SlabPass()
        check(self.lib.tbrm_slab_pass_begin(self.handle, int(index), C.byref(out)))
        return out

    def slab_pass_chunk(self, chunk):
        check(self.lib.tbrm_slab_pass_chunk(self.handle, int(chunk)))

    def slab_pass_plane(self, boundary, stream):
        p = C.c_void_p()
        check(self.lib.tbrm_slab_pass_plane(self.handle, int(boundary), int(stream), C.byref(p)))
        return p.value

    def raymarch_lit(self, camera, tile, params, world):
        out = np.empty((tile.h, tile.w, 4), dtype=np.float32)
        check(self.lib.tbrm_raymarch_lit(self.handle, C.byref(camera), C.byref(tile), C.byref(params), C.byref(world), out.ctypes.data))
        return out

    def raymarch_lit_device(self, camera, tile, params, world, out_ptr, depth_ptr=None):
        check(self.lib.tbrm_raymarch_lit_device(self.handle, C.byref(camera), C.byref(tile), C.byref(params), C.byref(world),
                                                C.c_void_p(depth_ptr), C.c_void_p(out_ptr)))

    def raymarch_lit_slab_device(self, camera, tile, params, world, state_ptr, slab, direction, depth_ptr=None):
        """one stage of a frame marched slab by slab: accumulates this slab's samples into the state (tile.h x tile.w x 4 floats)"""
        check(self.lib.tbrm_raymarch_lit_slab_device(self.handle, C.byref(camera), C.byref(tile), C.byref(params), C.byref(world),
                                                     depth_ptr, state_ptr, C.byref(slab), int(direction)))

    def raymarch_intensity(self, camera, tile, params, world):
        out = np.empty((tile.h, tile.w, 4), dtype=np.float32)
        check(self.lib.tbrm_raymarch_intensity(self.handle, C.byref(camera), C.byref(tile), C.byref(params), C.byref(world), out.ctypes.data))
        return out

    def raymarch_intensity_device(self, camera, tile, params, world, out_ptr, depth_ptr=None):
        check(self.lib.tbrm_raymarch_intensity_device(self.handle, C.byref(camera), C.byref(tile), C.byref(params), C.byref(world),
                                                      C.c_void_p(depth_ptr), C.c_void_p(out_ptr)))

    def generate_octree(self):
        check(self.lib.tbrm_generate_octree(self.handle))

    def octree_mip_dims(self, mip):
        d = (C.c_int32 * 3)()
        check(self.lib.tbrm_octree_mip_dims(self.handle, int(mip), C.byref(d)))
        return tuple(d[:])

    def download_octree_mip(self, mip):
        d = self.octree_mip_dims(mip)
        out = np.empty(d[::-1], dtype=np.uint16)
        check(self.lib.tbrm_download_octree_mip(self.handle, int(mip), out.ctypes.data, out.nbytes))
        return out

    def raymarch_octree(self, camera, tile, params, world, octree_mip):
        out = np.empty((tile.h, tile.w, 4), dtype=np.float32)
        check(self.lib.tbrm_raymarch_octree(self.handle, C.byref(camera), C.byref(tile), C.byref(params), C.byref(world), int(octree_mip), out.ctypes.data))
        return out

    def count_nominal_samples(self, camera, tile, params, world):
        n = C.c_uint64(0)
        check(self.lib.tbrm_count_nominal_samples(self.handle, C.byref(camera), C.byref(tile), C.byref(params), C.byref(world), C.byref(n)))
        return int(n.value)

    def download_light_volume(self):
        out = np.empty(self.light_dims[::-1], dtype=self.light_dtype)
        check(self.lib.tbrm_download_light_volume(self.handle, out.ctypes.data, out.nbytes))
        return out

    def upload_light_volume(self, lv):
        lv = np.ascontiguousarray(lv, dtype=self.light_dtype)
        assert lv.shape == self.light_dims[::-1]
        check(self.lib.tbrm_upload_light_volume(self.handle, lv.ctypes.data, lv.nbytes))

    def light_volume_device_ptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        check(self.lib.tbrm_light_volume_device_ptr(self.handle, C.byref(p), C.byref(n)))
        return p.value, n.value

    def launch_counters(self):
        out = (C.c_uint64 * 3)()
        check(self.lib.tbrm_launch_counters(self.handle, C.byref(out)))
        sweeps = C.c_uint64(0)
        check(self.lib.tbrm_sweep_launches(self.handle, C.byref(sweeps)))
        return {"chunk": int(out[0]), "slice": int(out[1]), "raymarch": int(out[2]), "sweep": int(sweeps.value)}

    PATH_COUNTERS = ("passes_sweep", "passes_chain", "passes_slice", "launches_sweep", "launches_chain", "launches_slice",
                     "occlusion_single", "occlusion_dual", "occlusion_cached", "raymarch", "pair_sweeps", "block_lists_built",
                     "operator_alloc_calls", "operator_host_syncs", "launches_sweep_chain", "occlusion_units_in_runs")

    def path_counters(self):
        """tbrm_path_counters: which kernels the light operators took (per axis pass and per launch)."""
        out = (C.c_uint64 * 16)()
        check(self.lib.tbrm_path_counters(self.handle, C.byref(out)))
        return {k: int(out[i]) for i, k in enumerate(self.PATH_COUNTERS)}

    def light_cache_stats(self):
        out = (C.c_uint64 * 4)()
        check(self.lib.tbrm_light_cache_stats(self.handle, C.byref(out)))
        return {"hits": int(out[0]), "propagated": int(out[1]), "entries": int(out[2]), "bytes": int(out[3])}

    VIEW_CACHE_STATS = ("plain", "counted", "filled", "relit", "dropped", "record_bytes")

    def view_cache_stats(self):
        """tbrm_view_cache_stats (include/tbrm_view_cache.h): how this handle's lit frames were served."""
        out = (C.c_uint64 * 6)()
        check(self.lib.tbrm_view_cache_stats(self.handle, C.byref(out)))
        return {k: int(out[i]) for i, k in enumerate(self.VIEW_CACHE_STATS)}

    def light_cache_clear(self):
        check(self.lib.tbrm_light_cache_clear(self.handle))

    def flush(self):
        check(self.lib.tbrm_flush(self.handle))

    def stream(self):
        s = C.c_void_p()
        check(self.lib.tbrm_stream(self.handle, C.byref(s)))
        return s.value

    def last_gpu_time_ms(self, kind):
        ms = C.c_float(0)
        check(self.lib.tbrm_last_gpu_time_ms(self.handle, int(kind), C.byref(ms)))
        return float(ms.value)
