// tbrm_api_labels.cpp — the label overlay's C-ABI (include/tbrm_labels.h): a uint8 segmentation volume on the data volume's grid,
// its colour table, and what the lit march needs to take the label step (k_raymarch_lit LABELS) with exact empty-space skipping.
//
// The reference sketches the feature in RaymarchExperimental.usf:138-215 (GetColorFromLabelValue, SampleLabelVolume,
// AccumulateOneRaymarchLabelStep) and never calls it; DESIGN.md "Label overlay" pins the semantics the kernel implements.
//
// Metadata, per label upload / region update / colour change:
//   d_lab_mask  per brick, the set of labels among its voxels (k_label_brick_masks; a region update recomputes the touched bricks)
//   d_lab_live  per brick, "holds a label whose colour alpha is > 0" (k_label_live, which also ORs the bricks' sets into the volume's)
// and, per frame when stale (ensure_label_skipping), the merge with the data volume's emptiness: d_empty_lab, d_dist_lab.
// None of it touches d_empty, d_dist, empty_gen, data_gen or tf_gen: the light operators, their block lists and the factor cache
// never see a label change. The occlusion stream never reads the label volume, so nothing here waits for it.
#include "tbrm_resources.h"
#include "../../include/tbrm_labels.h"

#include <cmath>
#include <cstring>

using namespace tbrm;
using namespace tbrm_host;

namespace {

void default_label_colors(float* out)
{
    for (int i = 0; i < 256; ++i) { // GetColorFromLabelValue (RaymarchExperimental.usf)
        float* c = out + 4 * i;
        c[0] = c[1] = c[2] = 0.0f;
        c[3] = 1.0f; // 3 .. 255: opaque black, so that stray labels show
        if (i == 0) c[3] = 0.0f;
        else if (i == 1) { c[0] = 1.0f; c[3] = 0.5f; }
        else if (i == 2) { c[1] = 1.0f; c[3] = 0.5f; }
    }
}

size_t label_voxels(const tbrm_resources* r) { return (size_t) r->desc.dim_x * r->desc.dim_y * r->desc.dim_z; }
size_t label_bricks(const tbrm_resources* r) { return (size_t) r->dbn[0] * r->dbn[1] * r->dbn[2]; }

// the colour table to the device and the set of labels it shows
int put_colors(tbrm_resources* r, const float* rgba)
{
    if (rgba != r->lab_colors) memcpy(r->lab_colors, rgba, sizeof(r->lab_colors));
    for (int w = 0; w < 8; ++w) r->lab_alive[w] = 0u;
    for (int i = 0; i < 256; ++i)
        if (r->lab_colors[4 * i + 3] > 0.0f) r->lab_alive[i >> 5] |= 1u << (i & 31);
    HIP_TRY(hipMemcpyAsync(r->d_lab_colors, r->lab_colors, sizeof(r->lab_colors), hipMemcpyHostToDevice, r->stream));
    return TBRM_OK;
}

} // namespace

namespace tbrm_host {

// the per-brick live bits and the volume's label set (from the per-brick sets); the merged metadata is stale after it
int refresh_live(tbrm_resources* r)
{
    LabelLiveParams lp{};
    lp.masks = r->d_lab_mask;
    lp.n_bricks = (int) label_bricks(r);
    for (int w = 0; w < 8; ++w) lp.alive[w] = r->lab_alive[w];
    lp.live = r->d_lab_live;
    lp.present = r->d_lab_present;
    HIP_TRY(hipMemsetAsync(r->d_lab_present, 0, 8 * sizeof(uint32_t), r->stream));
    HIP_TRY(launch_label_live(lp, r->stream));
    HIP_TRY(hipMemcpyAsync(r->lab_present, r->d_lab_present, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    r->lab_skip_valid = false;
    return TBRM_OK;
}

int brick_masks(tbrm_resources* r, const int b0[3], const int b1[3])
{
    LabelBrickParams bp{};
    bp.labels = r->d_labels;
    bp.masks = r->d_lab_mask;
    bp.bnx = r->dbn[0];
    bp.bny = r->dbn[1];
    for (int c = 0; c < 3; ++c) { bp.b0[c] = b0[c]; bp.b1[c] = b1[c]; }
    HIP_TRY(launch_label_brick_masks(bp, r->stream));
    return TBRM_OK;
}

int fail_box(const BoxVerdict& v, bool zero_is_whole, const int* dims, const int32_t* origin, const int32_t* extent)
{
    const int c = v.axis;
    char wide[32] = "not looked at yet";
    if (dims) snprintf(wide, sizeof(wide), "%d wide", dims[c]);
    return fail(TBRM_ERR_INVALID_ARG, "%s: [%d, %d + %d) along axis %d of a volume %s", box_refusal_text(v.what, zero_is_whole), origin ? (int) origin[c] : 0,
                origin ? (int) origin[c] : 0, extent ? (int) extent[c] : 0, c, wide);
}

int refuse_resident(const tbrm_resources* r)
{
    if (r->resident) return fail(TBRM_ERR_UNSUPPORTED, "slab-resident handle: it holds only some layers of the volume");
    return TBRM_OK;
}

int begin_label_edit(const tbrm_resources* r, const char* no_labels)
{
    if (!r->has_volume) return fail(TBRM_ERR_NOT_INITIALIZED, "no volume: upload one with tbrm_upload_volume");
    if (no_labels && !r->d_labels) return fail(TBRM_ERR_NOT_INITIALIZED, "%s: tbrm_attach_empty_label_volume or tbrm_upload_label_volume", no_labels);
    return bind(r);
}

int labels_changed(tbrm_resources* r, const int32_t bbox_min[3], const int32_t bbox_max[3])
{
    if (bbox_max[0] < 0) return TBRM_OK;
    int b0[3], b1[3];
    bbox_bricks(bbox_min, bbox_max, b0, b1);
    if (int e = brick_masks(r, b0, b1)) return e;
    return refresh_live(r);
}

int fail_value_range(const tbrm_resources* r, double lo, double hi, bool relative)
{
    const double top = r->desc.data_format == TBRM_FMT_G8 ? 255.0 : 65535.0, least = relative ? -top : 0.0;
    switch (value_range_refusal(lo, hi, r->desc.data_format == TBRM_FMT_R32_FLOAT, least, top)) {
    case RANGE_ORDER: return fail(TBRM_ERR_INVALID_ARG, "range [%g, %g]: needs lo <= hi", lo, hi);
    case RANGE_FLOAT: return fail(TBRM_ERR_INVALID_ARG, "range [%g, %g]: both must be finite as float32", lo, hi);
    case RANGE_CODES: return fail(TBRM_ERR_INVALID_ARG, "range [%g, %g]: needs integral codes with %g <= lo <= hi <= %g", lo, hi, least, top);
    default: return TBRM_OK;
    }
}

int ensure_bytes(tbrm_resources* r, char*& buffer, size_t& have, size_t bytes, const char* what)
{
    if (have >= bytes) return TBRM_OK;
    HIP_TRY(hipStreamSynchronize(r->stream));
    (void) hipFree(buffer);
    buffer = nullptr;
    have = 0;
    if (what) count_alloc(r, 1, what);
    HIP_TRY(hipMalloc((void**) &buffer, bytes));
    have = bytes;
    return TBRM_OK;
}

} // namespace tbrm_host

namespace {

// does some label present in the volume show (colour alpha > 0)?
bool labels_visible(const tbrm_resources* r)
{
    for (int w = 0; w < 8; ++w)
        if (r->lab_present[w] & r->lab_alive[w]) return true;
    return false;
}

// d_empty_lab / d_dist_lab from the current d_empty (ensure_skipping has run) and label occupancy: launches only, no allocation
int ensure_label_skipping(tbrm_resources* r)
{
    if (r->lab_skip_valid && r->lab_empty_gen == r->empty_gen) return TBRM_OK;
    const int mode = r->desc.data_address_mode == TBRM_ADDRESS_CLAMP ? ADDR_CLAMP : ADDR_WRAP;
    LabelMergeParams mp{r->d_empty, r->d_lab_live, r->d_empty_lab, {r->bn[0], r->bn[1], r->bn[2]}};
    HIP_TRY(launch_label_merge(mp, mode, r->stream));
    for (int axis = 0; axis < 3; ++axis) { // the three separable passes of the data volume's field (k_brick_dist)
        DistParams dp{r->d_empty_lab, axis == 0 ? nullptr : r->d_dist_lab[(axis + 1) & 1], r->d_dist_lab[axis & 1],
            {r->bn[0], r->bn[1], r->bn[2]}, axis};
        HIP_TRY(launch_brick_dist(dp, mode, r->stream));
    }
    r->lab_skip_valid = true;
    r->lab_empty_gen = r->empty_gen;
    return TBRM_OK;
}

} // namespace

namespace tbrm_host {

int label_ray_params(tbrm_resources* r, RayParams& p)
{
    if (!r->d_labels || !(labels_visible(r) || tune(TUNE_RAY_LABELS) > 0)) return TBRM_OK; // nothing shows: the kernel without labels
    p.labels = r->d_labels;
    p.lab_colors = r->d_lab_colors;
    if (p.skip_dist) {
        if (int e = ensure_label_skipping(r)) return e;
        p.empty_bits = r->d_empty_lab;
        p.skip_dist = r->d_dist_lab[0];
    }
    return TBRM_OK;
}

void release_labels(tbrm_resources* r)
{
    (void) hipFree(r->d_labels);
    (void) hipFree(r->d_lab_mask);
    (void) hipFree(r->d_lab_present);
    (void) hipFree(r->d_lab_live);
    (void) hipFree(r->d_empty_lab);
    for (uint8_t*& d : r->d_dist_lab) { (void) hipFree(d); d = nullptr; }
    (void) hipFree(r->d_lab_colors);
    r->d_labels = nullptr;
    r->d_lab_mask = r->d_lab_present = r->d_lab_live = r->d_empty_lab = nullptr;
    r->d_lab_colors = nullptr;
    for (int w = 0; w < 8; ++w) r->lab_present[w] = r->lab_alive[w] = 0u;
    r->lab_skip_valid = false;
}

int allocate_labels(tbrm_resources* r)
{
    if (r->d_labels) return TBRM_OK;
    // everything the label step and its skipping metadata use: rendering allocates nothing
    const size_t nb = label_bricks(r), nb_pad = (nb + 255) / 256 * 256;
    hipError_t e = hipMalloc((void**) &r->d_labels, nb * 512);
    if (e == hipSuccess) e = hipMalloc((void**) &r->d_lab_mask, nb * 8 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**) &r->d_lab_present, 8 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**) &r->d_lab_live, nb_pad / 8);
    if (e == hipSuccess) e = hipMalloc((void**) &r->d_empty_lab, nb_pad / 8);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipMalloc((void**) &r->d_dist_lab[k], nb_pad);
    if (e == hipSuccess) e = hipMalloc((void**) &r->d_lab_colors, 256 * sizeof(float4));
    if (e != hipSuccess) {
        release_labels(r);
        return fail(e == hipErrorOutOfMemory ? TBRM_ERR_OUT_OF_MEMORY : TBRM_ERR_NO_DEVICE, "label volume allocation failed: %s", hipGetErrorString(e));
    }
    default_label_colors(r->lab_colors);
    if (int e2 = put_colors(r, r->lab_colors)) { release_labels(r); return e2; }
    return TBRM_OK;
}

} // namespace tbrm_host

extern "C" {

int tbrm_labels_abi_version(void) { return TBRM_LABELS_ABI_VERSION; }

int tbrm_make_default_label_colors(float* out)
{
    if (!out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    default_label_colors(out);
    return TBRM_OK;
}

int tbrm_upload_label_volume(tbrm_resources* r, const uint8_t* host_labels, size_t n_bytes)
{
    if (r && r->resident) return fail(TBRM_ERR_UNSUPPORTED, "slab-resident handle: label volumes are not supported");
    if (int e = refuse_color(r, "tbrm_upload_label_volume")) return e;
    if (!r || !host_labels) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (n_bytes != label_voxels(r)) return fail(TBRM_ERR_INVALID_ARG, "label volume is %zu bytes, expected %zu", n_bytes, label_voxels(r));
    if (int e = bind(r)) return e;
    if (int e = allocate_labels(r)) return e;
    DeviceScratch staging; // linear copy in HBM, re-laid out into bricks by the GPU (k_relayout, 1-byte elements)
    if (int e = staging.make(n_bytes)) return e;
    HIP_TRY(hipMemcpyAsync(staging.p, host_labels, n_bytes, hipMemcpyHostToDevice, r->stream));
    HIP_TRY(launch_relayout(relayout_params(staging.p, r->d_labels, r->data_dims(), r->dbn, 1, true), r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream)); // the caller may free its buffer on return
    const int b0[3] = {0, 0, 0}, b1[3] = {r->dbn[0], r->dbn[1], r->dbn[2]};
    if (int e = brick_masks(r, b0, b1)) return e;
    return refresh_live(r);
}

int tbrm_update_label_region(tbrm_resources* r, const int32_t origin[3], const int32_t extent[3], const uint8_t* host_labels, size_t n_bytes)
{
    if (!r || !origin || !extent || !host_labels) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (!r->d_labels) return fail(TBRM_ERR_NOT_INITIALIZED, "no label volume: upload one with tbrm_upload_label_volume");
    const tbrm_resources::Dims dims = r->data_dims();
    VoxelBox box;
    const BoxVerdict v = box_resolve(dims, origin, extent, false, &box, nullptr);
    if (v.what != BOX_OK) return fail_box(v, false, dims, origin, extent);
    const size_t n = (size_t) extent[0] * (size_t) extent[1] * (size_t) extent[2];
    if (n_bytes != n) return fail(TBRM_ERR_INVALID_ARG, "region is %zu bytes, expected %zu", n_bytes, n);
    if (int e = bind(r)) return e;
    DeviceScratch staging;
    if (int e = staging.make(n_bytes)) return e;
    LabelRegionParams rp{};
    rp.src = (const uint8_t*) staging.p;
    rp.dst = r->d_labels;
    for (int c = 0; c < 3; ++c) { rp.origin[c] = origin[c]; rp.extent[c] = extent[c]; }
    rp.bnx = r->dbn[0];
    rp.bnxy = r->dbn[0] * r->dbn[1];
    HIP_TRY(hipMemcpyAsync(staging.p, host_labels, n_bytes, hipMemcpyHostToDevice, r->stream));
    HIP_TRY(launch_label_region(rp, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    const int32_t last[3] = {box.end[0] - 1, box.end[1] - 1, box.end[2] - 1};
    return labels_changed(r, box.origin, last);
}

int tbrm_download_label_volume(tbrm_resources* r, uint8_t* host_out, size_t n_bytes)
{
    if (!r || !host_out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (!r->d_labels) return fail(TBRM_ERR_NOT_INITIALIZED, "no label volume");
    if (n_bytes != label_voxels(r)) return fail(TBRM_ERR_INVALID_ARG, "label volume is %zu bytes, got %zu", label_voxels(r), n_bytes);
    if (int e = bind(r)) return e;
    DeviceScratch staging;
    if (int e = staging.make(n_bytes)) return e;
    HIP_TRY(launch_relayout(relayout_params(r->d_labels, staging.p, r->data_dims(), r->dbn, 1, false), r->stream));
    HIP_TRY(hipMemcpyAsync(host_out, staging.p, n_bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return TBRM_OK;
}

int tbrm_set_label_colors(tbrm_resources* r, const float* rgba_256x4)
{
    if (!r || !rgba_256x4) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < 1024; ++i) {
        const float v = rgba_256x4[i];
        if (!std::isfinite(v) || v < 0.0f || v > 1.0f)
            return fail(TBRM_ERR_INVALID_ARG, "label colour %d component %d is %g: components must be finite and in [0, 1]", i / 4, i % 4, (double) v);
    }
    if (!r->d_labels) return fail(TBRM_ERR_NOT_INITIALIZED, "no label volume: upload one with tbrm_upload_label_volume");
    if (int e = bind(r)) return e;
    HIP_TRY(hipStreamSynchronize(r->stream)); // (a frame in flight may still read the table)
    if (int e = put_colors(r, rgba_256x4)) return e;
    return refresh_live(r);
}

int tbrm_release_label_volume(tbrm_resources* r)
{
    if (!r) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (!r->d_labels) return TBRM_OK;
    if (int e = bind(r)) return e;
    HIP_TRY(hipStreamSynchronize(r->stream));
    release_labels(r);
    return TBRM_OK;
}

int tbrm_has_label_volume(const tbrm_resources* r)
{
    if (!r) {
        (void) fail(TBRM_ERR_INVALID_ARG, "null argument");
        return 0;
    }
    return r->d_labels ? 1 : 0;
}

} // extern "C"
