// tbrm_api_volume_region.cpp — region updates of the data volume (include/tbrm_volume_region.h): a dense sub-box scattered into
// the bricked volume (k_volume_region), read back by the same kernel, and the skipping metadata kept up to date incrementally.
//
// What a box invalidates: data_gen moves on, so the factor cache serves nothing computed from the old voxels (FactorKey), exactly
// as after tbrm_upload_volume; the octree is invalid. The per-brick value ranges (d_minmax) stay valid where no box reaches:
// the box joins tbrm_resources::dirty_boxes and ensure_skipping recomputes, with k_brick_minmax's own body, the bricks it
// reaches (box_reach below states the rule) before it rebuilds the emptiness bits, the shell flag and the distance field as a
// whole — they read the ranges only, 2.6 MiB at 512^3 — and bumps empty_gen, which the block lists and the label field follow.
#include "tbrm_resources.h"
#include "../../include/tbrm_volume_region.h"

#include <vector>

using namespace tbrm;
using namespace tbrm_host;

namespace {

// What every region call checks before it touches the device, in this order: the pointers, the box's signs (they need no handle),
// the handle and what it holds, the box against the volume, the byte count.
int region_args(const tbrm_resources* r, const int32_t origin[3], const int32_t extent[3], const void* voxels, size_t n_bytes, size_t* n_voxels)
{
    if (!origin || !extent || !voxels) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    BoxVerdict v = box_resolve(nullptr, origin, extent, false, nullptr, nullptr); // (what no volume can hold)
    if (v.what != BOX_OK) return fail_box(v, false, nullptr, origin, extent);
    if (!r) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (r->resident) return fail(TBRM_ERR_UNSUPPORTED, "slab-resident handle: its layers are uploaded with tbrm_upload_volume_slices");
    if (!r->has_volume) return fail(TBRM_ERR_NOT_INITIALIZED, "no volume: upload one with tbrm_upload_volume");
    const tbrm_resources::Dims dims = r->data_dims();
    v = box_resolve(dims, origin, extent, false, nullptr, nullptr);
    if (v.what != BOX_OK) return fail_box(v, false, dims, origin, extent);
    const size_t n = (size_t) extent[0] * (size_t) extent[1] * (size_t) extent[2];
    const size_t want = n * format_bytes(r->desc.data_format);
    if (n_bytes != want) return fail(TBRM_ERR_INVALID_ARG, "region is %zu bytes, expected %zu", n_bytes, want);
    *n_voxels = n;
    return TBRM_OK;
}

VolumeRegionParams region_params(const tbrm_resources* r, const int32_t origin[3], const int32_t extent[3], const void* box, bool to_bricks)
{
    VolumeRegionParams p{};
    p.box = box;
    p.bricked = r->d_data;
    for (int c = 0; c < 3; ++c) { p.origin[c] = origin[c]; p.extent[c] = extent[c]; }
    p.bnx = r->dbn[0];
    p.bnxy = r->dbn[0] * r->dbn[1];
    p.elem_bytes = (int) format_bytes(r->desc.data_format);
    p.to_bricks = to_bricks ? 1 : 0;
    return p;
}

// The bricks whose range a box [o, o + e) can have changed. k_brick_minmax's brick b reads, per axis, those of the texels
// 8b .. 8b + 8 that are <= N and addresses them like the sampler. All of them lie in [0, N) as they are, but one: the axis' last
// brick (8 (nb - 1) < N <= 8 (nb - 1) + 8, ragged or not) reads N itself, which wrap addressing sends to texel 0 and clamp
// addressing to N - 1, a texel that brick reads anyway. So along an axis the box reaches the bricks b with [8b, 8b + 8] meeting
// [o, o + e - 1], i.e. max(0, ceil((o - 8) / 8)) .. floor((o + e - 1) / 8), and under wrap addressing, when it holds texel 0, the
// axis' last brick as well. The three axes are independent (the kernel's tests are per axis): the reach is their product.
BrickReach box_reach(const tbrm_resources* r, const tbrm_resources::DirtyBox& box)
{
    BrickReach q{};
    const bool wrap = r->desc.data_address_mode != TBRM_ADDRESS_CLAMP;
    for (int c = 0; c < 3; ++c) {
        const int o = box.origin[c], e = box.extent[c], nb = r->bn[c];
        q.lo[c] = std::max(0, ceil_div(o - 8, 8));
        q.hi[c] = std::min(nb - 1, floor_div(o + e - 1, 8));
        q.last[c] = nb - 1;
        q.n[c] = q.hi[c] - q.lo[c] + 1;
        if (wrap && o == 0 && q.hi[c] < nb - 1) ++q.n[c];
    }
    return q;
}

uint64_t fnv1a(const void* data, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* p = (const unsigned char*) data;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

} // namespace

namespace tbrm_host {

int refresh_dirty_minmax(tbrm_resources* r, const BrickParams& whole)
{
    const uint64_t nb = (uint64_t) r->bn[0] * r->bn[1] * r->bn[2];
    uint64_t reached = 0;
    for (const tbrm_resources::DirtyBox& b : r->dirty_boxes) {
        const BrickReach q = box_reach(r, b);
        reached += (uint64_t) q.n[0] * q.n[1] * q.n[2];
    }
    if (reached >= nb) { // no cheaper than the whole grid
        r->minmax_valid = false;
        return TBRM_OK;
    }
    for (const tbrm_resources::DirtyBox& b : r->dirty_boxes) HIP_TRY(launch_brick_minmax_region(whole, box_reach(r, b), r->stream));
    r->region_counters[2] += reached;
    return TBRM_OK;
}

} // namespace tbrm_host

extern "C" {

int tbrm_volume_region_abi_version(void) { return TBRM_VOLUME_REGION_ABI_VERSION; }

int tbrm_update_volume_region_device(tbrm_resources* r, const int32_t origin[3], const int32_t extent[3], const void* device_voxels, size_t n_bytes)
{
    size_t n = 0;
    if (int e = region_args(r, origin, extent, device_voxels, n_bytes, &n)) return e;
    if (int e = bind(r)) return e;
    quiesce_occ_stream(r); // (nothing on the second stream may still be reading the volume)
    HIP_TRY(launch_volume_region(region_params(r, origin, extent, device_voxels, true), r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    r->region_written(origin, extent, n);
    return TBRM_OK;
}

int tbrm_update_volume_region(tbrm_resources* r, const int32_t origin[3], const int32_t extent[3], const void* host_voxels, size_t n_bytes)
{
    size_t n = 0;
    if (int e = region_args(r, origin, extent, host_voxels, n_bytes, &n)) return e;
    if (int e = bind(r)) return e;
    quiesce_occ_stream(r);
    DeviceScratch staging; // the box in HBM, scattered into the bricks by the GPU
    if (int e = staging.make(n_bytes)) return e;
    HIP_TRY(hipMemcpyAsync(staging.p, host_voxels, n_bytes, hipMemcpyHostToDevice, r->stream));
    HIP_TRY(launch_volume_region(region_params(r, origin, extent, staging.p, true), r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream)); // the caller may free its buffer on return
    r->region_written(origin, extent, n);
    return TBRM_OK;
}

int tbrm_download_volume_region(tbrm_resources* r, const int32_t origin[3], const int32_t extent[3], void* host_out, size_t n_bytes)
{
    size_t n = 0;
    if (int e = region_args(r, origin, extent, host_out, n_bytes, &n)) return e;
    if (int e = bind(r)) return e;
    DeviceScratch staging;
    if (int e = staging.make(n_bytes)) return e;
    HIP_TRY(launch_volume_region(region_params(r, origin, extent, staging.p, false), r->stream));
    HIP_TRY(hipMemcpyAsync(host_out, staging.p, n_bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return TBRM_OK;
}

int tbrm_volume_region_counters(const tbrm_resources* r, uint64_t out[4]) { return copy_counters(r, &tbrm_resources::region_counters, out); }

int tbrm_volume_skipping_digest(tbrm_resources* r, uint64_t out[4])
{
    if (!r || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (r->resident) return fail(TBRM_ERR_UNSUPPORTED, "slab-resident handle: its metadata covers the resident layers only");
    if (!r->has_volume || !r->has_tf) return fail(TBRM_ERR_NOT_INITIALIZED, "resources have no volume or transfer function");
    if (int e = bind(r)) return e;
    if (int e = ensure_skipping(r)) return e;
    const size_t nb = (size_t) r->bn[0] * r->bn[1] * r->bn[2];
    std::vector<float2> minmax(nb);
    std::vector<uint32_t> empty((nb + 31) / 32);
    std::vector<uint8_t> dist(nb);
    HIP_TRY(hipStreamSynchronize(r->stream));
    HIP_TRY(hipMemcpy(minmax.data(), r->d_minmax, nb * sizeof(float2), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(empty.data(), r->d_empty, empty.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dist.data(), r->d_dist[0], nb, hipMemcpyDeviceToHost));
    if (nb & 31) empty.back() &= (1u << (nb & 31)) - 1u; // (the bits beyond the last brick are padding)
    uint64_t n_empty = 0;
    for (uint32_t w : empty) n_empty += (uint64_t) __builtin_popcount(w);
    out[0] = nb;
    out[1] = n_empty;
    out[2] = fnv1a(minmax.data(), nb * sizeof(float2));
    out[3] = fnv1a(dist.data(), nb);
    return TBRM_OK;
}

} // extern "C"
