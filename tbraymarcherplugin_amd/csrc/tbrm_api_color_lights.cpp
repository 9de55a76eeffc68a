// tbrm_api_color_lights.cpp — the C-ABI of coloured directional lights (include/tbrm_color_lights.h): colour handles, the
// coloured Add / Change entry points and the per-channel transfers. The operator rule itself (one mono operator per live channel,
// occlusion once per light) is tbrm_light_operators.cpp's enqueue_color_add / enqueue_color_change; the RGB-light form of the lit
// march is k_raymarch_lit's (tbrm_kernels.hip). What a colour handle refuses is refused where the call lives (refuse_color).
#include "tbrm_resources.h"

#include <cmath>

using namespace tbrm;
using namespace tbrm_host;

namespace {

bool color_ok(const tbrm_color_dir_light& l)
{
    for (float c : l.color)
        if (!std::isfinite(c) || c < 0.0f || c > 1.0f) return false;
    return true;
}

// what every coloured operator checks before it enqueues anything
int color_operator_args(const tbrm_resources* r, const tbrm_color_dir_light* a, const tbrm_color_dir_light* b, const tbrm_world_params* world)
{
    if (!r || !a || !b || !world) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (r->light_channels != 3) return fail(TBRM_ERR_INVALID_ARG, "coloured lights need a colour handle (tbrm_resources_create_rgb)");
    if (!color_ok(*a) || !color_ok(*b)) return fail(TBRM_ERR_INVALID_ARG, "every colour component must be finite and in [0, 1]");
    if (!initialized(r)) return fail(TBRM_ERR_NOT_INITIALIZED, "resources have no volume or transfer function");
    return TBRM_OK;
}

} // namespace

extern "C" {

int tbrm_color_lights_abi_version(void) { return TBRM_COLOR_LIGHTS_ABI_VERSION; }

int tbrm_resources_create_rgb(const tbrm_resources_desc* desc, tbrm_resources** out) { return create_handle(desc, nullptr, 3, out); }

int tbrm_resources_light_channels(const tbrm_resources* r)
{
    if (!r) {
        (void) fail(TBRM_ERR_INVALID_ARG, "null argument");
        return 0;
    }
    return r->light_channels;
}

int tbrm_add_color_dir_light(tbrm_resources* r, const tbrm_color_dir_light* light, int added, const tbrm_world_params* world, int* light_added)
{
    if (light_added) *light_added = 0;
    if (int e = color_operator_args(r, light, light, world)) return e;
    if (light_added) *light_added = 1;
    if (int e = bind(r)) return e;
    if (int e = begin_timed(r, 0)) return e;
    const int e = enqueue_color_add(r, *light, added != 0, *world);
    const int e2 = end_timed(r, 0); // also after a failure: the events then bracket whatever was enqueued
    return e ? e : e2;
}

int tbrm_change_color_dir_light(tbrm_resources* r, const tbrm_color_dir_light* old_light, const tbrm_color_dir_light* new_light,
                                const tbrm_world_params* world, int* light_added)
{
    if (light_added) *light_added = 0;
    if (int e = color_operator_args(r, old_light, new_light, world)) return e;
    if (light_added) *light_added = 1;
    if (int e = bind(r)) return e;
    if (int e = begin_timed(r, 0)) return e;
    const int e = enqueue_color_change(r, *old_light, *new_light, *world);
    const int e2 = end_timed(r, 0);
    return e ? e : e2;
}

int tbrm_download_light_channel(tbrm_resources* r, int channel, void* host_out, size_t n_bytes) { return download_light_channel(r, channel, host_out, n_bytes); }
int tbrm_upload_light_channel(tbrm_resources* r, int channel, const void* host_in, size_t n_bytes) { return upload_light_channel(r, channel, host_in, n_bytes); }

} // extern "C"
