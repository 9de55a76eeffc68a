/* tbrm_color_lights.h — coloured directional lights: an RGB illumination volume (C-ABI, libtbrm.so).
 *
 * The reference kept "a single channel illumination volume (not a RGB light volume to accomodate for colored lights)"
 * (Readme.md:165). A colour handle (tbrm_resources_create_rgb) has a light volume of three channels R, G, B, each with the
 * dimensions and format a handle of the same tbrm_resources_desc has; a coloured light is a directional light and a colour.
 *
 * Propagation. Channel c after any sequence of coloured operators is, bit for bit, the light volume of a mono handle that ran the
 * same sequence with every light's intensity replaced by light_intensity * color[c] (one float32 product). A channel whose
 * product is 0 is skipped by an Add and by a Change 0 -> 0 (the shaders write nothing then, AddDirLightShader.usf:123). The
 * occlusion of a light does not depend on its intensity: it is sampled once per light, not once per channel.
 *
 * Frame. AccumulateWindowedRaymarchStep multiplies ColorSample.rgb by the light volume's .rgb, component-wise
 * (WindowedRaymarchMaterials.usf:30 with an RGB volume): frame channel c is the mono frame lit by channel c, alpha is the mono
 * frame's alpha.
 *
 * The mono entry points of tbrm.h act as white on a colour handle: tbrm_add_dir_light / tbrm_change_dir_light as colour (1, 1, 1),
 * tbrm_clear_light_volume on all channels; renderers, uploads, transfer function and windowing as on any handle. Not available on a
 * colour handle (TBRM_ERR_UNSUPPORTED, nothing enqueued): tbrm_add_dir_lights, the tbrm_slab_* calls, tbrm_raymarch_lit_slab_device,
 * tbrm_upload_label_volume, and tbrm_download_light_volume / tbrm_upload_light_volume / tbrm_light_volume_device_ptr, which the
 * per-channel transfers below replace. There is no colour form of tbrm_resources_create_slab. DESIGN.md "Coloured lights". */
#ifndef TBRM_COLOR_LIGHTS_H
#define TBRM_COLOR_LIGHTS_H

#include "tbrm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_COLOR_LIGHTS_ABI_VERSION 1

/* Every colour component finite and in [0, 1] (else TBRM_ERR_INVALID_ARG). */
typedef struct tbrm_color_dir_light {
    tbrm_dir_light_params light;
    float color[3];
    int32_t _pad;
} tbrm_color_dir_light;

TBRM_API int tbrm_color_lights_abi_version(void);
/* tbrm_resources_create with a light volume of three channels. */
TBRM_API int tbrm_resources_create_rgb(const tbrm_resources_desc* desc, tbrm_resources** out);
/* 1 or 3; a null handle: 0, and tbrm_last_error() says so. */
TBRM_API int tbrm_resources_light_channels(const tbrm_resources* res);
/* tbrm_add_dir_light per channel (added = 0: removes the light). A zero direction: as tbrm_add_dir_light. TBRM_ERR_INVALID_ARG on
 * a mono handle. */
TBRM_API int tbrm_add_color_dir_light(tbrm_resources* res, const tbrm_color_dir_light* light, int added, const tbrm_world_params* world,
                                      int* light_added);
/* tbrm_change_dir_light per channel; a change of colour alone is an ordinary Change. TBRM_ERR_INVALID_ARG on a mono handle. */
TBRM_API int tbrm_change_color_dir_light(tbrm_resources* res, const tbrm_color_dir_light* old_light, const tbrm_color_dir_light* new_light,
                                         const tbrm_world_params* world, int* light_added);
/* One channel (0 R, 1 G, 2 B), dense, x fastest, in the format and size of tbrm_download_light_volume / tbrm_upload_light_volume
 * (a mono handle has channel 0 only). An upload defines the channel, as tbrm_upload_light_volume defines the volume. */
TBRM_API int tbrm_download_light_channel(tbrm_resources* res, int channel, void* host_out, size_t n_bytes);
TBRM_API int tbrm_upload_light_channel(tbrm_resources* res, int channel, const void* host_in, size_t n_bytes);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_COLOR_LIGHTS_H */
