/* tbrm_labels.h — segmentation label-volume overlay of the lit raymarch (C-ABI, libtbrm.so).
 *
 * A label volume is uint8, dense, x fastest, with the data volume's dimensions: up to 256 labels, each mapped to an RGBA colour
 * by a 256-entry float table (every component finite and in [0, 1]; kept as float32, not baked like the transfer function).
 * At every sample the lit march takes (not clipped, inside the depth limit; full steps and the fractional final step), after
 * the data sample's AccumulateWindowedRaymarchStep and before the 0.95 early-exit test, the nearest label voxel
 * L = label[rint((N - 1) * saturate(pos))] (per axis, float32, round half to even) is accumulated unlit:
 *   a' = 1 - pow(1 - colors[L].a, step), LE.rgb += colors[L].rgb * a' * (1 - LE.a), LE.a += a' * (1 - LE.a)
 * with the data sample's world step (the reference's unfinished RaymarchExperimental.usf label functions). Labels take no part
 * in the illumination, the transfer function or the cut-offs. The Intensity and Octree renderers ignore labels; slab-resident
 * handles and the slab stage of the lit march refuse them (TBRM_ERR_UNSUPPORTED).
 *
 * Without a label volume, and with one none of whose present labels has a colour alpha > 0, every entry point behaves bit for bit
 * as without this header. DESIGN.md "Label overlay" has the details. */
#ifndef TBRM_LABELS_H
#define TBRM_LABELS_H

#include "tbrm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_LABELS_ABI_VERSION 1

TBRM_API int tbrm_labels_abi_version(void);
/* The reference's GetColorFromLabelValue: 0 -> (0,0,0,0), 1 -> (1,0,0,0.5), 2 -> (0,1,0,0.5), 3..255 -> (0,0,0,1). */
TBRM_API int tbrm_make_default_label_colors(float* out_rgba_256x4);
/* The whole label volume (n_bytes = dim_x * dim_y * dim_z); the caller's buffer is free on return. The first upload allocates the
 * label volume and its skipping metadata and sets the default colour table. */
TBRM_API int tbrm_upload_label_volume(tbrm_resources* res, const uint8_t* host_labels, size_t n_bytes);
/* A dense x-fastest sub-box [origin, origin + extent) of the attached label volume (edits, brush strokes); n_bytes = the box's voxels. */
TBRM_API int tbrm_update_label_region(tbrm_resources* res, const int32_t origin[3], const int32_t extent[3],
                                      const uint8_t* host_labels, size_t n_bytes);
TBRM_API int tbrm_download_label_volume(tbrm_resources* res, uint8_t* host_out, size_t n_bytes);
/* 256 x RGBA float; every component finite and in [0, 1] (else TBRM_ERR_INVALID_ARG). Needs an attached label volume. */
TBRM_API int tbrm_set_label_colors(tbrm_resources* res, const float* rgba_256x4);
/* Detaches and frees the label volume (a handle without one: no-op). */
TBRM_API int tbrm_release_label_volume(tbrm_resources* res);
/* 1 while a label volume is attached, else 0 (also for a null handle). */
TBRM_API int tbrm_has_label_volume(const tbrm_resources* res);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_LABELS_H */
