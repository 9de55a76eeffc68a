/* tbrm_view_cache.h — observability of the view cache (C-ABI, libtbrm.so).
 *
 * A lit frame (tbrm_raymarch_lit / tbrm_raymarch_lit_device) whose view is unchanged since the frames before it — camera, tile,
 * step count, jitter, volume, window, transfer function, clip plane, volume transform; everything but the light volume's
 * contents — is relit from records of the march instead of being marched again: of a sample only its light taps and the
 * accumulation depend on the light. The frames of one view go: marched plainly, marched and counted, marched and recorded,
 * then relit; any change of the view starts over with the plain march, so a host whose camera moves every frame runs the march
 * it always ran. Relit frames are bit-identical to marched ones. One view per handle. Frames with a scene depth, colour
 * handles, handles with a label volume, slab stages and slab-resident handles always march.
 *
 * The records live in one allocation PER HANDLE of at most `view_cache_mb` MiB (tunable, TBRM_VIEW_CACHE_MB; default 1536, 0 turns
 * the cache off; never more than half — a handle nobody reserved: an eighth — of the device memory free beyond 8 GiB), taken by
 * tbrm_resources_reserve or by the handle's first counting frame and freed with the handle: every reserved mono handle holds it,
 * so a host with many handles sets the tunable to what one view needs (tbrm_view_cache_stats [5]) or to 0. The allocation is made
 * ONCE, sized by the tunable's value at that moment: a later change of `view_cache_mb` (other than to 0, which turns the cache off
 * at once, and back) does not resize it, and a handle whose allocation failed marches every frame and does not try again. A view
 * whose records do not fit is marched until it changes.
 *
 * Restriction. The frame call itself moves the view's state on: the counting frame may allocate, the recording frame enqueues a
 * copy to pinned memory, and later frames ask an event whether it has arrived. Frame calls must therefore not be captured into a
 * HIP graph while the cache is on — a captured call would fail at those steps, and a replayed graph would repeat one state's
 * launch for ever; a host that captures its frames sets `view_cache_mb` to 0. */
#ifndef TBRM_VIEW_CACHE_H
#define TBRM_VIEW_CACHE_H

#include "tbrm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_VIEW_CACHE_ABI_VERSION 1

TBRM_API int tbrm_view_cache_abi_version(void);
/* Cumulative per handle: lit frames of a mono handle [0] marched plainly, [1] marched and counted, [2] marched and recorded,
 * [3] relit; [4] views dropped because their records did not fit; [5] record bytes the current view holds (0 until it is relit). */
TBRM_API int tbrm_view_cache_stats(const tbrm_resources* res, uint64_t out[6]);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_VIEW_CACHE_H */
