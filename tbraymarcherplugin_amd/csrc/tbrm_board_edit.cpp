// tbrm_board_edit.cpp — the frame of the board operators (tbrm_board_edit.h).
#include "tbrm_board_edit.h"

namespace tbrm_host {

int label_codes(int new_label, int erase_label, int reserved)
{
    if (new_label < -1 || new_label > 255) return fail(TBRM_ERR_INVALID_ARG, "new_label %d: must be 0 .. 255, or -1 to measure only", new_label);
    if (erase_label < 0 || erase_label > 255) return fail(TBRM_ERR_INVALID_ARG, "erase_label %d: must be 0 .. 255", erase_label);
    if (reserved != 0) return fail(TBRM_ERR_INVALID_ARG, "reserved = %d: must be 0", reserved);
    return TBRM_OK;
}

int BoardEdit::begin(const tbrm_resources* r, const int32_t* origin, const int32_t* extent, BrickRange* range)
{
    const tbrm_resources::Dims dims = r->data_dims();
    const BoxVerdict v = box_resolve(dims, origin, extent, true, &p.box, range);
    if (v.what != BOX_OK) return fail_box(v, true, dims, origin, extent);
    for (int c = 0; c < 3; ++c) p.dims[c] = dims[c];
    return begin_label_edit(r, "no label volume");
}

int BoardEdit::bind(tbrm_resources* r, const uint32_t source[8], const uint32_t writable[8], int new_label, int erase_label)
{
    if (int e = ensure_grow_scratch(r)) return e;
    const GrowScratch g = grow_scratch(r);
    p.labels = r->d_labels;
    p.bnx = r->dbn[0];
    p.bnxy = r->dbn[0] * r->dbn[1];
    for (int w = 0; w < 8; ++w) { p.source[w] = source[w]; p.writable[w] = writable[w]; }
    p.bits = g.bits;
    p.cls[0] = g.act[0];
    p.cls[1] = g.act[1];
    p.new_label = new_label;
    p.erase_label = erase_label;
    p.ctl = g.ctl;
    return TBRM_OK;
}

int BoardEdit::load(tbrm_resources* r)
{
    ctl_start(ctl, words, MORPH_MIN_X, p.dims);
    HIP_TRY(hipMemcpyAsync(p.ctl, ctl, (size_t) words * sizeof(int32_t), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(launch_morph_load(p, r->stream));
    return TBRM_OK;
}

int BoardEdit::read_ctl(tbrm_resources* r)
{
    HIP_TRY(hipMemcpyAsync(ctl, p.ctl, (size_t) words * sizeof(int32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return TBRM_OK;
}

int BoardEdit::write(tbrm_resources* r, int from)
{
    p.from = from;
    HIP_TRY(launch_morph_write(p, r->stream));
    return read_ctl(r);
}

int BoardEdit::end(tbrm_resources* r, uint64_t counters[4], int launches, bool count_call) const
{
    if (count_call) ++counters[0];
    counters[1] += (uint64_t) launches;
    counters[2] += count(MORPH_WINDOWS);
    counters[3] += count(MORPH_BRICKS_WRITTEN);
    if (p.new_label >= 0) return labels_changed(r, ctl + MORPH_MIN_X, ctl + MORPH_MAX_X); // (nothing joined or left: nothing to do)
    return TBRM_OK;
}

} // namespace tbrm_host
