// tbrm_board_edit.h — the frame of the board operators (DESIGN.md §17 "The board operators' frame"), stated once: label morphology,
// margins, smoothing, the scissors and the paint brush are the same call with a different middle.
//
//   label_codes                 new_label, erase_label and reserved of a desc
//   BoardEdit::begin            the box against the volume, then the handle (begin_label_edit)
//   BoardEdit::bind             the scratch of region growing, and everything of MorphParams that comes from it, the handle and the desc
//   BoardEdit::load             the control words' start values, the source set into board 0 (k_morph_load)
//   ... the operator's own kernels, board to board ...
//   BoardEdit::write            board `from` against the label bytes (k_morph_write), the control words back, the wait
//   BoardEdit::changes, result  what every result holds, from the control words
//   BoardEdit::end              the four counters, and behind a writing call what every label write ends with (labels_changed)
//
// An operator's file keeps its own argument checks, its plan (p.range, p.wrange), its own kernels' parameters and launches, and the
// result fields that are its own.
#pragma once
#include "tbrm_resources.h"

#include <cstring>

namespace tbrm_host {

// the label codes of a desc, in the order every board operator reports them (a desc without `reserved` passes 0)
int label_codes(int new_label, int erase_label, int reserved);

struct BoardEdit {
    MorphParams p{};
    int32_t ctl[GROW_CTL_WORDS]; // the call's control words on the host: `words` of them
    int words;

    explicit BoardEdit(int ctl_words) : words(ctl_words) {}

    // the box [origin, origin + extent) into p.box (and its bricks into *range), the volume into p.dims; then the handle
    int begin(const tbrm_resources* r, const int32_t* origin, const int32_t* extent, BrickRange* range = nullptr);
    int bind(tbrm_resources* r, const uint32_t source[8], const uint32_t writable[8], int new_label, int erase_label);
    template <class Desc> int bind(tbrm_resources* r, const Desc* d) { return bind(r, d->source, d->writable, d->new_label, d->erase_label); }
    // p.range and p.wrange of a plan that grows the box by a reach (morph_plan, margin_plan, smooth_plan)
    template <class Plan> void ranges(const Plan& plan)
    {
        for (int c = 0; c < 3; ++c) { p.range.b0[c] = plan.b0[c]; p.range.nb[c] = plan.nb[c]; p.wrange.b0[c] = plan.wb0[c]; p.wrange.nb[c] = plan.wnb[c]; }
    }
    int load(tbrm_resources* r);
    int write(tbrm_resources* r, int from);
    int read_ctl(tbrm_resources* r); // the control words back and the wait (write does it; a call without a write ends with it)

    uint64_t count(int i) const // the 64-bit count i of the control words
    {
        uint64_t v;
        memcpy(&v, ctl + 2 * i, sizeof(v));
        return v;
    }
    template <class Result> void changes(Result* out) const
    {
        out->added = count(MORPH_ADDED);
        out->removed = count(MORPH_REMOVED);
        out->relabelled = count(MORPH_RELABELLED);
        for (int c = 0; c < 3; ++c) { out->bbox_min[c] = ctl[MORPH_MIN_X + c]; out->bbox_max[c] = ctl[MORPH_MAX_X + c]; }
    }
    template <class Result> void result(Result* out) const
    {
        out->source_voxels = count(MORPH_SOURCE);
        out->result_voxels = count(MORPH_RESULT);
        changes(out);
    }
    // counters: the operator's four of the handle (count_call false: the caller has counted the call in [0] already)
    int end(tbrm_resources* r, uint64_t counters[4], int launches, bool count_call = true) const;
};

} // namespace tbrm_host
