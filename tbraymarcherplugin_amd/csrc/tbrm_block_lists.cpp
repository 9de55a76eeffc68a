// tbrm_block_lists.cpp — the block lists of the sparse occlusion (tbrm_resources.h BlockLists): which 16 x 16 x 8 blocks of an
// axis pass can see anything but empty bricks, the ascending list of those that can, their ranks, their count.
//
// Until round 5 every light operator rebuilt them (k_occ_flags + k_occ_compact per pass, k_unit_flags + k_occ_compact per dual
// launch: six dependent launches in front of every occlusion kernel, ~0.1 ms of every benchmark step on the occlusion stream).
// What k_occ_flags computes depends on the emptiness bits of the data bricks (volume, transfer function, window) and on the
// pass only through INTEGERS: per block column / row / slice group the range of data texels its samples' base taps fall into
// (texel_split of the block's first and last position + UVWOffset, tbrm_light_kernels.hip k_occ_flags). A light that turns by a
// few degrees keeps those integers — UVWOffset stays within the same texel — so the lists are kept under that signature and a
// pass that finds its signature launches nothing. The signature is evaluated here by the function k_occ_flags itself calls
// (tbrm_occ_footprint.h pass_tap_span: IEEE single operations, -ffp-contract=off on both sides).
#include "tbrm_resources.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace tbrm_host {

using namespace tbrm;

static constexpr size_t kMaxLists = 384;      // per handle (a reserved handle of eight lights starts with 240 spare ones); beyond: the least recently used ones nobody refers to go

// Everything k_occ_flags<NS, AXIS> reads of a one-chunk pass besides ChunkParams::empty_bits, as integers: the geometry and,
// per block column, block row and slice group, the lowest base tap and the highest upper tap over the streams the mode computes.
static void block_lists_signature(const ChunkParams& p, int occ_mode, std::vector<int32_t>& sig)
{
    const OccPassShape s = occ_pass_shape(p, occ_mode_streams(occ_mode), 0);
    sig.clear();
    for (int v : {s.ns, p.axis, p.W, p.H, p.dir, p.pass_start, p.pass_slices, p.chunk_slices, p.occ_groups, p.occ_blocks_x, p.occ_blocks_y, p.roi_by0,
                  p.roi_by1, p.data.nx, p.data.ny, p.data.nz, p.data.bnx, p.data.bnxy, p.lv_dims[0], p.lv_dims[1], p.lv_dims[2]})
        sig.push_back(v);
    pass_tap_spans(s, [&](int lo, int hi) { sig.push_back(lo); sig.push_back(hi); });
}

static void free_lists(BlockLists* l)
{
    if (!l) return;
    (void) hipFree(l->flags);
    (void) hipFree(l->list);
    (void) hipFree(l->slot);
    (void) hipFree(l->count);
    if (l->count_host) (void) hipHostFree(l->count_host);
    if (l->ev_done) (void) hipEventDestroy(l->ev_done);
    delete l;
}

// tbrm_path_counters [15]: a run list's launches each ran (live units - runs) units behind the first of their run — a number
// k_occ_runs leaves in pinned memory (count_host[1]). A list that goes, or is cut anew, hands its share to the handle first.
static void retire_run_list(tbrm_resources* r, BlockLists* l)
{
    if (l->run_launches) r->run_followers += l->run_launches * (uint64_t) std::max(l->count_host[1], 0);
    l->run_launches = 0;
    l->run_len = 0;
}

void release_block_lists(tbrm_resources* r)
{
    for (BlockLists* l : r->block_lists) {
        if (l->run_launches) (void) hipEventSynchronize(l->ev_done); // (tbrm_path_counters [15] counts since creation: the share of a list that goes stays)
        retire_run_list(r, l);
        free_lists(l);
    }
    r->block_lists.clear();
    for (BlockLists* l : r->spare_lists) free_lists(l);
    r->spare_lists.clear();
}

// (never waits: a list whose k_occ_runs has not finished yet — the event recorded behind it has not fired — adds its share later)
uint64_t units_in_runs(const tbrm_resources* r)
{
    uint64_t n = r->run_followers;
    for (const BlockLists* l : r->block_lists)
        if (l->run_launches) {
            if (hipEventQuery(l->ev_done) != hipSuccess) { (void) hipGetLastError(); continue; }
            n += l->run_launches * (uint64_t) std::max(l->count_host[1], 0);
        }
    return n;
}

// The run list of a dual launch's units cut for runs of up to `len`: what the occlusion launch and k_occ_runs are handed. A list
// cut for another length (the occ_run tunable changed) is cut anew, on the occlusion stream behind the launches that walk it.
bool run_list_for(tbrm_resources* r, BlockLists* l, int len, OccRuns* out, bool* build)
{
    if (!l->runs) return false;
    *build = l->run_len != len;
    if (*build && l->run_launches) { // (the number the old cut left for units_in_runs)
        ++r->sync_calls;
        (void) hipEventSynchronize(l->ev_done);
        retire_run_list(r, l);
    }
    l->run_len = len;
    *out = OccRuns{len, l->runs, l->count, l->count_host};
    return true;
}

static void drain(tbrm_resources* r)
{
    ++r->sync_calls;
    (void) hipStreamSynchronize(r->stream);
    if (r->occ_stream) (void) hipStreamSynchronize(r->occ_stream);
}

// (the units of a dual launch — no ranks — have their run list behind the work list: units + 8 * kOccRunMax words, OccRuns)
static BlockLists* allocate_lists(size_t blocks, bool with_ranks)
{
    BlockLists* l = new BlockLists{};
    const size_t list_words = with_ranks ? blocks : 2 * blocks + 8 * kOccRunMax;
    bool ok = hipMalloc((void**) &l->flags, blocks) == hipSuccess && hipMalloc((void**) &l->list, list_words * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc((void**) &l->count, 16 * sizeof(int)) == hipSuccess &&
              hipHostMalloc((void**) &l->count_host, 2 * sizeof(int), hipHostMallocDefault) == hipSuccess &&
              hipEventCreateWithFlags(&l->ev_done, hipEventDisableTiming) == hipSuccess;
    if (with_ranks) ok = ok && hipMalloc((void**) &l->slot, blocks * sizeof(int32_t)) == hipSuccess;
    else if (ok) l->runs = l->list + blocks;
    if (!ok) {
        (void) hipGetLastError();
        free_lists(l);
        fail(TBRM_ERR_OUT_OF_MEMORY, "no memory for the block lists of a pass (%zu blocks)", blocks);
        return nullptr;
    }
    l->cap = blocks;
    return l;
}

// tbrm_resources_reserve: lists made ahead of their first use
BlockLists* make_spare_lists(tbrm_resources* r, size_t blocks, bool with_ranks)
{
    BlockLists* l = allocate_lists(blocks, with_ranks);
    if (l) r->spare_lists.push_back(l);
    return l;
}

// Beyond kMaxLists (many distinct light directions under one volume / transfer function / window): the least recently used
// lists go, as far as no factor cache entry stores its blocks under their ranks. Buffers that launches in flight may still
// read are never freed under them: the streams are drained first.
static void prune(tbrm_resources* r)
{
    if (r->block_lists.size() < kMaxLists) return;
    drain(r);
    count_alloc(r, 4, "pruned block lists");
    std::vector<BlockLists*> keep;
    std::sort(r->block_lists.begin(), r->block_lists.end(), [](const BlockLists* a, const BlockLists* b) { return a->last_use > b->last_use; });
    for (BlockLists* l : r->block_lists) {
        if (l->users > 0 || l->last_use > r->block_lists_op_floor || keep.size() < kMaxLists / 2) keep.push_back(l); // (never the ones the operator being planned holds)
        else { retire_run_list(r, l); free_lists(l); }
    }
    // (units lists whose passes' lists went: ids are never reused, so they are merely never found again)
    r->block_lists.swap(keep);
}

// New lists for `blocks` blocks: the buffers of lists that were computed from skipping metadata which is gone (a new volume,
// transfer function or window: nothing will ask for them again) if some are large enough — no allocation while only the
// window moves (APerformanceTest1's sweep) —, else fresh ones.
// A list's buffers are rewritten only when nothing in flight can still read them: every launch that is handed a list's flags,
// work list or ranks notes its operator in BlockLists::last_read_op (the planner, for every list a plan points at), and a stale
// list — nobody's ranks (users == 0), computed from metadata that is gone — is taken again once that operator's "sweeps done"
// event has FIRED (op_finished: asked, not waited for). Round 5 drained the streams once per metadata change instead, which left a
// window: a list pinned by a cache entry across the change could be read by a sweep enqueued AFTER that drain and recycled when the
// entry let go of it.
static BlockLists* new_lists(tbrm_resources* r, size_t blocks, bool with_ranks)
{
    BlockLists* l = nullptr;
    // a spare one first (tbrm_resources_reserve): never used, nothing reads it
    for (size_t i = 0; i < r->spare_lists.size(); ++i) {
        BlockLists* c = r->spare_lists[i];
        if (c->cap >= blocks && (c->slot != nullptr) == with_ranks) {
            l = c;
            r->spare_lists.erase(r->spare_lists.begin() + (long) i);
            r->block_lists.push_back(l);
            break;
        }
    }
    if (!l) {
        // then one computed from metadata that is gone (nothing will ask for it again); then — a reserved handle keeps to the lists it
        // was given — the least recently used one of the current metadata (a light that turns leaves a trail of signatures behind)
        auto free_to_take = [&](const BlockLists* c) {
            return c->users == 0 && c->cap >= blocks && (c->slot != nullptr) == with_ranks && c->last_use <= r->block_lists_op_floor;
        };
        for (BlockLists* c : r->block_lists)
            if (c->empty_gen != r->empty_gen && free_to_take(c) && op_finished(r, c->last_read_op) && (!l || c->cap < l->cap)) l = c;
        if (!l && r->reserved)
            for (BlockLists* c : r->block_lists)
                if (free_to_take(c) && (!l || c->last_use < l->last_use) && op_finished(r, c->last_read_op)) l = c;
        if (l) {
            retire_run_list(r, l); // (op_finished: its kernels are done)
            l->sig.clear();
            l->a_id = l->b_id = 0;
            l->enqueued = false;
        }
    }
    if (!l) {
        prune(r);
        count_alloc(r, with_ranks ? 6 : 5, "new block lists (no spare or quiet list to take)");
        l = allocate_lists(blocks, with_ranks);
        if (!l) return nullptr;
        r->block_lists.push_back(l);
    }
    l->blocks = blocks;
    l->count_host[0] = l->count_host[1] = 0;
    l->empty_gen = r->empty_gen;
    l->id = ++r->block_lists_serial;
    l->last_use = l->id;
    l->last_read_op = r->op_serial; // (the operator being planned will launch over them)
    return l;
}

BlockLists* block_lists_for_pass(tbrm_resources* r, const ChunkParams& p, int occ_mode)
{
    std::vector<int32_t> sig;
    block_lists_signature(p, occ_mode, sig);
    for (BlockLists* l : r->block_lists)
        if (l->a_id == 0 && l->empty_gen == r->empty_gen && l->sig == sig) {
            l->last_use = ++r->block_lists_serial;
            l->last_read_op = std::max(l->last_read_op, r->op_serial);
            return l;
        }
    BlockLists* l = new_lists(r, (size_t) p.occ_groups * p.occ_blocks_y * p.occ_blocks_x, true);
    if (l) l->sig.swap(sig);
    return l;
}

BlockLists* block_lists_for_dual(tbrm_resources* r, const BlockLists* a, const BlockLists* b, size_t units)
{
    for (BlockLists* l : r->block_lists)
        if (l->a_id == a->id && l->b_id == b->id && l->blocks == units) {
            l->last_use = ++r->block_lists_serial;
            l->last_read_op = std::max(l->last_read_op, r->op_serial);
            return l;
        }
    BlockLists* l = new_lists(r, units, false);
    if (l) { l->a_id = a->id; l->b_id = b->id; }
    return l;
}

bool block_lists_count(BlockLists* l, bool wait, size_t* count)
{
    if (!l || !l->enqueued || !l->ev_done) return false;
    if (wait) (void) hipEventSynchronize(l->ev_done);
    else if (hipEventQuery(l->ev_done) != hipSuccess) { (void) hipGetLastError(); return false; }
    *count = (size_t) std::max(*l->count_host, 0);
    return true;
}

} // namespace tbrm_host
