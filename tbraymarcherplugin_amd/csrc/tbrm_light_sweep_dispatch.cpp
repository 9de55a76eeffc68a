// tbrm_light_sweep_dispatch.cpp — the host-side entry of k_light_sweep: checks a launch's shape and hands it to the translation
// unit that holds its mode (tbrm_light_sweep.hip is compiled once per mode: tbraymarcherplugin_amd/build.py).
#include "tbrm_light_sweep.h"

namespace tbrm {

// what every pass of a sweep has to be, launched alone or in a chain: the span (j0, n_steps) whole brick layers of the light
// volume, the occlusion factors handed over block-compact, 32 x 32 tiles over the whole slice plane
static bool sweep_pass_ok(const ChunkParams& p, const SweepParams& q, int mode)
{
    const bool aligned = (p.n_steps & 7) == 0 && (p.j0 & 7) == (p.dir > 0 ? 0 : 7) && p.occ_phase == 0 && p.n_steps <= sweep_max_slices();
    if (!aligned || !p.compact || !p.ones || !p.a.fs_slot || (sweep_two_streams(mode) && !p.r.fs_slot)) return false;
    if (q.reinit_slice < 0 || q.reinit_slice > 7 || (q.reinit_slice > 0 && p.n_steps < 16)) return false;
    if (q.n_real > p.n_steps || q.n_real <= p.n_steps - 8) return false; // (padding: less than one brick layer)
    return p.tiles_x == (p.W + kSweepTile - 1) / kSweepTile && p.tiles_y == (p.H + kSweepTile - 1) / kSweepTile;
}

// advances every tile through the span (j0, n_steps) in one launch; mode PASS_ADD, PASS_CHANGE, PASS_ADD2 or PASS_PLANES
hipError_t launch_light_sweep(const ChunkParams& p, const SweepParams& q, int mode, hipStream_t s)
{
    if (p.n_steps <= 0 || p.tiles_x <= 0 || p.tiles_y <= 0) return hipSuccess;
    if (!sweep_pass_ok(p, q, mode)) return hipErrorInvalidConfiguration;
    if (q.r_from_records && (mode != PASS_CHANGE || !q.rec[1])) return hipErrorInvalidConfiguration;
    if (mode == PASS_ADD) return launch_sweep_unit<PASS_ADD>(p, q, s);
    if (mode == PASS_CHANGE) return launch_sweep_unit<PASS_CHANGE>(p, q, s);
    if (mode == PASS_ADD2) return launch_sweep_unit<PASS_ADD2>(p, q, s);
    if (mode == PASS_PLANES) return launch_sweep_unit<PASS_PLANES>(p, q, s);
    return hipErrorInvalidConfiguration;
}

// Several passes in one launch (tbrm_internal.h SweepChainArgs): every pass checked like a launch of its own
hipError_t launch_light_sweep_chain(const SweepChainArgs& c, int mode, hipStream_t s)
{
    if (c.n < 1 || c.n > kSweepChainMax || (mode != PASS_ADD && mode != PASS_CHANGE)) return hipErrorInvalidConfiguration;
    int ticket0 = 0;
    for (int k = 0; k < c.n; ++k) {
        const ChunkParams& p = c.pass[k].p;
        const SweepParams& q = c.pass[k].q;
        if (p.n_steps <= 0 || p.tiles_x <= 0 || p.tiles_y <= 0 || !sweep_pass_ok(p, q, mode)) return hipErrorInvalidConfiguration;
        if (q.r_from_records || q.lv_f32 || (q.debug & 1)) return hipErrorInvalidConfiguration;
        const SweepLink& l = c.pass[k].link;
        if (!l.prog_out || !l.prog_in || l.ticket0 != ticket0 || (k == 0) != (l.in_G == 0) || q.ticket != c.pass[0].q.ticket) return hipErrorInvalidConfiguration;
        ticket0 += p.tiles_x * p.tiles_y;
    }
    for (int k = 0; k < c.n; ++k)
        if (c.pass[k].link.total_tiles != ticket0) return hipErrorInvalidConfiguration;
    return mode == PASS_ADD ? launch_sweep_chain_unit<PASS_ADD>(c, s) : launch_sweep_chain_unit<PASS_CHANGE>(c, s);
}

} // namespace tbrm
