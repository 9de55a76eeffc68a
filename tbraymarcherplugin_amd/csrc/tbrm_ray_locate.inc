// tbrm_ray_locate.inc — stages 1 and 2 of a trip of the marching kernels, included where they run (k_raymarch_lit, k_raymarch_hit):
// advance the lane's position to its sample of the trip, then decide whether the sample has to be evaluated and where its data taps
// lie. Text and not a function, for the reason tbrm_ray_replay.inc gives. Names it uses of its surroundings: p, b, base, kRayLanes,
// DMODE, TAB, SLAB, done, max_steps, n_samples, final_step, step_world, adds, pos0 .. pos2, sv0 .. sv2, nx, ny, nz, lnz (SLAB), tab_x,
// tab_y, tab_z (TAB), safe_until, eager, wave_skip, inv_texels_per_step. Names it leaves: idx, q0 .. q2, step, is_full, has, live, lab,
// ix, iy, iz, fx, fy, fz, tab_dt, any_live.
        const int idx = base + b; // this lane's sample of the ray
        // ---- 1. advance. CurPos += LocalCamVec before every full sample (:67): sample idx < max_steps sits idx+1 additions in, the
        // fractional sample max_steps additions plus one scaled step
        const int want = min(idx + 1, max_steps);
        if (__builtin_amdgcn_ballot_w64(!done && want - adds != kRayLanes) == 0) { // mid-ray everywhere: no predication
#pragma unroll
            for (int t = 0; t < kRayLanes; ++t) { pos0 = pos0 + sv0; pos1 = pos1 + sv1; pos2 = pos2 + sv2; }
            adds += kRayLanes;
        } else {
#pragma unroll
            for (int t = 0; t < kRayLanes; ++t)
                if (adds < want) { pos0 = pos0 + sv0; pos1 = pos1 + sv1; pos2 = pos2 + sv2; ++adds; }
        }
        float q0 = pos0, q1 = pos1, q2 = pos2, step = step_world;
        const bool is_full = idx < max_steps;
        const bool has = !done && idx < n_samples;
        if (!is_full) { q0 = pos0 + (sv0 * final_step); q1 = pos1 + (sv1 * final_step); q2 = pos2 + (sv2 * final_step); step = 100.0f * final_step; }

        // ---- 2. locate: does the sample have to be evaluated (live), where do its data taps lie (texel split, TAB offsets), and how far
        // does its brick's leap distance prove the lane's next samples empty (safe_until)
        bool live = has && idx > safe_until && !(p.clip_mode && is_clipped(q0, q1, q2, p.cc, p.cd));
        if constexpr (SLAB) { // only the samples of this handle's slab
            const int zi = min((int) (saturate_(q2) * lnz), p.lv_dims[2] - 1);
            live = live && zi >= p.slab_z0 && zi < p.slab_z1;
        }
        int ix = 0, iy = 0, iz = 0;
        float fx = 0.0f, fy = 0.0f, fz = 0.0f;
        int lab = -1; // LABELS: the label of this lane's sample when it has a label step to take
        // (after a trip in which no lane of the wave sampled, the lanes inside their proven-empty range look their brick up
        // again as well: all ranges then start from here, and the wave can take the trips they share in one go — below)
        const bool renew = eager && has && !live && idx <= safe_until;
        TapOffsets tab_dt{}; // TAB: the data taps' offsets, out of the tables
        if (live || renew) {
            if constexpr (TAB) { // (the host's promise behind the tables: positions within a step of the unit cube)
                texel_split_bounded(q0, nx, ix, fx);
                texel_split_bounded(q1, ny, iy, fy);
                texel_split_bounded(q2, nz, iz, fz);
            } else {
                texel_split(q0, nx, ix, fx);
                texel_split(q1, ny, iy, fy);
                texel_split(q2, nz, iz, fz);
            }
            uint32_t tab_brick = 0;
            if constexpr (TAB) { // (base taps -2 .. n: the host's promise; the clamp only keeps a broken promise, and the +1 entry, inside the tables)
                const int tx = min(max(ray_tab_index(ix), 0), ray_tab_last_base(p.data.nx));
                const int ty = min(max(ray_tab_index(iy), 0), ray_tab_last_base(p.data.ny));
                const int tz = min(max(ray_tab_index(iz), 0), ray_tab_last_base(p.data.nz));
                const uint2 ax = tab_x[tx], bx1 = tab_x[tx + 1], ay = tab_y[ty], by1 = tab_y[ty + 1], az = tab_z[tz], bz1 = tab_z[tz + 1];
                tab_dt.x0 = ax.x; tab_dt.x1 = bx1.x; tab_dt.y0 = ay.x; tab_dt.y1 = by1.x; tab_dt.z0 = az.x; tab_dt.z1 = bz1.x;
                tab_brick = ax.y + ay.y + az.y;
            }
            if (p.skip_dist) { // a sample based in a brick that maps every reachable value to opacity 0 is an exact no-op
                int dist;
                if constexpr (TAB) dist = p.skip_dist[tab_brick];
                else {
                    const int bx = address<DMODE>(ix, p.data.nx) >> kBrickShift;
                    const int by = address<DMODE>(iy, p.data.ny) >> kBrickShift;
                    const int bz = address<DMODE>(iz, p.data.nz) >> kBrickShift;
                    dist = p.skip_dist[(bz * p.bny + by) * p.bnx + bx];
                }
                live = live && dist == 0;
                // Every brick within Chebyshev distance < dist is empty as well. From anywhere inside this brick a base
                // tap has to move more than 8*(dist-1) texels along some axis to leave them, and a base tap moves at
                // most 1 texel more than the position does: the lane's samples up to that many steps ahead need no test.
                if (dist >= 2) safe_until = max(safe_until, idx + (int) fminf(((float) (8 * (dist - 1)) - 1.25f) * inv_texels_per_step, 1.0e6f));
            }
        }
        const bool any_live = !wave_skip || __builtin_amdgcn_ballot_w64(live) != 0;
