// tbrm_ray_leap.inc — stage 5 of a trip of the marching kernels, included where it runs (k_raymarch_lit, k_raymarch_hit). Text and
// not a function, for the reason tbrm_ray_replay.inc gives. Names it uses of its surroundings: b, base, kRayLanes, done, max_steps,
// any_live, safe_until, eager, renew_wait, adds, pos0 .. pos2, sv0 .. sv2.
        // ---- 5. leap. Empty space, wave-wide: when no lane of the wave had anything to sample in this trip, the trips that EVERY marching
        // lane would spend the same way — its sample still within its proven-empty range (safe_until), the ray still in its
        // full steps — are taken in one go: their only effect is the positions' additions, performed one by one as before
        // (a position is reached by performing every addition of the ray). 70 % of the benchmark's trips are of this kind.
        const bool renewed = eager;
        eager = false;
        if (!any_live) {
            int k_lane = INT32_MAX; // whole trips this lane can take blind after this one
            if (!done) {
                const int ahead = safe_until - base - b; // its sample of trip t from now is base + kRayLanes t + b
                const int by_safe = ahead >= kRayLanes ? ahead / kRayLanes : 0;
                const int left = max_steps - 1 - (base + kRayLanes); // full steps behind the end of this trip, but for the last
                const int by_length = left >= kRayLanes ? left / kRayLanes : 0;
                k_lane = min(by_safe, by_length);
            }
            int k = 0; // the wave's minimum (small: counted up with ballots)
            while (k < 64 && __builtin_amdgcn_ballot_w64(k_lane <= k) == 0) ++k;
            if (k > 0) {
                for (int t = 0; t < k * kRayLanes; ++t) { pos0 = pos0 + sv0; pos1 = pos1 + sv1; pos2 = pos2 + sv2; }
                adds += k * kRayLanes;
                base += k * kRayLanes;
            }
            // (next to the volume's content the ranges are a trip or two long: renewing them every empty trip would cost more
            // than the look-ups it aligns — small volumes lost 10 - 20 % of their frame that way)
            if (renewed && k == 0) renew_wait = 4;
            else if (renew_wait > 0) --renew_wait;
            eager = renew_wait == 0;
        }
