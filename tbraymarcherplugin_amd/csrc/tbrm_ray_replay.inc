// tbrm_ray_replay.inc — stage 4 of a trip of the frame kernels, included where it runs (k_raymarch_lit; all of a k_relight trip
// behind its shading): the lanes of a ray exchange their samples x = (colour * alpha, alpha) through s_x and each replays accumulate()
// over the ray's kRayLanes samples in ray order; the early exit belongs to the full steps only (:75-79). LABELS: with the label step
// of every sample behind its data step. Text and not a function: at 80 registers the march's allocation does not survive the stage
// as an inlined function (tbrm_kernels.hip). Names it uses of its surroundings: p, s_x, xs, x, base, max_steps, le, done, and for
// LABELS s_lb, s_lab, lab, final_step.
            s_x[threadIdx.x] = x;
            if constexpr (LABELS) s_lb[threadIdx.x] = (short) lab;
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int t = 0; t < kRayLanes; ++t) {
                const float4 c = xs[t];
                const bool is_full_step = base + t < max_steps;
                const bool data_step = !(c.w < 0.0f);
                // (a slot without a step to take gets no exit test either: a slab stage leaves the state it took over alone)
                if (done || (!LABELS && !data_step)) continue;
                if (data_step) accumulate(le, c);
                if constexpr (LABELS) { // then the label step (AccumulateOneRaymarchLabelStep: unlit)
                    const int lb = s_lb[(threadIdx.x & ~(kRayLanes - 1)) + t];
                    if (lb >= 0) {
                        float4 e;
                        if (is_full_step) e = s_lab[lb];
                        else { // the fractional step (once per ray): its own a' with the step 100 * FinalStep
                            const float4 raw = p.lab_colors[lb];
                            const float a = raw.w != 0.0f ? one_minus_pow01_(1.0f - raw.w, 100.0f * final_step) : 0.0f;
                            e = make_float4(raw.x * a, raw.y * a, raw.z * a, a);
                        }
                        accumulate(le, e);
                    }
                }
                if (exit_reached(le[3], is_full_step)) { le[3] = 1.0f; done = true; }
            }
            __builtin_amdgcn_wave_barrier();
