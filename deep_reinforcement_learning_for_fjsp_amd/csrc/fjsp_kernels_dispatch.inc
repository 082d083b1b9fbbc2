// The wave-family kernels that dispatch, included twice by fjsp_kernels.hip: with FJSP_REC 0 they are step_kernel /
// rollout_kernel / rollout_policy_kernel, with FJSP_REC 1 their recording builds step_rec_kernel / rollout_rec_kernel /
// rollout_policy_rec_kernel, which also store every dispatch in `rec` (SchedRec, fjsp_env_record_schedule).  One text for
// both keeps the plain kernels' code exactly what it is without recording (a shared __device__ body inlined into both
// changes the optimiser's pass order, hence the code).
#if FJSP_REC
#define FJSP_K(name) name##_rec_kernel
#define FJSP_REC_ARG , SchedRec rec
#define FJSP_REC_LOCAL
#else
#define FJSP_K(name) name##_kernel
#define FJSP_REC_ARG
#define FJSP_REC_LOCAL const SchedRec rec{};
#endif

// One step of every environment.  Single-order variants share the observation tail inside the workgroup
// (observe_tail above): every live wave of a workgroup passes the same four barriers, whatever happened to its
// environment (finished episode, invalid rule), so nothing below returns between the first barrier and the last.
// SJ: one job per kind in every instance of the batch (compile-time: the single-job kernel carries none of the list walks,
// statistics rows or their registers)
template <int KC, int V, bool SJ>
// (four chunks of per-lane operation state do not fit 128 VGPRs: K > 128 runs at half the occupancy instead of spilling)
__global__ __launch_bounds__(256, KC >= 4 ? 2 : (KC == 2 ? 3 : 4)) void FJSP_K(step)(DevBatch b, const uint8_t *actions, const double *mo, int autoreset,
                                                      double *state_out, double *reward_out, uint8_t *done_out,
                                                      int16_t *trace_km, uint8_t *ready FJSP_REC_ARG) {
    constexpr bool REC = FJSP_REC != 0;
    FJSP_REC_LOCAL
    constexpr bool SHARED = FJSP_SHARED_TAIL && !is_mord_v<V>;
    const int wave = uni((int)(threadIdx.x >> 6));   // wave-uniform: keeps every record pointer in SGPRs
    const int env_raw = blockIdx.x * (blockDim.x >> 6) + wave;
    // the waves past the last environment of a partial workgroup address the last environment until their loads are
    // out and leave then: no kernel argument has to arrive before the state loads can be issued
    const int env = min(env_raw, b.N - 1);
#if defined(FJSP_ABLATE) && FJSP_ABLATE == 5
    return;                                     // diagnostic: launch overhead only
#endif
    W<KC, V> w;
    STAMP_BEGIN(w);
    // The action pair (wave-uniform, 2-byte aligned: checked by the host entry points) comes through the VECTOR memory
    // path and is only moved to scalar registers after the state loads are out: a scalar load of it here would be waited
    // for at once -- scalar loads return out of order, every wait on one drains them all -- one full memory round trip
    // before the first state load could be issued.
    const uint32_t araw = reinterpret_cast<const uint16_t *>(actions)[env];
    const uint32_t lds_stride = (uint32_t)lds_bytes_per_wave(b.JP, b.MP, kWave * KC, false);
    open_env<KC, V, SJ ? 1 : 0>(w, &b, env, fjsp_lds + wave * lds_stride, false, true, true);
    if (env_raw >= b.N) return;                       // (a finished wave no longer counts at the workgroup's barriers)
    if constexpr (REC) { w.rec = rec.rec; w.rec_cap = rec.cap; }
    const int a0 = uni((int)(araw & 0xFFu)), a1 = uni((int)(araw >> 8));
    STAMP(w, 0);
#if defined(FJSP_ABLATE) && FJSP_ABLATE == 4
    store_dynamic<KC, V>(w, false);                // diagnostic: state in / state out only
    return;
#endif
    if (is_mord_v<V> && ready) {
        // asynchronous arrival service (fjsp_env_step_async): environments parked at an order arrival sit this launch
        // out (ready = 0), one that arrival_kernel has just finished in this same call keeps the outputs it was given
        if (w.pending == 2) { if (w.lane == 0) env_ptr<EnvScalars>(b, env, 0)->pending = 0; return; }
        if (w.pending == 1) { if (w.lane == 0) ready[env] = 0; return; }
    }
    const bool need_obs = state_out != nullptr;
    bool go = true;                  // this wave's environment takes a step in this launch
    if (w.done) {
        if (autoreset != 1) {        // 0: flag the misuse; 2: idle silently (non-fused rollout fallback)
            if (autoreset == 0) w.status |= FJSP_ST_STEP_AFTER_DONE;
            go = false;
        } else {
            init_episode<KC, V>(w, &b, nullptr, true);
        }
    } else if (w.single_job || !w.stats_ok) {
        compute_params<KC, V>(w);            // a handful of selects; batches with longer lists found the statistics in the record
    }
    STAMP(w, 1);
#if defined(FJSP_ABLATE) && FJSP_ABLATE == 3
    store_dynamic<KC, V>(w, false);                // diagnostic: + compute_params
    return;
#endif
    int k_sel = -1, m_sel = -1;
    double reward = 0.0;
    const double *mo_e = mo ? mo + (size_t)env * 4 : nullptr;
    if constexpr (!SHARED) {
        if (go) reward = env_step<KC, V, 8, REC>(w, &b, a0, a1, mo_e, state_out, &k_sel, &m_sel, need_obs);
        if (go && w.pending) {
            // an order arrived inside this step: park the env for the host LP service (fjsp_env.hip), which
            // finishes the step with arrival_kernel; the outputs of this env are written there
            if (w.lane == 0) {
                int16_t *stash = reinterpret_cast<int16_t *>(w.er + b.L.e_lpq) + 2 * b.KP;
                stash[0] = (int16_t)k_sel; stash[1] = (int16_t)m_sel;
            }
            // take a slot of the service's staging area and leave the LP inputs there: the host fetches the
            // inputs of all parked envs with one copy
            uint32_t slot = 0;
            if (w.lane == 0) { slot = atomicAdd(b.pending_count, 1u); if (slot < (uint32_t)b.N) b.pending_count[1 + slot] = (uint32_t)env; }
            slot = min(uniu(slot), (uint32_t)b.N - 1u);     // (N slots: an env parks at most once per service; see service_arrivals)
            wave_sync_global();
            const uint32_t *src = reinterpret_cast<const uint32_t *>(w.er + b.L.e_lpq);     // u16[2][KP] as KP words
            uint32_t *dst = reinterpret_cast<uint32_t *>(b.lp_in + (size_t)slot * 2 * b.KP);
            for (int i = w.lane; i < b.KP; i += kWave) dst[i] = src[i];
            if (ready && w.lane == 0) ready[env] = 0;
            store_dynamic<KC, V>(w, false, false);        // (statistics are stale until arrival_kernel finishes the step)
            return;
        }
    } else {
        if (go && need_obs && w.obs_stale) obs_refresh<KC, V>(w);
        if (go) go = env_step_decide<KC, V, 8, REC>(w, &b, a0, a1, &k_sel, &m_sel);
#if defined(FJSP_ABLATE) && (FJSP_ABLATE == 7 || FJSP_ABLATE == 8 || FJSP_ABLATE == 9)
        store_dynamic<KC, V>(w, false);
        return;
#endif
        double frv[KC], grv[KC];
        long long tard_unproc = 0;
        if (go) {
            w.step_count++;                                                  // SO_FJSSP.py:252
            compute_params<KC, V>(w);
            STAMP(w, 5);
#if !(defined(FJSP_ABLATE) && FJSP_ABLATE == 2)
            tard_unproc = observe_prepare<KC, V>(w, !need_obs, frv, grv);
#endif
            STAMP(w, 6);
        }
#if !(defined(FJSP_ABLATE) && FJSP_ABLATE == 2)
        if (need_obs) {              // (uniform over the grid: a kernel argument)
            // the walker runs the sequential tail of every environment of the workgroup; slots whose wave has
            // nothing to observe (finished episode, error) announce an empty row
            const int nslots = min(4, b.N - (int)blockIdx.x * 4);
            const int walker = min((int)(blockIdx.x & 3u), nslots - 1);
            if (!go && w.lane == 0) w.hdrL[H_N8] = 0;
            tail_sync<true>();
            STAMP(w, 7);
            if (wave == walker) tail_pass<V, 8>(fjsp_lds, lds_stride, nslots, kWave * KC);
            tail_sync<true>();
            STAMP(w, 8);
            if (go) { observe_deviations<KC, V>(w, frv, grv); wave_sync(); }     // (the standard deviations: no walk, no barrier)
            STAMP(w, 9);
            STAMP(w, 10);
            if (go) {
                observe_finish<KC, V, 8>(w);
#if !(defined(FJSP_ABLATE) && FJSP_ABLATE == 1)
                emit_state<KC, V>(w, state_out, false);
#endif
                STAMP(w, 11);
            }
        } else if (go) {
            w.obs_stale = 1;
        }
#endif
        if (go) reward = step_reward<KC, V>(w, mo_e, V == FJSP_VARIANT_SO_SFJSP ? 0 : tard_unproc);
    }
    if (w.lane == 0) {
        if (reward_out) reward_out[env] = reward;
        if (done_out) done_out[env] = (uint8_t)w.done;
        if (trace_km) { trace_km[(size_t)env * 2] = (int16_t)k_sel; trace_km[(size_t)env * 2 + 1] = (int16_t)m_sel; }
        if (ready) ready[env] = 1;
    }
    store_dynamic<KC, V>(w, false);
    STAMP(w, 12);
    STAMP_FLUSH(w);
}

// T fused steps per launch: the environment lives in registers + LDS for the whole episode.
template <int KC, int V>
__global__ __launch_bounds__(256, (KC == 1 && V == FJSP_VARIANT_SO_FJSSP) ? 4 : 1) void FJSP_K(rollout)(DevBatch b, const uint8_t *actions, const double *mo, int T,
                                                      int16_t *trace_km, double *reward_out, double *state_last FJSP_REC_ARG) {
    constexpr bool REC = FJSP_REC != 0;
    FJSP_REC_LOCAL
    const int wave = uni((int)(threadIdx.x >> 6));   // wave-uniform: keeps every record pointer in SGPRs
    const int env = blockIdx.x * (blockDim.x >> 6) + wave;
    if (env >= b.N) return;
    W<KC, V> w;
    open_env<KC, V>(w, &b, env, fjsp_lds + wave * lds_bytes_per_wave(b.JP, b.MP, b.KP, true), true, true);
    if constexpr (REC) { w.rec = rec.rec; w.rec_cap = rec.cap; }
    compute_params<KC, V>(w);
    for (int s = 0; s < T; ++s) {
        const size_t o = (size_t)s * b.N + env;
        int k_sel = -1, m_sel = -1;
        double reward = 0.0;
        const bool live = !w.done && !(w.status & (FJSP_ST_BAD_TASK_RULE | FJSP_ST_BAD_MACHINE_RULE | FJSP_ST_NO_EVENT));
        if (live) {
            const int a0 = actions[o * 2], a1 = actions[o * 2 + 1];
            reward = env_step<KC, V, 2, REC>(w, &b, uni(a0), uni(a1), mo ? mo + (size_t)env * 4 : nullptr, state_last, &k_sel, &m_sel,
                                             state_last != nullptr);
        }
        if (w.lane == 0) {
            if (trace_km) { trace_km[o * 2] = (int16_t)k_sel; trace_km[o * 2 + 1] = (int16_t)m_sel; }
            if (reward_out) reward_out[o] = reward;
        }
    }
    store_dynamic<KC, V>(w, true);
}

// The T-step rollout with the actor inside the launch (replaces the per-step loop MPPPO.py:245-252: policy
// inference, sampling, env.step, buffer append): one wavefront per environment for the whole episode, sixteen
// per workgroup sharing the actor's weights in LDS.  Per step: actor_probs on the current state, sample_action
// by lane 0 (the counter-based stream of fjsp_policy_sample: same seed, same actions as the per-step path),
// the environment step, the buffer row.  Finished environments idle; their rows are marked invalid.
template <int KC, int V>
__global__ __launch_bounds__(1024) void FJSP_K(rollout_policy)(DevBatch b, ActorParams ap, PolicyRolloutIO io, const double *mo, int T FJSP_REC_ARG) {
    constexpr bool REC = FJSP_REC != 0;
    FJSP_REC_LOCAL
    float *lds = reinterpret_cast<float *>(fjsp_lds);
    actor_lds_fill(lds, ap, (int)threadIdx.x, (int)blockDim.x);
    __syncthreads();                                   // (the only workgroup barrier: waves may leave after it)
    const int wave = uni((int)(threadIdx.x >> 6));
    const int env = blockIdx.x * 16 + wave;
    if (env >= b.N) return;
    const uint32_t env_stride = (uint32_t)lds_bytes_per_wave(b.JP, b.MP, b.KP, false);
    unsigned char *wave_lds = fjsp_lds + ((actor_lds_floats(ap.S) * 4 + 255) & ~(size_t)255) +
                              (size_t)wave * (env_stride + (32 + kActorH + kActorAP) * 4);
    float *xs = reinterpret_cast<float *>(wave_lds + env_stride);
    float *hs = xs + 32, *ps = hs + kActorH;
    W<KC, V> w;
    open_env<KC, V>(w, &b, env, wave_lds, false, true);
    if constexpr (REC) { w.rec = rec.rec; w.rec_cap = rec.cap; }
    compute_params<KC, V>(w);
    const int S = ap.S, A = ap.A, N = b.N;
    if (w.lane < S) xs[w.lane] = (float)io.state_in[(size_t)env * S + w.lane];
    const float eps = io.epsilon[0];
    const uint64_t seed = io.seed[0];
    const double *mo_e = mo ? mo + (size_t)env * 4 : nullptr;
    wave_sync();
    for (int t = 0; t < T; ++t) {
        const size_t row = (size_t)t * N + env;
        const bool live = !w.done && !(w.status & (FJSP_ST_BAD_TASK_RULE | FJSP_ST_BAD_MACHINE_RULE | FJSP_ST_NO_EVENT));
        if (!live) {
            if (w.done) w.status |= FJSP_ST_STEP_AFTER_DONE;       // what the per-step loop flags for the same launches
            // (rows of finished environments are masked by `valid`; they still get finite contents -- the last state,
            // like the per-step loop leaves there -- because masked arithmetic multiplies them by zero)
            if (w.lane < S) { io.o_state[row * S + w.lane] = xs[w.lane]; io.o_next[row * S + w.lane] = xs[w.lane]; }
            if (w.lane == 0) {
                io.o_valid[row] = 0.0f; io.o_reward[row] = 0.0f; io.o_done[row] = 1.0f;
                io.o_actions[row * 2] = 0.0f; io.o_actions[row * 2 + 1] = 0.0f; io.o_flat[row] = 0.0f; io.o_logp[row] = 0.0f;
            }
            continue;
        }
        if (w.lane < S) io.o_state[row * S + w.lane] = xs[w.lane];
        actor_probs(lds, xs, hs, ps, S, A);
        int action = 0;
        float logp = 0.0f;
        if (w.lane == 0) {
            const SampledAction sa = sample_action(ps, A, eps, seed, (uint64_t)t, env);
            action = sa.action; logp = sa.log_prob;
        }
        action = uni(action);
        const int a0 = io.pair_div > 0 ? action / io.pair_div : action, a1 = io.pair_div > 0 ? action % io.pair_div : 0;
        int k_sel, m_sel;
        const double reward = env_step<KC, V, 2, REC>(w, &b, a0, a1, mo_e, io.state_last, &k_sel, &m_sel, true, xs);
        if (w.lane < S) io.o_next[row * S + w.lane] = xs[w.lane];
        if (w.lane == 0) {
            io.o_actions[row * 2] = (float)a0; io.o_actions[row * 2 + 1] = (float)a1;
            io.o_reward[row] = (float)reward; io.o_done[row] = (float)w.done; io.o_valid[row] = 1.0f;
            io.o_flat[row] = (float)action; io.o_logp[row] = logp;
        }
    }
    store_dynamic<KC, V>(w, false, false);
}

// Decoding a trained policy (fjsp_env_play_policy): every environment plays to the end of its episode with the actor
// inside the launch, as rollout_policy above but without buffer rows.  One wavefront per environment, sixteen per
// workgroup sharing the actor's weights in LDS.  Per step: actor_probs, then the action -- envs below n_greedy take the
// first index of the largest probability (torch.argmax), the others draw from the stream of fjsp_policy_sample with
// epsilon 0 (counter = step index of this call, env = local index) -- then the environment step.  Step 0 applies
// io.first instead where given.  The start observation is row state_src[env] of state_in: v(t-1) of the state vector is
// not in the env record, so a branch batch reads its source's rows through the map.  A wave leaves its loop once its env
// is done or carries an error bit; T only bounds the loop.
template <int KC, int V>
__global__ __launch_bounds__(1024) void FJSP_K(play_policy)(DevBatch b, ActorParams ap, PolicyPlayIO io, const double *mo, int T FJSP_REC_ARG) {
    constexpr bool REC = FJSP_REC != 0;
    FJSP_REC_LOCAL
    float *lds = reinterpret_cast<float *>(fjsp_lds);
    actor_lds_fill(lds, ap, (int)threadIdx.x, (int)blockDim.x);
    __syncthreads();                                   // (the only workgroup barrier: waves may leave after it)
    const int wave = uni((int)(threadIdx.x >> 6));
    const int env = blockIdx.x * 16 + wave;
    if (env >= b.N) return;
    const int S = ap.S, A = ap.A, N = b.N;
    const int src = uni(io.state_src ? io.state_src[env] : env);
    if (src < 0 || src >= io.n_state_in) {             // (refused by the host entry; an env given no start row stays put)
        if (__lane_id() == 0) io.steps_out[env] = 0;
        return;
    }
    const uint32_t env_stride = (uint32_t)lds_bytes_per_wave(b.JP, b.MP, b.KP, false);
    unsigned char *wave_lds = fjsp_lds + ((actor_lds_floats(ap.S) * 4 + 255) & ~(size_t)255) +
                              (size_t)wave * (env_stride + (32 + kActorH + kActorAP) * 4);
    float *xs = reinterpret_cast<float *>(wave_lds + env_stride);
    float *hs = xs + 32, *ps = hs + kActorH;
    W<KC, V> w;
    open_env<KC, V>(w, &b, env, wave_lds, false, true);
    if constexpr (REC) { w.rec = rec.rec; w.rec_cap = rec.cap; }
    compute_params<KC, V>(w);
    const double x0 = w.lane < S ? io.state_in[(size_t)src * S + w.lane] : 0.0;
    if (w.lane < S) xs[w.lane] = (float)x0;
    const uint64_t seed = io.seed ? io.seed[0] : 0;
    const bool greedy = env < io.n_greedy;
    const double *mo_e = mo ? mo + (size_t)env * 4 : nullptr;
    wave_sync();
    double reward = 0.0;
    int t = 0;
    for (; t < T; ++t) {
        if (w.done || (w.status & (FJSP_ST_BAD_TASK_RULE | FJSP_ST_BAD_MACHINE_RULE | FJSP_ST_NO_EVENT))) break;
        int a0, a1;
        if (t == 0 && io.first) {
            a0 = uni((int)io.first[(size_t)env * 2]); a1 = uni((int)io.first[(size_t)env * 2 + 1]);
        } else {
            actor_probs(lds, xs, hs, ps, S, A);
            int action = 0;
            if (w.lane == 0) {
                if (greedy) {
                    float best = ps[0];
                    for (int a = 1; a < A; ++a)
                        if (ps[a] > best) { best = ps[a]; action = a; }
                } else {
                    action = sample_action(ps, A, 0.0f, seed, (uint64_t)t, env).action;
                }
            }
            action = uni(action);
            a0 = io.pair_div > 0 ? action / io.pair_div : action; a1 = io.pair_div > 0 ? action % io.pair_div : 0;
        }
        int k_sel, m_sel;
        reward = env_step<KC, V, 2, REC>(w, &b, a0, a1, mo_e, io.state_last, &k_sel, &m_sel, true, xs);
        if (io.actions_out && w.lane == 0) {
            const size_t row = (size_t)t * N + env;
            io.actions_out[row * 2] = (uint8_t)a0; io.actions_out[row * 2 + 1] = (uint8_t)a1;
        }
    }
    if (w.lane == 0) {
        io.steps_out[env] = t;
        io.done_last[env] = (uint8_t)w.done;
        if (t > 0) io.reward_last[env] = reward;
    }
    if (t == 0 && w.lane < S) io.state_last[(size_t)env * S + w.lane] = x0;     // (an env that took no step keeps its start row)
    store_dynamic<KC, V>(w, false, false);
}

#undef FJSP_K
#undef FJSP_REC_ARG
#undef FJSP_REC_LOCAL
