// The wave-family kernels that dispatch, included twice by fjsp_kernels.hip: with FJSP_REC 0 they are step_kernel /
// rollout_kernel, with FJSP_REC 1 their recording builds step_rec_kernel / rollout_rec_kernel, which also store every
// dispatch in `rec` (SchedRec, fjsp_env_record_schedule).  One text for both keeps the plain kernels' code exactly what it
// is without recording (a shared __device__ body inlined into both changes the optimiser's pass order, hence the code).
// The kernels with the actor inside the launch follow the same scheme in fjsp_kernels_policy.inc.
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

#undef FJSP_K
#undef FJSP_REC_ARG
#undef FJSP_REC_LOCAL
