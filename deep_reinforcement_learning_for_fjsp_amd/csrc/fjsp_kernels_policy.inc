// The kernels that run the actor inside the environment launch: two texts, rollout_policy and play_policy, included eight
// times by fjsp_kernels.hip under three switches.  Each switch adds its suffix to the kernel's name, in this order:
//   FJSP_ORD 1  _orders  one SEGMENT of the episode on a multi-order batch (V = kMord; PolicySegment, fjsp_policy.h).  A step
//               that meets an order arrival parks the env (park_env) and its wave leaves; the host entry runs the arrival
//               service, whose arrival_kernel finishes the parked step into rows indexed by env, and launches the next
//               segment.  The segment arguments (PolicySegment sg of the rollout, int seg of the play) come and go like `rec`:
//               FJSP_ORD 0 has a zero constant in their place and every segment statement under `if constexpr (ORD)`.
//   FJSP_PW 1   _w       W = blockDim.x / 64 environments per workgroup, W in {8, 4, 2, 1} (policy_geometry() in
//               fjsp_kernels.hip picks the largest that fits), at most 512 threads: two waves per SIMD, a budget of 256
//               VGPRs, which the four chunks of W<4, V> need.  FJSP_PW 0: sixteen environments, 1024 threads, the constant
//               16 in the code -- the build of every batch whose sixteen LDS slices fit beside the actor's weights.
//   FJSP_REC 1  _rec     the recording twins, as in fjsp_kernels_dispatch.inc.
// One text for all eight keeps each build's code what it is without the others (see fjsp_kernels_dispatch.inc).
// The only workgroup barrier of either kernel follows actor_lds_fill, before any wave leaves: waves past the last
// environment (a partial last workgroup, N < W) pass it and return; everything after it is per wave.
#if FJSP_ORD
#define FJSP_SFX_ORD _orders
#define FJSP_SEG_ARG(decl) , decl
#define FJSP_SEG_LOCAL(decl)
#else
#define FJSP_SFX_ORD
#define FJSP_SEG_ARG(decl)
#define FJSP_SEG_LOCAL(decl) const decl{};
#endif
#if FJSP_PW
#define FJSP_SFX_PW _w
#define FJSP_PW_THREADS 512
#define FJSP_PW_ENVS ((int)(blockDim.x >> 6))
#else
#define FJSP_SFX_PW
#define FJSP_PW_THREADS 1024
#define FJSP_PW_ENVS 16
#endif
#if FJSP_REC
#define FJSP_SFX_REC _rec
#define FJSP_REC_ARG , SchedRec rec
#define FJSP_REC_LOCAL
#else
#define FJSP_SFX_REC
#define FJSP_REC_ARG
#define FJSP_REC_LOCAL const SchedRec rec{};
#endif
#define FJSP_K_(name, ord, pw, rec) name##ord##pw##rec##_kernel
#define FJSP_K_X(name, ord, pw, rec) FJSP_K_(name, ord, pw, rec)
#define FJSP_K(name) FJSP_K_X(name, FJSP_SFX_ORD, FJSP_SFX_PW, FJSP_SFX_REC)

// The T-step rollout with the actor inside the launch (replaces the per-step loop MPPPO.py:245-252: policy
// inference, sampling, env.step, buffer append): one wavefront per environment for the whole episode,
// FJSP_PW_ENVS per workgroup sharing the actor's weights in LDS.  Per step: actor_probs on the current state, sample_action
// by lane 0 (the counter-based stream of fjsp_policy_sample: same seed, same actions as the per-step path),
// the environment step, the buffer row.  Finished environments idle; their rows are marked invalid.
// ORD: segment sg.seg of it.  Segment 0 runs up to the first park.  A later segment takes up only the envs the previous one
// left parked: it completes the row of the parked step (next state, reward, done: what arrival_kernel wrote to
// io.state_last, sg.reward, sg.done) and goes on at the step after it.  A wave that reaches T has written every row of its
// env (filler rows included) and clears its parked flag.
template <int KC, int V>
__global__ __launch_bounds__(FJSP_PW_THREADS) void FJSP_K(rollout_policy)(DevBatch b, ActorParams ap, PolicyRolloutIO io FJSP_SEG_ARG(PolicySegment sg), const double *mo, int T FJSP_REC_ARG) {
    constexpr bool REC = FJSP_REC != 0, ORD = FJSP_ORD != 0;
    FJSP_REC_LOCAL
    FJSP_SEG_LOCAL(PolicySegment sg)
    float *lds = reinterpret_cast<float *>(fjsp_lds);
    actor_lds_fill(lds, ap, (int)threadIdx.x, (int)blockDim.x);
    __syncthreads();                                   // (the only workgroup barrier: waves may leave after it)
    const int wave = uni((int)(threadIdx.x >> 6));
    const int env = blockIdx.x * FJSP_PW_ENVS + wave;
    if (env >= b.N) return;
    const bool resumed = ORD && sg.seg > 0;
    if constexpr (ORD)
        if (resumed && uni((int)sg.parked[env]) == 0) return;      // (its rows were finished by an earlier segment)
    const int t0 = resumed ? uni(sg.next_t[env]) : 0;
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
    const double *x_in = resumed ? io.state_last : io.state_in;
    const float x0 = w.lane < S ? (float)x_in[(size_t)env * S + w.lane] : 0.0f;
    if (w.lane < S) xs[w.lane] = x0;
    if constexpr (ORD) {
        if (resumed) {
            const size_t row = (size_t)(t0 - 1) * N + env;          // the parked step: its other columns were written at the park
            if (w.lane < S) io.o_next[row * S + w.lane] = x0;
            if (w.lane == 0) { io.o_reward[row] = (float)sg.reward[env]; io.o_done[row] = (float)sg.done[env]; }
        }
    }
    const float eps = io.epsilon[0];
    const uint64_t seed = io.seed[0];
    const double *mo_e = mo ? mo + (size_t)env * 4 : nullptr;
    wave_sync();
    for (int t = t0; t < T; ++t) {
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
        // (the row's stores keep each build's own order: the single-order kernels' code depends on it)
        if constexpr (ORD) {
            if (w.lane == 0) {
                io.o_actions[row * 2] = (float)a0; io.o_actions[row * 2 + 1] = (float)a1; io.o_valid[row] = 1.0f;
                io.o_flat[row] = (float)action; io.o_logp[row] = logp;
            }
            if (w.pending) {             // an order arrived inside this step: the next segment completes the row
                if (w.lane == 0) { sg.next_t[env] = t + 1; sg.parked[env] = 1; }
                park_env<KC, V>(w, b, env, k_sel, m_sel);
                return;
            }
            if (w.lane < S) io.o_next[row * S + w.lane] = xs[w.lane];
            if (w.lane == 0) { io.o_reward[row] = (float)reward; io.o_done[row] = (float)w.done; }
        } else {
            if (w.lane < S) io.o_next[row * S + w.lane] = xs[w.lane];
            if (w.lane == 0) {
                io.o_actions[row * 2] = (float)a0; io.o_actions[row * 2 + 1] = (float)a1;
                io.o_reward[row] = (float)reward; io.o_done[row] = (float)w.done; io.o_valid[row] = 1.0f;
                io.o_flat[row] = (float)action; io.o_logp[row] = logp;
            }
        }
    }
    if constexpr (ORD)
        if (w.lane == 0) sg.parked[env] = 0;
    store_dynamic<KC, V>(w, false, false);
}

// Decoding a trained policy (fjsp_env_play_policy): every environment plays to the end of its episode with the actor
// inside the launch, as rollout_policy above but without buffer rows.  One wavefront per environment,
// FJSP_PW_ENVS per workgroup sharing the actor's weights in LDS.  Per step: actor_probs, then the action -- envs below
// n_greedy take the first index of the largest probability (torch.argmax), the others draw from the stream of fjsp_policy_sample with
// epsilon 0 (counter = step index of this call, env = local index) -- then the environment step.  Step 0 applies
// io.first instead where given.  The start observation is row state_src[env] of state_in: v(t-1) of the state vector is
// not in the env record, so a branch batch reads its source's rows through the map.  A wave leaves its loop once its env
// is done or carries an error bit; T only bounds the loop.
// ORD: segment `seg` of it.  io.steps_out is the per-env progress: segment 0 starts every env at step 0 as above; a later
// segment starts env i at step steps_out[i] from row i of io.state_last, the f64 state arrival_kernel wrote for the parked
// step (a parked step counts: its action row is written).  io.state_last / reward_last / done_last are also
// arrival_kernel's outputs, so a parked last step needs nothing more.  The sample counter stays the step index within the call.
template <int KC, int V>
__global__ __launch_bounds__(FJSP_PW_THREADS) void FJSP_K(play_policy)(DevBatch b, ActorParams ap, PolicyPlayIO io, const double *mo, int T FJSP_SEG_ARG(int seg) FJSP_REC_ARG) {
    constexpr bool REC = FJSP_REC != 0, ORD = FJSP_ORD != 0;
    FJSP_REC_LOCAL
    FJSP_SEG_LOCAL(int seg)
    float *lds = reinterpret_cast<float *>(fjsp_lds);
    actor_lds_fill(lds, ap, (int)threadIdx.x, (int)blockDim.x);
    __syncthreads();                                   // (the only workgroup barrier: waves may leave after it)
    const int wave = uni((int)(threadIdx.x >> 6));
    const int env = blockIdx.x * FJSP_PW_ENVS + wave;
    if (env >= b.N) return;
    const int S = ap.S, A = ap.A, N = b.N;
    const int src = uni(io.state_src ? io.state_src[env] : env);
    if (src < 0 || src >= io.n_state_in) {             // (refused by the host entry; an env given no start row stays put)
        if (__lane_id() == 0) io.steps_out[env] = 0;
        return;
    }
    const int t0 = seg > 0 ? uni(io.steps_out[env]) : 0;
    const uint32_t env_stride = (uint32_t)lds_bytes_per_wave(b.JP, b.MP, b.KP, false);
    unsigned char *wave_lds = fjsp_lds + ((actor_lds_floats(ap.S) * 4 + 255) & ~(size_t)255) +
                              (size_t)wave * (env_stride + (32 + kActorH + kActorAP) * 4);
    float *xs = reinterpret_cast<float *>(wave_lds + env_stride);
    float *hs = xs + 32, *ps = hs + kActorH;
    W<KC, V> w;
    open_env<KC, V>(w, &b, env, wave_lds, false, true);
    if constexpr (REC) { w.rec = rec.rec; w.rec_cap = rec.cap; }
    compute_params<KC, V>(w);
    const double *x_row = seg > 0 ? io.state_last + (size_t)env * S : io.state_in + (size_t)src * S;
    const double x0 = w.lane < S ? x_row[w.lane] : 0.0;
    if (w.lane < S) xs[w.lane] = (float)x0;
    const uint64_t seed = io.seed ? io.seed[0] : 0;
    const bool greedy = env < io.n_greedy;
    const double *mo_e = mo ? mo + (size_t)env * 4 : nullptr;
    wave_sync();
    double reward = 0.0;
    int t = t0;
    for (; t < T; ++t) {
        if (w.done || (w.status & (FJSP_ST_BAD_TASK_RULE | FJSP_ST_BAD_MACHINE_RULE | FJSP_ST_NO_EVENT))) break;
        int a0, a1;
        if (seg == 0 && t == 0 && io.first) {
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
        if constexpr (ORD) {
            if (w.pending) {         // an order arrived inside this step: arrival_kernel writes the env's last rows
                if (w.lane == 0) io.steps_out[env] = t + 1;
                park_env<KC, V>(w, b, env, k_sel, m_sel);
                return;
            }
        }
    }
    if (w.lane == 0) {
        io.steps_out[env] = t;
        io.done_last[env] = (uint8_t)w.done;
        if (t > t0) io.reward_last[env] = reward;
    }
    if (seg == 0 && t == 0 && w.lane < S) io.state_last[(size_t)env * S + w.lane] = x0;     // (an env that took no step keeps its start row)
    store_dynamic<KC, V>(w, false, false);
}

#undef FJSP_K
#undef FJSP_K_X
#undef FJSP_K_
#undef FJSP_SFX_ORD
#undef FJSP_SFX_PW
#undef FJSP_SFX_REC
#undef FJSP_SEG_ARG
#undef FJSP_SEG_LOCAL
#undef FJSP_REC_ARG
#undef FJSP_REC_LOCAL
#undef FJSP_PW_THREADS
#undef FJSP_PW_ENVS
