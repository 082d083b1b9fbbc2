// The row-family kernels that dispatch, included twice by fjsp_group.hip: with FJSP_REC 0 they are gstep_kernel /
// grollout_kernel, with FJSP_REC 1 their recording builds gstep_rec_kernel / grollout_rec_kernel, which also store every
// dispatch in `rec` (SchedRec, fjsp_env_record_schedule).  One text for both keeps the plain kernels' code exactly what it
// is without recording (a shared __device__ body inlined into both changes the optimiser's pass order, hence the code).
#if FJSP_REC
#define FJSP_K(name) name##_rec_kernel
#define FJSP_REC_ARG , SchedRec rec
#define FJSP_REC_LOCAL
#else
#define FJSP_K(name) name##_kernel
#define FJSP_REC_ARG
#define FJSP_REC_LOCAL const SchedRec rec{};
#endif

// One step of every environment of a group batch (fjsp_kernels.hip step_kernel for the same batch gives the same results)
// EARLY: request the gap_ave rows together with the state (small batches: a wave is alone on its SIMD and nothing else hides
// the memory round trip); otherwise they are fetched where they are used and the kernel keeps to 128 registers
template <int V, int MPC, bool EARLY>
__global__ __launch_bounds__(EARLY ? 256 : 64, EARLY ? 1 : 4) void FJSP_K(gstep)(DevBatch b, const uint8_t *actions, const double *mo, int autoreset, double *state_out,
                                                   double *reward_out, uint8_t *done_out, int16_t *trace_km FJSP_REC_ARG) {
    constexpr bool REC = FJSP_REC != 0;
    FJSP_REC_LOCAL
    GE<V> e;
    GSTAMP_DECL;
    GSTAMP_BEGIN();
    // (small batches are launched four waves to a workgroup -- a quarter of the workgroups to dispatch; the waves never meet)
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wave_id = (int)blockIdx.x * (int)(blockDim.x >> 6) + wib;
    unsigned char *const my_lds = g_lds + (size_t)wib * group_lds_bytes<MPC, EARLY>();
    // the action pair of the row's environment (2-byte aligned: checked by the host entry points)
    const int env_raw = wave_id * 4 + (int)(__lane_id() >> 4);
    const int env0 = min(env_raw, b.N - 1);
    const uint32_t araw = reinterpret_cast<const uint16_t *>(actions)[env0];
    MoW mw = {0.0, 1.0, 0.0, 0.0};
    if (V == FJSP_VARIANT_MO_FJSSP_DISCRETES && mo) {
        const double2 m01 = *reinterpret_cast<const double2 *>(mo + (size_t)env0 * 4), m23 = *reinterpret_cast<const double2 *>(mo + (size_t)env0 * 4 + 2);
        mw.w0 = m01.x; mw.w1 = m01.y; mw.cn = m23.x; mw.tn = m23.y;
    }
    GCols<MPC> cr;
    bool gap_need = false;
    g_open<V, EARLY>(e, b, wave_id, my_lds, group_rows<MPC, EARLY>(), []() {});
    if constexpr (REC) { e.rec = rec.rec; e.rec_cap = rec.cap; e.nenv = b.N; }
    gap_need = env_raw < b.N && rule_wants_gap_ave<V>(araw);
    const int a0 = (int)(araw & 0xFFu), a1 = (int)(araw >> 8);
    bool go = e.live;
    GSTAMP(0);
    if (wave_any(go && e.done != 0)) {
        const bool was_done = go && e.done != 0;
        if (autoreset == 1) g_restart<V, EARLY>(e, b, was_done);
        else {
            if (was_done && autoreset == 0) e.status |= FJSP_ST_STEP_AFTER_DONE;      // 2: idle silently
            go = go && !was_done;
        }
    }
    int k_sel = -1, m_sel = -1;
    GSTAMP(1);
    // small batches: Machine.gap_ave's operands are requested now (the machines that are idle are known), used after task_select
    if (EARLY && wave_any(gap_need && go)) g_cols_issue<V, MPC>(e, b, gap_need && go, cr);
    const double reward = g_step<V, MPC, EARLY, REC>(e, b, go, a0, a1, mw, state_out != nullptr, state_out, gap_need && go, cr, &k_sel, &m_sel GSTAMP_ARG);
    if (e.live && e.l == 0) {
        if (reward_out) reward_out[e.env] = reward;
        if (done_out) done_out[e.env] = (uint8_t)e.done;
        if (trace_km) { trace_km[(size_t)e.env * 2] = (int16_t)k_sel; trace_km[(size_t)e.env * 2 + 1] = (int16_t)m_sel; }
    }
    g_store<V>(e, b);
    GSTAMP(8);
    GSTAMP_FLUSH();
}

// T fused steps per launch with the actions given (rule sweeps): the environments live in registers for the whole
// launch.  Same outputs as fjsp_kernels.hip rollout_kernel.
template <int V, int MPC, bool EARLY>
__global__ __launch_bounds__(EARLY ? 256 : 64, EARLY ? 1 : 2) void FJSP_K(grollout)(DevBatch b, const uint8_t *actions, const double *mo, int T, int16_t *trace_km,
                                                      double *reward_out, double *state_last, int resident FJSP_REC_ARG) {
    constexpr bool REC = FJSP_REC != 0;
    FJSP_REC_LOCAL
    GE<V> e;
    GSTAMP_DECL;
    GSTAMP_BEGIN();
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wave_id = (int)blockIdx.x * (int)(blockDim.x >> 6) + wib;
    unsigned char *const my_lds = g_lds + (size_t)wib * group_lds_bytes<MPC, EARLY>();
    g_open<V, EARLY>(e, b, wave_id, my_lds, group_rows<MPC, EARLY>(), []() {});
    if constexpr (REC) { e.rec = rec.rec; e.rec_cap = rec.cap; e.nenv = b.N; }
    // (small batches, one wave to a workgroup: the static tables next to the rows, see res_bytes)
    if (!EARLY && resident) g_make_resident<V, MPC>(e, b, (uint32_t)group_lds_bytes<MPC, EARLY>() + (uint32_t)(__lane_id() >> 4) * res_bytes<MPC>());
    MoW mw = {0.0, 1.0, 0.0, 0.0};
    if (V == FJSP_VARIANT_MO_FJSSP_DISCRETES && mo) {
        mw.w0 = mo[(size_t)e.env * 4]; mw.w1 = mo[(size_t)e.env * 4 + 1]; mw.cn = mo[(size_t)e.env * 4 + 2]; mw.tn = mo[(size_t)e.env * 4 + 3];
    }
    for (int s = 0; s < T; ++s) {
        const size_t o = (size_t)s * b.N + e.env;
        const bool go = e.live && !e.done && !(e.status & (FJSP_ST_BAD_TASK_RULE | FJSP_ST_BAD_MACHINE_RULE | FJSP_ST_NO_EVENT));
        if (!wave_any(go)) {
            if (e.live && e.l == 0) {
                if (trace_km) { trace_km[o * 2] = -1; trace_km[o * 2 + 1] = -1; }
                if (reward_out) reward_out[o] = 0.0;
            }
            continue;
        }
        const uint32_t araw = reinterpret_cast<const uint16_t *>(actions)[o];
        const bool gap_need = go && rule_wants_gap_ave<V>(araw);
        GCols<MPC> cr;
        if (EARLY) g_cols_issue<V, MPC>(e, b, gap_need, cr);
        int k_sel = -1, m_sel = -1;
        const double reward = g_step<V, MPC, EARLY, REC>(e, b, go, (int)(araw & 0xFFu), (int)(araw >> 8), mw, state_last != nullptr, state_last,
                                             gap_need, cr, &k_sel, &m_sel GSTAMP_ARG);
        if (e.live && e.l == 0) {
            if (trace_km) { trace_km[o * 2] = (int16_t)k_sel; trace_km[o * 2 + 1] = (int16_t)m_sel; }
            if (reward_out) reward_out[o] = reward;
        }
    }
    g_store<V>(e, b);
}

#undef FJSP_K
#undef FJSP_REC_ARG
#undef FJSP_REC_LOCAL
