// Explicit schedules decoded on the device (fjsp_schedule_decode; schedule.decode, policy_search.improve): an operation
// sequence with a machine per operation -> the times the reference's dispatch gives it (SO_FJSSP.py:176-196: time_begin =
// the later of the job's and the machine's release, time_end = time_begin + time_mrj_dict) and the two objectives, with
// the jobs released at their order's arrival and numbered as class_FJSSP.py:212-218 numbers them.
//
// One candidate is a strictly sequential chain of L operations; candidates are independent.  So ONE LANE owns one
// candidate.  Its state -- ready[jobs] (i32), the jobs' next stage (u8) and free[M] (i32) -- lives in LDS, word w of the
// candidate in slot s of the workgroup at word w * G + s, G = the candidates of a workgroup, a multiple of 32: the 32
// lanes that one LDS cycle of a 4-byte (or 1-byte) access serves then sit on 32 different banks whatever job or machine
// each of them addresses.  G is the largest of 256, 128, 64 whose state fits 64 KB (two or more workgroups to a CU), else
// 64 or 32 within the CU's 160 KB (decode_group); with G = 32 the upper half of the one wave idles.  Candidate g = env *
// n_cand + q sits in slot g % G of workgroup g / G: the candidates of one env are neighbours, so the rows of a shared
// parent plan are one address to the wave.
//
// Per row a lane loads the row (12 bytes; the next row is requested before this one is worked on), the kind's entry of
// the kind table (8 bytes: first job | jobs, first operation type | stages), p[k][m] (2 bytes) and, at a job's last
// stage, its due date.  The kind table, r -> those two words and in front of them (kinds, operations) of the instance, is
// what the instance record lacks (it is indexed by operation type and by job); decode_kinds_kernel rebuilds it from the
// record in front of every decode, stream-ordered, so a regenerated handle needs no bookkeeping.
//
// Nothing is left to fault: every index a plan or a move supplies is range-checked before it is used, a candidate that
// fails a check keeps reading rows only to find the plan's end (a move outside the plan outranks the other codes) and
// its outputs are -1.  No atomics, no barriers; the outputs are a function of the inputs alone.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/fjsp_amd.h"
#include "fjsp_env_impl.h"
#include "fjsp_launch.h"

namespace {
using namespace fjsp;

constexpr size_t kLdsTwo = 64 * 1024, kLdsCu = 160 * 1024;

struct DecodeArgs {
    const int32_t *plan;     // i32[N][q_plans][cap][3]
    const int32_t *moves;    // i32[N][n_cand][3], nullable
    int64_t *objective;      // i64[N][n_cand][2]
    int32_t *status;         // i32[N][n_cand]
    int32_t *table;          // i32[N][n_cand][cap][6], nullable
    int32_t *len;            // i32[N][n_cand], nullable
    const uint2 *kinds;      // [n_inst][KP + 1]
    long long total;         // N * n_cand
    int n_cand, q_plans, cap;
    int G, JW;               // candidates per workgroup; job words of a candidate (DevBatch::jcap)
};

// words of one candidate's state: ready[JW], the stage bytes of four jobs to a word, free[MP]
__host__ __device__ inline int state_words(int JW, int MP) { return JW + JW / 4 + MP; }

// entry 0: (kinds, operations of the instance); entry 1 + r: (first job | jobs << 16, first operation type | stages << 16)
__global__ __launch_bounds__(64) void decode_kinds_kernel(DevBatch b, uint2 *kinds) {
    const int inst = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (inst >= b.n_inst) return;
    const InstHeader h = *inst_ptr<const InstHeader>(b, inst, 0);
    const uint32_t *kA = inst_ptr<const uint32_t>(b, inst, b.L.i_kA), *kB = inst_ptr<const uint32_t>(b, inst, b.L.i_kB);
    uint2 *out = kinds + (size_t)inst * (size_t)(b.KP + 1);
    const int K = h.K < b.KP ? h.K : b.KP;
    uint32_t ops = 0;
    for (int k = 0; k < K; ++k) {
        const uint32_t kb = kB[k];
        if ((kb & 0xFFu) != 0) continue;                     // stage 0 of its kind only
        const uint32_t r = (kb >> 16) & 0xFFu, Jr = (kb >> 8) & 0xFFu, ka = kA[k];
        if ((int)r < b.KP) out[1 + r] = make_uint2(ka, (uint32_t)k | (Jr << 16));
        ops += (ka >> 16) * Jr;
    }
    const uint32_t R = (uint32_t)h.R & 0xFFFFu;
    out[0] = make_uint2(R < (uint32_t)b.KP ? R : (uint32_t)b.KP, ops);
}

struct Row { int r, n, m; };
__device__ __forceinline__ bool is_end(const Row &x) { return x.r == -1 && x.n == -1 && x.m == -1; }
__device__ __forceinline__ Row row_at(const int32_t *pl, int idx) { return Row{pl[3 * idx], pl[3 * idx + 1], pl[3 * idx + 2]}; }

extern __shared__ __attribute__((aligned(16))) uint32_t decode_lds[];

__global__ __launch_bounds__(256) void schedule_decode_kernel(DevBatch b, DecodeArgs a) {
    const int s = (int)threadIdx.x;
    const long long g = (long long)blockIdx.x * a.G + s;
    if (s >= a.G || g >= a.total) return;
    const int env = (int)(g / a.n_cand), q = (int)(g - (long long)env * a.n_cand), inst = env % b.n_inst;
    const int G = a.G, JW = a.JW, MP = b.MP, cap = a.cap;

    const unsigned char *ir = b.inst + (size_t)inst * b.L.i_stride;
    const InstHeader h = *reinterpret_cast<const InstHeader *>(ir);
    const int M = h.M < MP ? h.M : MP;
    const int S = b.mord ? min(h.R >> 16, b.SP) : 1;
    const uint2 *kinds = a.kinds + (size_t)inst * (size_t)(b.KP + 1);
    const int R = (int)kinds[0].x, ops = (int)kinds[0].y;
    const uint16_t *p = reinterpret_cast<const uint16_t *>(ir + b.L.i_p);
    const int32_t *due = reinterpret_cast<const int32_t *>(ir + b.L.i_due);

    uint32_t *ready = decode_lds + s;                                    // ready[j]  at ready[j * G]
    uint8_t *stage = reinterpret_cast<uint8_t *>(decode_lds + (size_t)JW * G + s);   // stage[j] at stage[(j >> 2) * 4 G + (j & 3)]
    uint32_t *mfree = decode_lds + (size_t)(JW + JW / 4) * G + s;        // free[m]   at mfree[m * G]

    // ---- the move, checked against the plan before anything is decoded
    const int32_t *pl = a.plan + ((size_t)env * a.q_plans + (a.q_plans == 1 ? 0 : q)) * (size_t)cap * 3;
    int kind = 0, asked = 0, u = 0, m_new = 0;     // asked: the move's kind as given (kind drops to 0 for a swap within a job)
    bool bad_move = false;
    if (a.moves) {
        const int32_t *mv = a.moves + (size_t)g * 3;
        kind = asked = mv[0]; u = mv[1]; m_new = mv[2];
        if (kind == 1) {
            bad_move = u < 0 || u >= cap || is_end(row_at(pl, u));
        } else if (kind == 2) {
            bad_move = u < 0 || u >= cap - 1;
            if (!bad_move) {
                const Row x = row_at(pl, u), y = row_at(pl, u + 1);
                bad_move = is_end(x) || is_end(y);
                if (!bad_move && x.r == y.r && x.n == y.n) kind = 0;     // two rows of one job: nothing changes
            }
        } else if (kind != 0) {
            bad_move = true;
        }
    }

    int err = 0, L = 0;
    long long makespan = 0, tard = 0;
    int32_t *tab = a.table ? a.table + (size_t)g * (size_t)cap * 6 : nullptr;
    if (!bad_move) {
        // ---- the candidate's state: jobs released at their order's arrival, machines free at 0
        const int32_t *oarr = reinterpret_cast<const int32_t *>(ir + b.L.i_oarr);
        const uint16_t *ocnt = reinterpret_cast<const uint16_t *>(ir + b.L.i_ocnt);
        for (int w = 0; w < JW / 4; ++w) decode_lds[(size_t)(JW + w) * G + s] = 0u;
        for (int m = 0; m < MP; ++m) mfree[(size_t)m * G] = 0u;
        for (int r = 0; r < R; ++r) {
            const uint32_t ka = kinds[1 + r].x;
            const int jbeg = (int)(ka & 0xFFFFu), cnt = (int)(ka >> 16);
            int n = 0;
            for (int so = 0; so < S; ++so) {
                const int arr = oarr[so];
                for (int c = (int)ocnt[(size_t)so * b.RP + r]; c > 0 && n < cnt && jbeg + n < JW; --c, ++n) ready[(size_t)(jbeg + n) * G] = (uint32_t)arr;
            }
        }

        // ---- row by row; position t of the moved plan is row src(t) of the plan
        const int u2 = kind == 2 ? u : -2;
        auto src = [&](int t) { return t == u2 ? t + 1 : (t == u2 + 1 ? t - 1 : t); };
        Row nxt = row_at(pl, src(0));
        for (int t = 0; t < cap; ++t) {
            Row x = nxt;
            if (is_end(x)) break;
            if (t + 1 < cap) nxt = row_at(pl, src(t + 1));
            L = t + 1;
            if (err) continue;                                           // only the plan's end is still of interest
            if (kind == 1 && t == u) x.m = m_new;
            if (x.r < 0 || x.r >= R) { err = 1; continue; }
            const uint2 kd = kinds[1 + x.r];
            const int jbeg = (int)(kd.x & 0xFFFFu), cnt = (int)(kd.x >> 16), koff = (int)(kd.y & 0xFFFFu), Jr = (int)(kd.y >> 16);
            if (x.n < 0 || x.n >= cnt || jbeg + x.n >= JW) { err = 1; continue; }
            const int j = jbeg + x.n;
            uint8_t *sj = stage + (size_t)(j >> 2) * 4 * G + (j & 3);
            const int stg = (int)*sj;
            if (stg >= Jr || koff + stg >= b.KP) { err = 2; continue; }
            if (x.m < 0 || x.m >= M) { err = 3; continue; }
            const int pv = (int)p[(size_t)(koff + stg) * MP + x.m];
            if (pv == 0) { err = 3; continue; }
            const int begin = max((int)ready[(size_t)j * G], (int)mfree[(size_t)x.m * G]), end = begin + pv;
            ready[(size_t)j * G] = (uint32_t)end;
            mfree[(size_t)x.m * G] = (uint32_t)end;
            *sj = (uint8_t)(stg + 1);
            makespan = max(makespan, (long long)end);
            if (stg == Jr - 1) tard += max(0LL, (long long)end - (long long)due[j]);
            if (tab) {
                int32_t *o = tab + (size_t)t * 6;
                o[0] = x.r; o[1] = stg; o[2] = x.n; o[3] = x.m; o[4] = begin; o[5] = end;
            }
        }
        if (!err && L != ops) err = 2;                                   // operations missing
        // a plan with rows behind its first -1 row can have let a move past the checks above
        if (asked == 1 && u >= L) bad_move = true;
        if (asked == 2 && u + 1 >= L) bad_move = true;
    }
    const int st = bad_move ? 4 : err;
    a.status[g] = st;
    a.objective[2 * g] = st ? -1 : makespan;
    a.objective[2 * g + 1] = st ? -1 : tard;
    if (a.len) a.len[g] = st ? 0 : L;
    if (tab) {
        for (int t = st ? 0 : L; t < cap; ++t) {
            int32_t *o = tab + (size_t)t * 6;
            o[0] = -1; o[1] = -1; o[2] = -1; o[3] = -1; o[4] = -1; o[5] = -1;
        }
    }
}

// candidates per workgroup, 0 = the state of 32 candidates does not fit the LDS of a CU
int decode_group(const DevBatch &b) {
    const size_t bytes = (size_t)state_words(b.jcap, b.MP) * 4;
    for (int G = 256; G >= 64; G >>= 1)
        if (G * bytes <= kLdsTwo) return G;
    if (64 * bytes <= kLdsCu) return 64;
    return 32 * bytes <= kLdsCu ? 32 : 0;
}

}  // namespace

extern "C" int fjsp_schedule_decode_capacity(const fjsp_env *e) { return e ? e->ops_max : 0; }

extern "C" int fjsp_schedule_decode_group(const fjsp_env *e) {
    return (e && e->b.variant != FJSP_VARIANT_MO_DFJSP) ? decode_group(e->b) : 0;
}

extern "C" int fjsp_schedule_decode(fjsp_env *e, const int32_t *d_plan, int32_t q_plans, const int32_t *d_moves, int32_t n_cand,
                                    int64_t *d_objective, int32_t *d_status, int32_t *d_table, int32_t *d_len, void *stream) {
    if (!e || !d_plan || !d_objective || !d_status) { set_error("fjsp_schedule_decode: null env, plan, objective or status pointer"); return FJSP_E_ARG; }
    if (n_cand < 1 || (q_plans != 1 && q_plans != n_cand)) { set_error("fjsp_schedule_decode: needs n_cand >= 1 and q_plans = 1 or n_cand"); return FJSP_E_ARG; }
    if (e->b.variant == FJSP_VARIANT_MO_DFJSP) {
        set_error("fjsp_schedule_decode: MO_DFJSP batches are not decoded (breakdown shifts and energy)"); return FJSP_E_UNSUPPORTED;
    }
    if (e->gen_failed) { set_error("fjsp_schedule_decode: the last regenerate of this handle failed"); return FJSP_E_STATE; }
    const DevBatch &b = e->b;
    const int G = decode_group(b);
    if (G == 0) {
        set_error("fjsp_schedule_decode: a candidate's state (5 bytes per job of the largest instance, rounded up to 16 jobs, + 4 per machine: " +
                  std::to_string(state_words(b.jcap, b.MP) * 4) + " bytes) exceeds 5120 bytes");
        return FJSP_E_UNSUPPORTED;
    }
    const long long total = (long long)b.N * (long long)n_cand;
    if (e->ops_max <= 0 || total > 0x7fffffffLL) { set_error("fjsp_schedule_decode: no operations, or more than 2^31 - 1 candidates"); return FJSP_E_ARG; }
    DeviceGuard guard(e->device);
    if (!e->d_decode_kinds && !dev_alloc(e, (size_t)b.n_inst * (size_t)(b.KP + 1) * sizeof(uint2), &e->d_decode_kinds, "hipMalloc (decode kind table)")) return FJSP_E_HIP;
    hipStream_t st = (hipStream_t)stream;
    if (launch(decode_kinds_kernel, dim3((unsigned)((b.n_inst + 63) / 64)), dim3(64), 0, st, b, e->d_decode_kinds) != 0) {
        set_error("decode_kinds_kernel launch failed"); return FJSP_E_HIP;
    }
    const DecodeArgs a{d_plan, d_moves, d_objective, d_status, d_table, d_len, e->d_decode_kinds, total, (int)n_cand, (int)q_plans, e->ops_max, G, b.jcap};
    const size_t lds = (size_t)state_words(b.jcap, b.MP) * 4 * (size_t)G;
    if (launch(schedule_decode_kernel, dim3((unsigned)((total + G - 1) / G)), dim3((unsigned)(G < 64 ? 64 : G)), lds, st, b, a) != 0) {
        set_error("schedule_decode_kernel launch failed"); return FJSP_E_HIP;
    }
    return FJSP_OK;
}
