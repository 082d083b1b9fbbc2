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
// A move is applied while the plan is read: a reassignment is a select, a swap and a pair move (kind 4: rows u and v stand,
// v first, behind row w, u <= w < v; the swap is the pair u, u + 1, u) are one index map, position -> row, in src().
//
// fjsp_schedule_critical is the decode run backwards, on the tables decode writes: one lane per table, the same grouping,
// the same banked words -- per job and per machine "tail + duration of the latest row seen", as decode keeps ready / free.
// A forward scan finds the table's end, checks every index it supplies, and the first row that ends at the makespan; the
// backward scan writes tails and critical flags and follows one critical path in the same pass (the predecessors of the
// path's current row are the next rows of its job and on its machine that the scan meets); a last pass over the path's
// windows writes its neighbourhood as moves the decoder takes.
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
    int pu = 0x7fffffff, pw = 0, pv = 0;           // rows pu and pv stand, pv first, behind row pw (a swap: pw = pu, pv = pu + 1)
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
                if (!bad_move && kind == 2) { pu = pw = u; pv = u + 1; }
            }
        } else if (kind == 4) {
            const int dv = m_new & 0xFFFF, dw = m_new >> 16;
            bad_move = m_new < 0 || dv < 1 || dw >= dv || u < 0 || u >= cap - dv;
            if (!bad_move) bad_move = is_end(row_at(pl, u)) || is_end(row_at(pl, u + dv));
            if (!bad_move) { pu = u; pw = u + dw; pv = u + dv; }
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
        auto src = [&](int t) { return (t < pu || t > pv) ? t : (t < pw ? t + 1 : (t == pw ? pv : (t == pw + 1 ? pu : t - 1))); };
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
        if (asked == 4 && pv >= L) bad_move = true;
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

// ---- fjsp_schedule_critical: the decode run backwards, one lane per table, the same grouping and banked layout
struct CriticalArgs {
    const int32_t *table;    // i32[N][n_cand][cap][6]
    int32_t *tail;           // i32[N][n_cand][cap]
    uint8_t *flags;          // u8[N][n_cand][cap]
    int32_t *path;           // i32[N][n_cand][cap]
    int32_t *path_len;       // i32[N][n_cand]
    int32_t *moves;          // i32[N][n_cand][max_moves][3], null with max_moves = 0
    int32_t *n_moves, *skipped, *status, *makespan;   // i32[N][n_cand] each
    const uint2 *kinds;      // [n_inst][KP + 1]
    long long total;         // N * n_cand
    int n_cand, cap, max_moves;
    int G, JW;
};

struct TRow { int r, stage, n, m, begin, end; };
__device__ __forceinline__ TRow trow_at(const int32_t *tb, int t) {
    const int32_t *o = tb + (size_t)t * 6;
    return TRow{o[0], o[1], o[2], o[3], o[4], o[5]};
}

__global__ __launch_bounds__(256) void schedule_critical_kernel(DevBatch b, CriticalArgs a) {
    const int s = (int)threadIdx.x;
    const long long g = (long long)blockIdx.x * a.G + s;
    if (s >= a.G || g >= a.total) return;
    const int env = (int)(g / a.n_cand), inst = env % b.n_inst;
    const int G = a.G, JW = a.JW, MP = b.MP, cap = a.cap;

    const unsigned char *ir = b.inst + (size_t)inst * b.L.i_stride;
    const InstHeader h = *reinterpret_cast<const InstHeader *>(ir);
    const int M = h.M < MP ? h.M : MP;
    const uint2 *kinds = a.kinds + (size_t)inst * (size_t)(b.KP + 1);
    const int R = (int)kinds[0].x;
    const uint16_t *p = reinterpret_cast<const uint16_t *>(ir + b.L.i_p);

    const int32_t *tb = a.table + (size_t)g * (size_t)cap * 6;
    int32_t *tail = a.tail + (size_t)g * cap, *path = a.path + (size_t)g * cap;
    uint8_t *flags = a.flags + (size_t)g * cap;
    int32_t *mv = a.moves ? a.moves + (size_t)g * (size_t)a.max_moves * 3 : nullptr;

    // ---- forward: the table's end, every index it supplies checked, the makespan and the first row that ends there
    int st = 0, L = 0, C = 0, e0 = -1;
    TRow nxt = trow_at(tb, 0);                                           // (the next row is requested before this one is worked on)
    for (int t = 0; t < cap; ++t) {
        const TRow x = nxt;
        if ((x.r & x.stage & x.n & x.m & x.begin & x.end) == -1) break;
        if (t + 1 < cap) nxt = trow_at(tb, t + 1);
        L = t + 1;
        bool ok = x.r >= 0 && x.r < R;
        if (ok) {
            const uint2 kd = kinds[1 + x.r];
            const int jbeg = (int)(kd.x & 0xFFFFu), cnt = (int)(kd.x >> 16), koff = (int)(kd.y & 0xFFFFu), Jr = (int)(kd.y >> 16);
            ok = x.n >= 0 && x.n < cnt && jbeg + x.n < JW && x.m >= 0 && x.m < M && x.stage >= 0 && x.stage < Jr &&
                 koff + x.stage < b.KP && x.begin >= 0 && x.begin < x.end;
        }
        if (!ok) { st = 1; break; }
        if (x.end > C) { C = x.end; e0 = t; }
    }
    if (!st && L == 0) st = 2;

    int plen = 0, n_moves = 0, skipped = 0;
    if (!st) {
        // ---- backward: tail + duration of the latest row seen, per job and per machine, as decode keeps ready / free
        uint32_t *jtail = decode_lds + s;                                // of job j     at jtail[j * G]
        uint32_t *mtail = decode_lds + (size_t)JW * G + s;               // of machine m at mtail[m * G]
        for (int j = 0; j < JW; ++j) jtail[(size_t)j * G] = 0u;
        for (int m = 0; m < MP; ++m) mtail[(size_t)m * G] = 0u;
        int curj = 0, curm = 0, curb = 0;                                // the path's current row: job word, machine, begin
        bool needj = false, needm = false;                               // its job / machine predecessor is still to come
        nxt = trow_at(tb, L - 1);
        for (int t = L - 1; t >= 0; --t) {
            const TRow x = nxt;
            if (t > 0) nxt = trow_at(tb, t - 1);
            const int j = (int)(kinds[1 + x.r].x & 0xFFFFu) + x.n;
            const uint32_t tj = jtail[(size_t)j * G], tm = mtail[(size_t)x.m * G], tl = tj > tm ? tj : tm;
            jtail[(size_t)j * G] = mtail[(size_t)x.m * G] = tl + (uint32_t)(x.end - x.begin);
            uint32_t f = ((uint32_t)x.end + tl == (uint32_t)C) ? 1u : 0u;
            bool on = t == e0;
            if (!on && (needj || needm)) {
                const bool isj = needj && j == curj, ism = needm && x.m == curm;
                if (isj || ism) {
                    if (x.end == curb) { on = true; if (!isj) f |= 4u; }
                    else { if (isj) needj = false; if (ism) needm = false; }
                }
            }
            if (on) { f |= 2u; path[plen++] = t; curj = j; curm = x.m; curb = x.begin; needj = needm = true; }
            tail[t] = (int32_t)tl;
            flags[t] = (uint8_t)f;
        }

        // ---- the path's neighbourhood: its machine arcs as pair moves, then its operations on their other machines
        auto emit = [&](int kind, int u, int third) {
            if (n_moves < a.max_moves) { int32_t *o = mv + (size_t)n_moves * 3; o[0] = kind; o[1] = u; o[2] = third; }
            ++n_moves;
        };
        for (int i = 0; i + 1 < plen; ++i) {
            const int u = path[i + 1], v = path[i];
            if (!(flags[u] & 4u)) continue;
            const int ra = tb[(size_t)u * 6], na = tb[(size_t)u * 6 + 2], rb = tb[(size_t)v * 6], nb = tb[(size_t)v * 6 + 2];
            int w = u, first = v;                                        // last row of b's job, first row of a's job in (u, v)
            for (int t = v - 1; t > u; --t) {
                const int r = tb[(size_t)t * 6], n = tb[(size_t)t * 6 + 2];
                if (w == u && r == rb && n == nb) w = t;
                if (r == ra && n == na) first = t;
            }
            if (w < first && w - u <= 32767) emit(4, u, (v - u) | ((w - u) << 16));    // (the field stays a non-negative int)
            else ++skipped;
        }
        for (int i = 0; i < plen; ++i) {
            const int t = path[i];
            const TRow x = trow_at(tb, t);
            const uint16_t *pk = p + (size_t)((int)(kinds[1 + x.r].y & 0xFFFFu) + x.stage) * MP;
            for (int m = 0; m < M; ++m)
                if (m != x.m && pk[m] != 0) emit(1, t, m);
        }
    }
    for (int t = st ? 0 : L; t < cap; ++t) { tail[t] = -1; flags[t] = 0; }
    for (int t = plen; t < cap; ++t) path[t] = -1;
    for (int i = n_moves < a.max_moves ? n_moves : a.max_moves; i < a.max_moves; ++i) { mv[(size_t)i * 3] = 0; mv[(size_t)i * 3 + 1] = 0; mv[(size_t)i * 3 + 2] = 0; }
    a.status[g] = st;
    a.makespan[g] = st ? -1 : C;
    a.path_len[g] = plen;
    a.n_moves[g] = n_moves;
    a.skipped[g] = skipped;
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

extern "C" int fjsp_schedule_critical(fjsp_env *e, const int32_t *d_table, int32_t n_cand, int32_t *d_tail, uint8_t *d_flags, int32_t *d_path,
                                      int32_t *d_path_len, int32_t *d_moves, int32_t max_moves, int32_t *d_n_moves, int32_t *d_skipped,
                                      int32_t *d_status, int32_t *d_makespan, void *stream) {
    if (!e || !d_table || !d_tail || !d_flags || !d_path || !d_path_len || !d_n_moves || !d_skipped || !d_status || !d_makespan) {
        set_error("fjsp_schedule_critical: null env, table or output pointer"); return FJSP_E_ARG;
    }
    if (n_cand < 1 || max_moves < 0 || (max_moves > 0 && !d_moves)) { set_error("fjsp_schedule_critical: needs n_cand >= 1, max_moves >= 0 and d_moves with max_moves > 0"); return FJSP_E_ARG; }
    if (e->b.variant == FJSP_VARIANT_MO_DFJSP) {
        set_error("fjsp_schedule_critical: MO_DFJSP batches are not decoded (breakdown shifts and energy)"); return FJSP_E_UNSUPPORTED;
    }
    if (e->gen_failed) { set_error("fjsp_schedule_critical: the last regenerate of this handle failed"); return FJSP_E_STATE; }
    const DevBatch &b = e->b;
    const int G = decode_group(b);
    if (G == 0) {
        set_error("fjsp_schedule_critical: a candidate's decode state (" + std::to_string(state_words(b.jcap, b.MP) * 4) + " bytes) exceeds 5120 bytes");
        return FJSP_E_UNSUPPORTED;
    }
    const long long total = (long long)b.N * (long long)n_cand;
    if (e->ops_max <= 0 || total > 0x7fffffffLL) { set_error("fjsp_schedule_critical: no operations, or more than 2^31 - 1 tables"); return FJSP_E_ARG; }
    DeviceGuard guard(e->device);
    if (!e->d_decode_kinds && !dev_alloc(e, (size_t)b.n_inst * (size_t)(b.KP + 1) * sizeof(uint2), &e->d_decode_kinds, "hipMalloc (decode kind table)")) return FJSP_E_HIP;
    hipStream_t st = (hipStream_t)stream;
    if (launch(decode_kinds_kernel, dim3((unsigned)((b.n_inst + 63) / 64)), dim3(64), 0, st, b, e->d_decode_kinds) != 0) {
        set_error("decode_kinds_kernel launch failed"); return FJSP_E_HIP;
    }
    const CriticalArgs a{d_table, d_tail, d_flags, d_path, d_path_len, max_moves > 0 ? d_moves : nullptr, d_n_moves, d_skipped, d_status, d_makespan,
                         e->d_decode_kinds, total, (int)n_cand, e->ops_max, (int)max_moves, G, b.jcap};
    const size_t lds = (size_t)(b.jcap + b.MP) * 4 * (size_t)G;
    if (launch(schedule_critical_kernel, dim3((unsigned)((total + G - 1) / G)), dim3((unsigned)(G < 64 ? 64 : G)), lds, st, b, a) != 0) {
        set_error("schedule_critical_kernel launch failed"); return FJSP_E_HIP;
    }
    return FJSP_OK;
}
