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
// v first, behind row w, u <= w < v; the swap is the pair u, u + 1, u) are one index map, position -> row, in move_src().
//
// fjsp_schedule_decode_dyn is the same kernel text compiled with DYN for MO_DFJSP handles (schedule_decode_dyn_kernel): per
// row the lane also gathers the machine's window range and walks its windows, power[k][m] and the machine's idle power, and
// keeps one more banked word per machine, the end of its last task; free[m] is the machine's end there and the objective
// has a third entry, energy.  The three kernels without DYN compile to what they compiled to before the switch.
//
// fjsp_schedule_decode_active is the plain kernel text once more with a placement policy (Gaps, at its definition): a row
// goes into the earliest idle interval of its machine that fits, the intervals of a candidate in a workspace of the handle,
// a bounded grid whose workgroups loop over the call's groups (schedule_decode_active_kernel).  The kernels without the
// policy compile to what they compiled to before it.
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
//
// fjsp_schedule_search runs hill climbing and tabu search over those two: one wavefront per env, all rounds in one launch,
// built from the same device functions (its own head comment is at schedule_search_kernel; its barriers are those of a
// one-wave workgroup around its LDS plan).  fjsp_schedule_search_dyn is that kernel text compiled with DYN for MO_DFJSP
// handles (schedule_search_kernel<true>): the uniform neighbourhood only, every decode decode_plan<true>, three objectives.
// fjsp_schedule_search_front is the same text once more, for both families (schedule_search_kernel<DYN, FrontArgs>): the
// uniform neighbourhood, the selection by a weighted sum of the objectives, and per env the Pareto archive of every vector
// the search decodes, kept in LDS by the wave (ballots and prefix counts; no atomics).
//
// fjsp_schedule_evolve is a genetic algorithm on those decodes (its head comment is at EvolveArgs); fjsp_schedule_evolve_active
// is its text with Gaps in every decode, on decode_active's workspace and bounded grid (schedule_evolve_active_kernel).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/fjsp_amd.h"
#include "fjsp_env_impl.h"
#include "fjsp_gen_stream.h"
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

// BW of the MO_DFJSP kernels: the windows from i_bk to the record's end -- no window index reaches past the record, whatever
// i_bkoff holds
__host__ __device__ inline int dyn_windows(const DevBatch &b) { return (int)((b.L.i_stride - b.L.i_bk) / 8); }

// words of one candidate's state: ready[JW], the stage bytes of four jobs to a word, free[MP]
__host__ __device__ inline int state_words(int JW, int MP) { return JW + JW / 4 + MP; }
// the MO_DFJSP decode keeps one more word per machine behind them (the end of its last task)
__host__ __device__ inline int dyn_state_words(int JW, int MP) { return state_words(JW, MP) + MP; }

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

// ---- the texts that schedule_decode_kernel, schedule_critical_kernel and schedule_search_kernel share: the instance as
// they read it, a candidate's banked state, the index map of a move, the decode of a plan row by row, the forward and the
// backward scan of a table with the move list.  Plans and tables come through accessors (index -> row), so that the same
// text reads them from global memory (the first two kernels) and from LDS (the search); every function inlines, and the
// pointers keep their address space.
struct Shop {
    const unsigned char *ir;
    const uint2 *kinds;      // the instance's kind table
    const uint16_t *p;
    const int32_t *due;
    int R, ops, M, MP, KP, JW, S;
};
__device__ __forceinline__ Shop shop_of(const DevBatch &b, const uint2 *kind_table, int inst, int JW) {
    Shop sh;
    sh.ir = b.inst + (size_t)inst * b.L.i_stride;
    const InstHeader h = *reinterpret_cast<const InstHeader *>(sh.ir);
    sh.MP = b.MP; sh.KP = b.KP; sh.JW = JW;
    sh.M = h.M < b.MP ? h.M : b.MP;
    sh.S = b.mord ? min(h.R >> 16, b.SP) : 1;
    sh.kinds = kind_table + (size_t)inst * (size_t)(b.KP + 1);
    sh.R = (int)sh.kinds[0].x; sh.ops = (int)sh.kinds[0].y;
    sh.p = reinterpret_cast<const uint16_t *>(sh.ir + b.L.i_p);
    sh.due = reinterpret_cast<const int32_t *>(sh.ir + b.L.i_due);
    return sh;
}

// slot s of a workgroup of G candidates: ready[j] at ready[j * G], stage[j] at stage[(j >> 2) * 4 G + (j & 3)] (its words
// at words[w * G]), free[m] at mfree[m * G]
struct State { uint32_t *ready, *words, *mfree; uint8_t *stage; int G; };
__device__ __forceinline__ State state_at(uint32_t *lds, int s, int G, int JW) {
    return State{lds + s, lds + (size_t)JW * G + s, lds + (size_t)(JW + JW / 4) * G + s, reinterpret_cast<uint8_t *>(lds + (size_t)JW * G + s), G};
}

// A move checked against its plan (row: index -> Row, an end row past the plan).  kind drops to 0 for a swap within a job,
// asked keeps it; rows pu and pv stand, pv first, behind row pw (a swap: pw = pu, pv = pu + 1).
struct Move { int kind, asked, u, m_new, pu, pw, pv; bool bad; };
__device__ __forceinline__ Move no_move() { return Move{0, 0, 0, 0, 0x7fffffff, 0, 0, false}; }
template <class RowAt>
__device__ __forceinline__ Move move_of(int kind, int u, int m_new, int cap, RowAt row) {
    Move mv{kind, kind, u, m_new, 0x7fffffff, 0, 0, false};
    if (kind == 1) {
        mv.bad = u < 0 || u >= cap || is_end(row(u));
    } else if (kind == 2) {
        mv.bad = u < 0 || u >= cap - 1;
        if (!mv.bad) {
            const Row x = row(u), y = row(u + 1);
            mv.bad = is_end(x) || is_end(y);
            if (!mv.bad && x.r == y.r && x.n == y.n) mv.kind = 0;        // two rows of one job: nothing changes
            if (!mv.bad && mv.kind == 2) { mv.pu = mv.pw = u; mv.pv = u + 1; }
        }
    } else if (kind == 4) {
        const int dv = m_new & 0xFFFF, dw = m_new >> 16;
        mv.bad = m_new < 0 || dv < 1 || dw >= dv || u < 0 || u >= cap - dv;
        if (!mv.bad) mv.bad = is_end(row(u)) || is_end(row(u + dv));
        if (!mv.bad) { mv.pu = u; mv.pw = u + dw; mv.pv = u + dv; }
    } else if (kind != 0) {
        mv.bad = true;
    }
    return mv;
}
// position t of the moved plan is row move_src(mv, t) of the plan
__device__ __forceinline__ int move_src(const Move &mv, int t) {
    return (t < mv.pu || t > mv.pv) ? t : (t < mv.pw ? t + 1 : (t == mv.pw ? mv.pv : (t == mv.pw + 1 ? mv.pu : t - 1)));
}
// a plan with rows behind its first -1 row can have let a move past the checks of move_of: L is the plan's length
__device__ __forceinline__ bool move_past(const Move &mv, int L) {
    return (mv.asked == 1 && mv.u >= L) || (mv.asked == 2 && mv.u + 1 >= L) || (mv.asked == 4 && mv.pv >= L);
}

// What a decoded row adds to its table: stage, operation type, times
struct Step { int stg, k, begin, end; };

// What the MO_DFJSP decode (fjsp_schedule_decode_dyn) reads and keeps beside Shop and State: power and idle power, the
// machines' breakdown windows (machine m's are windows bkoff[m] .. bkoff[m + 1] - 1, file order; BW = the windows a record
// has room for) and, behind free[MP] in the banked state, the end of every machine's last task (-1: none, as e_dyn keeps it)
struct DynShop {
    const uint16_t *pw, *bkoff;
    const int32_t *ipw;
    const int2 *bk;
    uint32_t *mlast;
    int BW;
};
__device__ __forceinline__ DynShop dyn_shop_of(const DevBatch &b, const Shop &sh, const State &st, int BW) {
    return DynShop{reinterpret_cast<const uint16_t *>(sh.ir + b.L.i_pw), reinterpret_cast<const uint16_t *>(sh.ir + b.L.i_bkoff),
                   reinterpret_cast<const int32_t *>(sh.ir + b.L.i_ipw), reinterpret_cast<const int2 *>(sh.ir + b.L.i_bk),
                   st.mfree + (size_t)sh.MP * st.G, BW};
}

// The decode of one plan under one move on the state `st`: jobs released at their order's arrival, machines free at 0,
// then row by row.  Returns the status of the rows (0, 1, 2, 3), L = the plan's length whatever the status (a candidate
// that fails a check keeps reading rows only to find the plan's end); sink(t, row, step) sees every decoded row.
// DYN (MO_DFJSP_breakdown.py:203-256 without the event clock; the contract is at fjsp_schedule_decode_dyn): the dispatch
// time t0 = max(ready, free) is shifted by the machine's windows, walked from the first in file order at every row as the
// reference walks them; free[m] and ready[job] become the MACHINE's end, which a window that starts exactly at the task's
// end moves on its own; *energy gathers power x duration and idle power x the gap from the last task's end to t0.
// fix(t, row, operation type), which only fjsp_schedule_evolve passes, may put row t on another machine once its stage is
// known and before its machine is checked; the callers that do not pass it compile to what they compiled to without it.
// gaps, which only fjsp_schedule_decode_active passes (Gaps, below; the caller's object, which counts), places a row in the
// earliest idle interval of its machine in place of max(ready, free): free[m] is then the policy's word (the machine's
// latest interval), not a clock.
struct NoFix { __device__ __forceinline__ void operator()(int, Row &, int) const {} };
struct NoGaps { static constexpr bool on = false; };
template <bool DYN = false, class RowAt, class Sink, class Fix = NoFix, class Place = NoGaps>
__device__ __forceinline__ int decode_plan(const DevBatch &b, const Shop &sh, const State &st, RowAt row, int cap, const Move &mv, Sink sink,
                                           int &L, long long &makespan, long long &tard, const DynShop *dy = nullptr, long long *energy = nullptr,
                                           Fix fix = Fix{}, Place *gaps = nullptr) {
    const int G = st.G, JW = sh.JW, MP = sh.MP;
    const int32_t *oarr = reinterpret_cast<const int32_t *>(sh.ir + b.L.i_oarr);
    const uint16_t *ocnt = reinterpret_cast<const uint16_t *>(sh.ir + b.L.i_ocnt);
    for (int w = 0; w < JW / 4; ++w) st.words[(size_t)w * G] = 0u;
    for (int m = 0; m < MP; ++m) st.mfree[(size_t)m * G] = 0u;
    if constexpr (DYN) {
        for (int m = 0; m < MP; ++m) dy->mlast[(size_t)m * G] = 0xFFFFFFFFu;
        *energy = 0;
    }
    for (int r = 0; r < sh.R; ++r) {
        const uint32_t ka = sh.kinds[1 + r].x;
        const int jbeg = (int)(ka & 0xFFFFu), cnt = (int)(ka >> 16);
        int n = 0;
        for (int so = 0; so < sh.S; ++so) {
            const int arr = oarr[so];
            for (int c = (int)ocnt[(size_t)so * b.RP + r]; c > 0 && n < cnt && jbeg + n < JW; --c, ++n) st.ready[(size_t)(jbeg + n) * G] = (uint32_t)arr;
        }
    }
    int err = 0;
    L = 0; makespan = 0; tard = 0;
    Row nxt = row(move_src(mv, 0));
    for (int t = 0; t < cap; ++t) {
        Row x = nxt;
        if (is_end(x)) break;
        if (t + 1 < cap) nxt = row(move_src(mv, t + 1));                 // (the next row is requested before this one is worked on)
        L = t + 1;
        if (err) continue;                                               // only the plan's end is still of interest
        if (mv.kind == 1 && t == mv.u) x.m = mv.m_new;
        if (x.r < 0 || x.r >= sh.R) { err = 1; continue; }
        const uint2 kd = sh.kinds[1 + x.r];
        const int jbeg = (int)(kd.x & 0xFFFFu), cnt = (int)(kd.x >> 16), koff = (int)(kd.y & 0xFFFFu), Jr = (int)(kd.y >> 16);
        if (x.n < 0 || x.n >= cnt || jbeg + x.n >= JW) { err = 1; continue; }
        const int j = jbeg + x.n;
        uint8_t *sj = st.stage + (size_t)(j >> 2) * 4 * G + (j & 3);
        const int stg = (int)*sj;
        if (stg >= Jr || koff + stg >= sh.KP) { err = 2; continue; }
        fix(t, x, koff + stg);
        if (x.m < 0 || x.m >= sh.M) { err = 3; continue; }
        const int pv = (int)sh.p[(size_t)(koff + stg) * MP + x.m];
        if (pv == 0) { err = 3; continue; }
        int begin;
        if constexpr (Place::on) begin = gaps->place(t, (int)st.ready[(size_t)j * G], pv, st.mfree + (size_t)x.m * G);
        else begin = max((int)st.ready[(size_t)j * G], (int)st.mfree[(size_t)x.m * G]);
        int end = begin + pv;
        if constexpr (DYN) {
            const int t0 = begin;
            int mend = end;
            const int q1 = min((int)dy->bkoff[x.m + 1], dy->BW);                  // (x.m + 1 <= MP; no window index past the record)
            for (int q = (int)dy->bkoff[x.m]; q < q1; ++q) {
                const int2 w = dy->bk[q];
                if (w.x <= t0 && t0 < w.y) { begin += w.y - t0; end += w.y - t0; mend = end; }
                else if (t0 < w.x && w.x < end) { end += w.y - w.x; mend = end; }
                else if (w.x == end) mend += w.y - w.x;
                else if (w.x > end) break;
            }
            *energy += (long long)dy->pw[(size_t)(koff + stg) * MP + x.m] * (long long)pv;
            const int last = (int)dy->mlast[(size_t)x.m * G];
            if (last >= 0) *energy += (long long)(t0 - last) * (long long)dy->ipw[x.m];
            dy->mlast[(size_t)x.m * G] = (uint32_t)end;
            st.ready[(size_t)j * G] = (uint32_t)mend;
            st.mfree[(size_t)x.m * G] = (uint32_t)mend;
        } else {
            st.ready[(size_t)j * G] = (uint32_t)end;
            if constexpr (!Place::on) st.mfree[(size_t)x.m * G] = (uint32_t)end;
        }
        *sj = (uint8_t)(stg + 1);
        makespan = max(makespan, (long long)end);
        if (stg == Jr - 1) tard += max(0LL, (long long)end - (long long)sh.due[j]);
        sink(t, x, Step{stg, koff + stg, begin, end});
    }
    if (!err && L != sh.ops) err = 2;                                    // operations missing
    return err;
}

// ---- fjsp_schedule_decode_active: insertion into machine gaps.  A candidate keeps the busy intervals of its machines in
// global memory, one entry per decoded row: entry t (the row at plan position t) is the pair (begin, duration | pred <<
// 16), pred = the entry in front of it on its machine, 1-based, 0 = none (a plan has at most 65535 rows and p is 16 bits
// wide, fjsp_env_create).  The chain of a machine is followed from its LATEST interval, which free[m]'s word holds
// (1-based, 0 = an idle machine: what decode_plan initialises it to): the contract walks the intervals from the first and
// takes the first gap that fits; the intervals of a machine are disjoint, so their ends ascend with their begins, gap i
// (behind interval i, in front of interval i + 1) fits iff max(s, e_i) + d <= b_{i + 1}, and no gap in front of an
// interval that ends at or before s can fit -- so the walk from the back, down to the first such interval, that keeps
// the LOWEST gap that fits finds the same one, and is as long as the intervals that end after the job is ready, not as
// the machine's whole list.  Entry i of the candidate in slot s of workgroup w is ws[(w * cap + i) * G + s]: the lanes of
// a wave that touch entry i of their candidates read one 8-byte word each at consecutive addresses.  A lane reads only
// entries it reaches from a tail word that it reset itself, and each of those it wrote in this decode: what an earlier
// candidate left in the slot is never looked at, and the workspace needs no clearing between candidates, groups or calls.
struct Gaps {
    static constexpr bool on = true;
    uint2 *ws;               // entry 0 of this lane's slot
    int G;
    int inserted;            // rows placed in front of an interval
    __device__ __forceinline__ int place(int t, int s, int d, uint32_t *tail) {
        uint32_t cur = *tail, succ = 0, succ_y = 0, at_pred = cur, at_succ = 0, at_succ_y = 0;
        int nb = 0x7fffffff, start = s;                                  // begin of the interval behind the gap looked at
        for (int n = 0; n <= t; ++n) {                                   // (a chain holds at most the t rows decoded so far)
            const uint2 x = cur ? ws[(size_t)(cur - 1) * G] : make_uint2(0u, 0u);
            const int e = cur ? (int)(x.x + (x.y & 0xFFFFu)) : s;
            const int at = max(s, e);
            if (at + d <= nb) { start = at; at_pred = cur; at_succ = succ; at_succ_y = succ_y; }
            if (e <= s) break;                                           // (the front of the list included)
            nb = (int)x.x; succ = cur; succ_y = x.y; cur = x.y >> 16;
        }
        ws[(size_t)t * G] = make_uint2((uint32_t)start, (uint32_t)d | (at_pred << 16));
        if (at_succ) { ws[(size_t)(at_succ - 1) * G].y = (at_succ_y & 0xFFFFu) | ((uint32_t)(t + 1) << 16); ++inserted; }
        else *tail = (uint32_t)(t + 1);
        return start;
    }
};

// One candidate of schedule_decode_kernel (objective i64[2]), of schedule_decode_dyn_kernel (DYN: MO_DFJSP, objective
// i64[3] with the energy, the state a word per machine longer) and of schedule_decode_active_kernel (ACTIVE: group grp of
// the call, its intervals in the workgroup's part `ws` of the workspace)
template <bool DYN, bool ACTIVE = false>
__device__ __forceinline__ void decode_candidate(const DevBatch &b, const DecodeArgs &a, int BW, long long grp, uint2 *ws = nullptr,
                                                 int32_t *d_inserted = nullptr) {
    constexpr int NO = DYN ? 3 : 2;
    const int s = (int)threadIdx.x;
    const long long g = grp * a.G + s;
    if (s >= a.G || g >= a.total) return;
    const int env = (int)(g / a.n_cand), q = (int)(g - (long long)env * a.n_cand), inst = env % b.n_inst;
    const int cap = a.cap;
    const Shop sh = shop_of(b, a.kinds, inst, a.JW);
    const State st = state_at(decode_lds, s, a.G, a.JW);

    // ---- the move, checked against the plan before anything is decoded
    const int32_t *pl = a.plan + ((size_t)env * a.q_plans + (a.q_plans == 1 ? 0 : q)) * (size_t)cap * 3;
    auto row = [&](int idx) { return row_at(pl, idx); };
    Move mv = no_move();
    if (a.moves) {
        const int32_t *m3 = a.moves + (size_t)g * 3;
        mv = move_of(m3[0], m3[1], m3[2], cap, row);
    }

    int err = 0, L = 0;
    long long makespan = 0, tard = 0, energy = 0;
    DynShop dy{};
    if constexpr (DYN) dy = dyn_shop_of(b, sh, st, BW);
    int32_t *tab = a.table ? a.table + (size_t)g * (size_t)cap * 6 : nullptr;
    int inserted = 0;
    if (!mv.bad) {
        auto sink = [&](int t, const Row &x, const Step &d) {
            if (tab) {
                int32_t *o = tab + (size_t)t * 6;
                o[0] = x.r; o[1] = d.stg; o[2] = x.n; o[3] = x.m; o[4] = d.begin; o[5] = d.end;
            }
        };
        if constexpr (ACTIVE) {
            Gaps gaps{ws + s, a.G, 0};
            err = decode_plan<DYN>(b, sh, st, row, cap, mv, sink, L, makespan, tard, &dy, &energy, NoFix{}, &gaps);
            inserted = gaps.inserted;
        } else err = decode_plan<DYN>(b, sh, st, row, cap, mv, sink, L, makespan, tard, &dy, &energy);
        if (move_past(mv, L)) mv.bad = true;
    }
    const int stt = mv.bad ? 4 : err;
    if constexpr (ACTIVE)
        if (d_inserted) d_inserted[g] = stt ? 0 : inserted;
    a.status[g] = stt;
    a.objective[NO * g] = stt ? -1 : makespan;
    a.objective[NO * g + 1] = stt ? -1 : tard;
    if constexpr (DYN) a.objective[NO * g + 2] = stt ? -1 : energy;
    if (a.len) a.len[g] = stt ? 0 : L;
    if (tab) {
        for (int t = stt ? 0 : L; t < cap; ++t) {
            int32_t *o = tab + (size_t)t * 6;
            o[0] = -1; o[1] = -1; o[2] = -1; o[3] = -1; o[4] = -1; o[5] = -1;
        }
    }
}

__global__ __launch_bounds__(256) void schedule_decode_kernel(DevBatch b, DecodeArgs a) { decode_candidate<false>(b, a, 0, (long long)blockIdx.x); }
__global__ __launch_bounds__(256) void schedule_decode_dyn_kernel(DevBatch b, DecodeArgs a, int BW) { decode_candidate<true>(b, a, BW, (long long)blockIdx.x); }
// A bounded grid: workgroup w decodes the groups w, w + gridDim.x, ... of the call one after the other, all of them on
// its own cap x G entries of the workspace.  A lane's state words and entries are its own, so nothing orders the groups.
__global__ __launch_bounds__(256) void schedule_decode_active_kernel(DevBatch b, DecodeArgs a, uint2 *ws, int32_t *d_inserted) {
    uint2 *mine = ws + (size_t)blockIdx.x * (size_t)a.cap * (size_t)a.G;
    for (long long grp = blockIdx.x; grp * a.G < a.total; grp += gridDim.x) decode_candidate<false, true>(b, a, 0, grp, mine, d_inserted);
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
__device__ __forceinline__ TRow trow_at7(const int32_t *tb, int t) {       // the search's rows of seven words, the identity last
    const int32_t *o = tb + (size_t)t * 7;
    return TRow{o[0], o[1], o[2], o[3], o[4], o[5]};
}

// forward over a table (trow: index -> TRow): its end L, every index it supplies checked, the makespan C and the first row
// e0 that ends there.  Returns the status (0, 1 a row fails a check, 2 the table is empty).
template <class TRowAt>
__device__ __forceinline__ int critical_forward(const Shop &sh, TRowAt trow, int cap, int &L, int &C, int &e0) {
    int st = 0;
    L = 0; C = 0; e0 = -1;
    TRow nxt = trow(0);                                                  // (the next row is requested before this one is worked on)
    for (int t = 0; t < cap; ++t) {
        const TRow x = nxt;
        if ((x.r & x.stage & x.n & x.m & x.begin & x.end) == -1) break;
        if (t + 1 < cap) nxt = trow(t + 1);
        L = t + 1;
        bool ok = x.r >= 0 && x.r < sh.R;
        if (ok) {
            const uint2 kd = sh.kinds[1 + x.r];
            const int jbeg = (int)(kd.x & 0xFFFFu), cnt = (int)(kd.x >> 16), koff = (int)(kd.y & 0xFFFFu), Jr = (int)(kd.y >> 16);
            ok = x.n >= 0 && x.n < cnt && jbeg + x.n < sh.JW && x.m >= 0 && x.m < sh.M && x.stage >= 0 && x.stage < Jr &&
                 koff + x.stage < sh.KP && x.begin >= 0 && x.begin < x.end;
        }
        if (!ok) { st = 1; break; }
        if (x.end > C) { C = x.end; e0 = t; }
    }
    if (!st && L == 0) st = 2;
    return st;
}

// What the backward scan writes: tail[L] (nullable), flags[L], path[<= L], mv[max_moves][3] (null with max_moves = 0)
struct CritOut { int32_t *tail; uint8_t *flags; int32_t *path, *mv; int max_moves; };

// backward over a checked table: tail + duration of the latest row seen, per job (jtail[j * G]) and per machine (mtail[m * G]),
// as decode keeps ready / free; tails, flags and one critical path in the same pass; then the path's neighbourhood, its
// machine arcs as pair moves and its operations on their other machines.
template <class TRowAt>
__device__ __forceinline__ void critical_backward(const Shop &sh, TRowAt trow, int L, int C, int e0, uint32_t *jtail, uint32_t *mtail, int G,
                                                  const CritOut o, int &plen_out, int &n_moves_out, int &skipped_out) {
    int plen = 0, n_moves = 0, skipped = 0;
    for (int j = 0; j < sh.JW; ++j) jtail[(size_t)j * G] = 0u;
    for (int m = 0; m < sh.MP; ++m) mtail[(size_t)m * G] = 0u;
    int curj = 0, curm = 0, curb = 0;                                    // the path's current row: job word, machine, begin
    bool needj = false, needm = false;                                   // its job / machine predecessor is still to come
    TRow nxt = trow(L - 1);
    for (int t = L - 1; t >= 0; --t) {
        const TRow x = nxt;
        if (t > 0) nxt = trow(t - 1);
        const int j = (int)(sh.kinds[1 + x.r].x & 0xFFFFu) + x.n;
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
        if (on) { f |= 2u; o.path[plen++] = t; curj = j; curm = x.m; curb = x.begin; needj = needm = true; }
        if (o.tail) o.tail[t] = (int32_t)tl;
        o.flags[t] = (uint8_t)f;
    }

    auto emit = [&](int kind, int u, int third) {
        if (n_moves < o.max_moves) { int32_t *e = o.mv + (size_t)n_moves * 3; e[0] = kind; e[1] = u; e[2] = third; }
        ++n_moves;
    };
    for (int i = 0; i + 1 < plen; ++i) {
        const int u = o.path[i + 1], v = o.path[i];
        if (!(o.flags[u] & 4u)) continue;
        const TRow a = trow(u), bb = trow(v);
        int w = u, first = v;                                            // last row of b's job, first row of a's job in (u, v)
        for (int t = v - 1; t > u; --t) {
            const TRow x = trow(t);
            if (w == u && x.r == bb.r && x.n == bb.n) w = t;
            if (x.r == a.r && x.n == a.n) first = t;
        }
        if (w < first && w - u <= 32767) emit(4, u, (v - u) | ((w - u) << 16));    // (the field stays a non-negative int)
        else ++skipped;
    }
    for (int i = 0; i < plen; ++i) {
        const int t = o.path[i];
        const TRow x = trow(t);
        const uint16_t *pk = sh.p + (size_t)((int)(sh.kinds[1 + x.r].y & 0xFFFFu) + x.stage) * sh.MP;
        for (int m = 0; m < sh.M; ++m)
            if (m != x.m && pk[m] != 0) emit(1, t, m);
    }
    plen_out = plen; n_moves_out = n_moves; skipped_out = skipped;
}

__global__ __launch_bounds__(256) void schedule_critical_kernel(DevBatch b, CriticalArgs a) {
    const int s = (int)threadIdx.x;
    const long long g = (long long)blockIdx.x * a.G + s;
    if (s >= a.G || g >= a.total) return;
    const int env = (int)(g / a.n_cand), inst = env % b.n_inst;
    const int G = a.G, cap = a.cap;
    const Shop sh = shop_of(b, a.kinds, inst, a.JW);

    const int32_t *tb = a.table + (size_t)g * (size_t)cap * 6;
    auto trow = [&](int t) { return trow_at(tb, t); };
    int32_t *tail = a.tail + (size_t)g * cap, *path = a.path + (size_t)g * cap;
    uint8_t *flags = a.flags + (size_t)g * cap;
    int32_t *mv = a.moves ? a.moves + (size_t)g * (size_t)a.max_moves * 3 : nullptr;

    int L = 0, C = 0, e0 = -1, plen = 0, n_moves = 0, skipped = 0;
    const int st = critical_forward(sh, trow, cap, L, C, e0);
    if (!st)
        critical_backward(sh, trow, L, C, e0, decode_lds + s, decode_lds + (size_t)a.JW * G + s, G, CritOut{tail, flags, path, mv, a.max_moves},
                          plen, n_moves, skipped);
    for (int t = st ? 0 : L; t < cap; ++t) { tail[t] = -1; flags[t] = 0; }
    for (int t = plen; t < cap; ++t) path[t] = -1;
    for (int i = n_moves < a.max_moves ? n_moves : a.max_moves; i < a.max_moves; ++i) { mv[(size_t)i * 3] = 0; mv[(size_t)i * 3 + 1] = 0; mv[(size_t)i * 3 + 2] = 0; }
    a.status[g] = st;
    a.makespan[g] = st ? -1 : C;
    a.path_len[g] = plen;
    a.n_moves[g] = n_moves;
    a.skipped[g] = skipped;
}

// ---- fjsp_schedule_search: hill climbing and tabu search, every round of every env in ONE launch.  One 64-lane workgroup
// owns one env, lane q decodes candidate q of a round on its own banked state (G = 64, the decoder's layout and text).
// Beside the states the env keeps in LDS: its plan rows (r, n, m, operation type, identity), the tabu list until[identity]
// and, for the critical neighbourhoods, the current plan's table with the identity as a seventh word, the permutation
// inv[] that puts it into begin order (the table itself is not moved: the scans read row inv[t]), the path, its flags and
// the move list.  A round touches global memory for the instance's tables (kind table, p, due) and its own outputs only.
//   critical modes, per round: every lane decodes the current plan (lane 0 keeps the table); rank by (begin, index) across
//   the lanes -> inv; the rows are rebuilt in begin order from the table; lane 0 runs critical_forward / critical_backward.
//   every mode: the lanes draw their moves (splitmix64 of the global env id, include/fjsp_amd.h), decode them with the move
//   applied while reading, a butterfly over the wave finds the least (objective, q), and the wave applies the move taken: a
//   reassignment is one store, a swap and a pair move rotate the window [pu, pv] of rows, 64 rows to a step.
struct SearchArgs {
    const int32_t *plan;     // i32[N][cap][3]
    int32_t *plan_out;       // i32[N][cap][3]
    int64_t *objective;      // i64[N][2], DYN: i64[N][3]
    int64_t *history;        // i64[rounds + 1][N]
    int32_t *accepted, *status;   // i32[N]
    int32_t *trace;          // i32[rounds][N][3], nullable
    const uint2 *kinds;      // [n_inst][KP + 1]
    unsigned long long seed; // of the search stream (the caller's seed ^ FJSP_SEARCH_STREAM)
    long long first_env;
    int rounds, n_cand, col, nbh, accept, tenure, cap, JW;
};

constexpr int kSearchMoves = 128;                                        // entries of the critical move list a round draws from
// words of LDS behind the 64 states: rows 5, until 1, table 7, inv 1, path 1 per plan row, the flag bytes, the move list
__host__ __device__ inline size_t search_words(int JW, int MP, int cap) {
    return (size_t)state_words(JW, MP) * 64 + (size_t)cap * 15 + (size_t)(cap + 3) / 4 + (size_t)kSearchMoves * 3 + 4;
}

// fjsp_schedule_search_dyn: the states a word per machine longer; rows 5 and until 1 per plan row are all that the uniform
// neighbourhood keeps behind them (no table, inv, path, flag bytes or move list, and so no shared word for the list's length)
__host__ __device__ inline size_t search_dyn_words(int JW, int MP, int cap) { return (size_t)dyn_state_words(JW, MP) * 64 + (size_t)cap * 6; }

__device__ __forceinline__ uint32_t search_pick(uint64_t d, uint32_t n) { return (uint32_t)(((d >> 32) * (uint64_t)n) >> 32); }

// fjsp_schedule_search_front: the search steered by a weighted sum of the objectives, with the Pareto archive of everything
// it decodes.  The kernel is schedule_search_kernel's text compiled with these arguments in place of SearchArgs.
struct FrontArgs : SearchArgs {
    const int64_t *weights;  // i64[N][NO]
    int64_t *front_obj;      // i64[N][cap_front][NO]
    int32_t *front_src;      // i32[N][cap_front][2]
    int32_t *front_plan;     // i32[N][cap_front][cap][3], nullable
    int32_t *front_count, *front_dropped;   // i32[N]
    int cap_front;
};

// words of LDS of that search, both families (states = state_words or dyn_state_words): the 64 states, rows 5 and until 1
// per plan row, and the archive -- vector (NO i64) and source (2) per slot, the round's candidate vectors (NO i64 per lane)
// and the slot of the r-th free one (1 per lane)
__host__ __device__ inline size_t search_front_words(int states, int cap, int cap_front, int NO) {
    return (size_t)states * 64 + (size_t)cap * 6 + (size_t)cap_front * (size_t)(2 * NO + 2) + (size_t)64 * (size_t)(2 * NO + 1);
}

// a key's products and partial sums saturate here, one below the "no candidate" sentinel (weights and objectives are >= 0)
constexpr long long kKeyMax = 0x7ffffffffffffffeLL;
__device__ __forceinline__ long long key_mul(long long w, long long x) {
    long long p;
    return (__builtin_mul_overflow(w, x, &p) || p > kKeyMax) ? kKeyMax : p;
}
__device__ __forceinline__ long long key_add(long long x, long long y) {
    long long s;
    return (__builtin_add_overflow(x, y, &s) || s > kKeyMax) ? kKeyMax : s;
}

// DYN (fjsp_schedule_search_dyn, MO_DFJSP): every decode is decode_plan<true> on a state a word per machine longer, the
// objective has the energy as a third entry carried beside the other two, and the neighbourhood is the uniform one: nbh is
// 0 at compile time, so the critical block and its arrays are not in that kernel.  The template sits on the kernel itself:
// behind a __device__ wrapper the compiler allocated the plain kernel's registers differently and its uniform round ran
// 1.5 % slower; in this form it compiles to the instructions it had before the switch, but for a few reordered ones
// (which is also why the best plan's update below compares first and selects the column after).
//
// A = FrontArgs (fjsp_schedule_search_front, both families): the same switch, one level up.  The neighbourhood is the
// uniform one at compile time, "the chosen objective" is the key sum_c w[c] obj[c] of the env's weights, saturating below
// the sentinel, and the env keeps the Pareto archive of every vector it decodes in LDS behind until[]: per slot the vector
// and its source (round, q), (-1, -1) = free.  Per round, between the decodes and the move taken: the lanes put their
// vectors into LDS; lane = candidate checks itself against the members (broadcast reads, a loop over the bits of the held
// slots' mask) and, if it is past them, against the other candidates that are -> the entrants, a ballot; lane = slot checks
// its member against the entrants and leaves if one dominates it -> the free slots, a ballot; free slot s of rank r (prefix
// count of the ballot) writes fslot[r] = s, entrant of rank r takes fslot[r] and the wave writes its plan, rows read through
// the move's index map.  No lane does the wave's work alone; the loops over members and entrants are wave-uniform.
template <bool DYN, class A = SearchArgs>
__global__ __launch_bounds__(64) void schedule_search_kernel(DevBatch b, A a) {
    constexpr int NO = DYN ? 3 : 2;
    constexpr bool FRONT = std::is_same<A, FrontArgs>::value;
    const int q = (int)threadIdx.x, env = (int)blockIdx.x, inst = env % b.n_inst;
    const int cap = a.cap, Q = a.n_cand, N = b.N, nbh = (DYN || FRONT) ? 0 : a.nbh;
    const Shop sh = shop_of(b, a.kinds, inst, a.JW);
    const State st = state_at(decode_lds, q, 64, a.JW);
    DynShop dy{};
    if constexpr (DYN) dy = dyn_shop_of(b, sh, st, dyn_windows(b));
    int32_t *rows = reinterpret_cast<int32_t *>(decode_lds + (size_t)(DYN ? dyn_state_words(a.JW, b.MP) : state_words(a.JW, b.MP)) * 64);     // [cap][5]
    int32_t *until = rows + (size_t)cap * 5, *tab = until + cap, *inv = tab + (size_t)cap * 7, *path = inv + cap;
    int32_t *mvl = path + cap, *shared = mvl + kSearchMoves * 3;
    uint8_t *flags = reinterpret_cast<uint8_t *>(shared + 4);
    const int32_t *pl = a.plan + (size_t)env * cap * 3;
    int32_t *po = a.plan_out + (size_t)env * cap * 3;

    // ---- the archive (FRONT): vectors, the round's candidate vectors, sources, the slot of the r-th free one; the weights
    long long *fobj = reinterpret_cast<long long *>(until + cap), *cvec = fobj;
    int32_t *fsrc = nullptr, *fslot = nullptr, *fplan = nullptr;
    long long w0 = 0, w1 = 0, w2 = 0;
    int F = 0, dropped = 0;
    bool bad_w = false;
    if constexpr (FRONT) {
        F = a.cap_front;
        cvec = fobj + (size_t)F * NO;
        fsrc = reinterpret_cast<int32_t *>(cvec + 64 * NO); fslot = fsrc + 2 * F;
        if (a.front_plan) fplan = a.front_plan + (size_t)env * F * cap * 3;
        const long long *w = reinterpret_cast<const long long *>(a.weights) + NO * (size_t)env;
        w0 = w[0]; w1 = w[1];
        if constexpr (DYN) w2 = w[2];
        bad_w = w0 < 0 || w1 < 0 || w2 < 0 || (w0 | w1 | w2) == 0;
    }

    // ---- the input plan: copied through, decoded by every lane (one address to the wave), kept by lane 0
    for (int i = q; i < cap * 3; i += 64) po[i] = pl[i];
    int L = 0;
    long long cur_mk = 0, cur_td = 0, cur_en = 0;
    // the chosen objective of (makespan, tardiness, energy); FRONT: their key
    auto chosen = [&](long long mk, long long td, long long en) {
        if constexpr (FRONT) return key_add(key_add(key_mul(w0, mk), key_mul(w1, td)), DYN ? key_mul(w2, en) : 0LL);
        else return DYN && a.col == 2 ? en : (a.col ? td : mk);
    };
    const int st0 = bad_w ? 5 : decode_plan<DYN>(b, sh, st, [&](int idx) { return row_at(pl, idx); }, cap, no_move(), [&](int t, const Row &x, const Step &d) {
        if (q == 0) { int32_t *o = rows + (size_t)t * 5; o[0] = x.r; o[1] = x.n; o[2] = x.m; o[3] = d.k; o[4] = t; until[t] = 0; }
    }, L, cur_mk, cur_td, &dy, &cur_en);
    if (st0 != 0) {                                                      // (the same in every lane)
        if (q == 0) {
            a.status[env] = st0; a.accepted[env] = 0;
            for (int c = 0; c < NO; ++c) a.objective[NO * (size_t)env + c] = -1;
        }
        for (int t = q; t <= a.rounds; t += 64) a.history[(size_t)t * N + env] = -1;
        if (a.trace)
            for (int i = q; i < a.rounds * 3; i += 64) a.trace[((size_t)(i / 3) * N + env) * 3 + i % 3] = 0;
        if constexpr (FRONT) {                                           // an empty archive
            if (q < F) {
                for (int c = 0; c < NO; ++c) a.front_obj[((size_t)env * F + q) * NO + c] = -1;
                a.front_src[((size_t)env * F + q) * 2] = -1; a.front_src[((size_t)env * F + q) * 2 + 1] = -1;
            }
            if (q == 0) { a.front_count[env] = 0; a.front_dropped[env] = 0; }
            if (fplan)
                for (size_t i = q; i < (size_t)F * cap * 3; i += 64) fplan[i] = -1;
        }
        return;
    }
    if constexpr (FRONT) {                                               // the archive is {the input plan} in slot 0
        if (q < F) { fsrc[2 * q] = -1; fsrc[2 * q + 1] = q == 0 ? 0 : -1; }
        if (q == 0) { fobj[0] = cur_mk; fobj[1] = cur_td; if constexpr (DYN) fobj[2] = cur_en; }
    }
    __syncthreads();
    long long best_mk = cur_mk, best_td = cur_td, best_en = cur_en;      // of the plan in plan_out (tabu)
    int taken = 0, n_list = 0;
    unsigned long long heldm = 1ULL;                                     // FRONT: the slots that hold a member, the same in every lane
    if (q == 0) a.history[env] = chosen(cur_mk, cur_td, cur_en);
    const uint64_t sg = gen::draw(a.seed, (uint32_t)(a.first_env + env));
    auto lrow = [&](int idx) { const int32_t *o = rows + (size_t)idx * 5; return idx < L ? Row{o[0], o[1], o[2]} : Row{-1, -1, -1}; };
    auto write_out = [&]() {                                             // the current plan -> plan_out
        for (int t = q; t < cap; t += 64) {
            const Row x = lrow(t);
            po[3 * t] = x.r; po[3 * t + 1] = x.n; po[3 * t + 2] = x.m;
        }
    };
    if constexpr (FRONT)
        if (fplan)
            for (int i = q; i < cap; i += 64) { const Row x = lrow(i); fplan[3 * i] = x.r; fplan[3 * i + 1] = x.n; fplan[3 * i + 2] = x.m; }

    for (int t = 0; t < a.rounds; ++t) {
        if (nbh != 0) {
            // ---- the current plan's table, put into begin order, and the moves of its critical path
            long long mk, td;
            int len;
            decode_plan(b, sh, st, lrow, cap, no_move(), [&](int i, const Row &x, const Step &d) {
                if (q == 0) { int32_t *o = tab + (size_t)i * 7; o[0] = x.r; o[1] = d.stg; o[2] = x.n; o[3] = x.m; o[4] = d.begin; o[5] = d.end; o[6] = rows[(size_t)i * 5 + 4]; }
            }, len, mk, td);
            __syncthreads();
            for (int s = q; s < L; s += 64) {
                const int bs = tab[(size_t)s * 7 + 4];
                int rank = 0;
                for (int i = 0; i < L; ++i) { const int bi = tab[(size_t)i * 7 + 4]; rank += (bi < bs || (bi == bs && i < s)) ? 1 : 0; }
                inv[rank] = s;
            }
            __syncthreads();
            for (int s = q; s < L; s += 64) {
                const int32_t *x = tab + (size_t)inv[s] * 7;
                int32_t *o = rows + (size_t)s * 5;
                o[0] = x[0]; o[1] = x[2]; o[2] = x[3]; o[3] = (int)(sh.kinds[1 + x[0]].y & 0xFFFFu) + x[1]; o[4] = x[6];
            }
            if (q == 0) {
                auto trow = [&](int i) { return i < L ? trow_at7(tab, inv[i]) : TRow{-1, -1, -1, -1, -1, -1}; };
                int Lt = 0, C = 0, e0 = -1, plen = 0, n_moves = 0, skipped = 0;
                if (critical_forward(sh, trow, cap, Lt, C, e0) == 0)
                    critical_backward(sh, trow, Lt, C, e0, decode_lds, decode_lds + (size_t)a.JW * 64, 64, CritOut{nullptr, flags, path, mvl, kSearchMoves},
                                      plen, n_moves, skipped);
                shared[0] = n_moves < kSearchMoves ? n_moves : kSearchMoves;
            }
            __syncthreads();
            n_list = shared[0];
        }

        // ---- candidate q of the round: its draws, its move, its decode
        const uint32_t d0 = 3u * ((uint32_t)t * (uint32_t)Q + (uint32_t)q);
        const bool from_list = nbh == 1 || (nbh == 2 && q < Q / 2);
        bool masked = q >= Q || L == 0;
        int kind = 0, u = 0, third = 0;
        if (!masked) {
            if (from_list) {
                if (n_list == 0) masked = true;
                else { const int32_t *e = mvl + 3 * (size_t)search_pick(gen::draw(sg, d0 + 2u), (uint32_t)n_list); kind = e[0]; u = e[1]; third = e[2]; }
            } else if ((q & 1) == 0) {
                kind = 1; u = (int)search_pick(gen::draw(sg, d0), (uint32_t)L);
                const uint16_t *pk = sh.p + (size_t)rows[(size_t)u * 5 + 3] * sh.MP;
                int n_e = 0;
                for (int m = 0; m < sh.M; ++m) n_e += pk[m] != 0 ? 1 : 0;
                if (n_e == 0) masked = true;
                else {
                    int left = (int)search_pick(gen::draw(sg, d0 + 1u), (uint32_t)n_e);
                    for (int m = 0; m < sh.M; ++m)
                        if (pk[m] != 0 && left-- == 0) { third = m; break; }
                }
            } else {
                kind = 2; u = (int)search_pick(gen::draw(sg, d0), (uint32_t)(L > 1 ? L - 1 : 1));
            }
        }
        long long mk = 0, td = 0, en = 0, key = 0x7fffffffffffffffLL;
        Move mv = no_move();
        int id_a = 0, id_b = -1;                                         // identities of the rows the move moves
        bool decoded = false;                                            // a candidate of the archive: status 0, tabu or not
        if (!masked) {
            mv = move_of(kind, u, third, cap, lrow);
            int len = 0;
            int err = 4;
            if (!mv.bad) {
                err = decode_plan<DYN>(b, sh, st, lrow, cap, mv, [](int, const Row &, const Step &) {}, len, mk, td, &dy, &en);
                if (move_past(mv, len)) err = 4;
            }
            bool ok = err == 0;
            decoded = ok;
            if (ok && a.accept == 2) {
                id_a = rows[(size_t)u * 5 + 4];
                if (kind != 1) id_b = rows[(size_t)(kind == 2 ? u + 1 : mv.pv) * 5 + 4];
                const bool same = kind == 1 ? third == rows[(size_t)u * 5 + 2] : mv.kind == 0;
                const bool tabu = until[id_a] > t || (id_b >= 0 && until[id_b] > t);
                ok = !same && (!tabu || chosen(mk, td, en) < chosen(best_mk, best_td, best_en));
            }
            if (ok) key = chosen(mk, td, en);
        }
        if constexpr (FRONT) {
            // ---- the archive takes the round's candidates, before the move taken is applied
            auto le = [&](const long long *x, long long y0, long long y1, long long y2) { return x[0] <= y0 && x[1] <= y1 && (!DYN || x[2] <= y2); };
            cvec[q * NO] = mk; cvec[q * NO + 1] = td;
            if constexpr (DYN) cvec[q * NO + 2] = en;
            // lane = candidate: no member <= it ...
            bool ent = decoded;
            for (unsigned long long m = heldm; m; m &= m - 1)
                if (le(fobj + (__ffsll(m) - 1) * NO, mk, td, en)) ent = false;
            const unsigned long long past = __ballot(ent);
            __syncthreads();
            // ... no other candidate dominates it, none of lower q equals it.  Only the candidates that are past the members
            // need looking at: where a member is <= a candidate, it is <= everything that candidate dominates or equals
            for (unsigned long long m = past; m; m &= m - 1) {
                const int o = __ffsll(m) - 1;
                const long long *x = cvec + o * NO;
                if (o != q && le(x, mk, td, en) && (o < q || x[0] != mk || x[1] != td || (DYN && x[2] != en))) ent = false;
            }
            const unsigned long long ents = __ballot(ent);
            // lane = slot: a member that an entrant dominates leaves (no member is <= an entrant, so <= is domination)
            bool held = (heldm >> q) & 1ULL;
            if (held) {
                const long long m0 = fobj[q * NO], m1 = fobj[q * NO + 1], m2 = DYN ? fobj[q * NO + 2] : 0;
                for (unsigned long long m = ents; m; m &= m - 1)
                    if (le(cvec + (__ffsll(m) - 1) * NO, m0, m1, m2)) held = false;
            }
            const unsigned long long freem = __ballot(q < F && !held), below = (1ULL << q) - 1ULL;
            if (q < F && !held) { fslot[__popcll(freem & below)] = q; fsrc[2 * q] = -1; fsrc[2 * q + 1] = -1; }
            __syncthreads();
            // entrants take the lowest free slots in ascending q; the others are dropped
            const int n_free = __popcll(freem), n_ent = __popcll(ents), rank = __popcll(ents & below);
            int slot = -1;
            if (ent && rank < n_free) {
                slot = fslot[rank];
                fobj[slot * NO] = mk; fobj[slot * NO + 1] = td;
                if constexpr (DYN) fobj[slot * NO + 2] = en;
                fsrc[2 * slot] = t; fsrc[2 * slot + 1] = q;
            }
            if (n_ent > n_free) dropped += n_ent - n_free;
            if (fplan) {
                for (unsigned long long m = ents; m; m &= m - 1) {
                    const int o = __ffsll(m) - 1, so = __shfl(slot, o);
                    if (so < 0) break;                                   // (nor do the entrants behind it find a slot)
                    Move w = no_move();
                    w.kind = __shfl(mv.kind, o); w.u = __shfl(mv.u, o); w.m_new = __shfl(mv.m_new, o);
                    w.pu = __shfl(mv.pu, o); w.pw = __shfl(mv.pw, o); w.pv = __shfl(mv.pv, o);
                    int32_t *fp = fplan + (size_t)so * cap * 3;
                    for (int i = q; i < cap; i += 64) {
                        Row x = lrow(move_src(w, i));
                        if (w.kind == 1 && i == w.u) x.m = w.m_new;
                        fp[3 * i] = x.r; fp[3 * i + 1] = x.n; fp[3 * i + 2] = x.m;
                    }
                }
            }
            __syncthreads();
            heldm = __ballot(q < F && fsrc[2 * q + 1] != -1);
        }
        // ---- the least (objective, q) of the wave
        int wq = q;
        for (int off = 32; off > 0; off >>= 1) {
            const long long ok2 = __shfl_xor(key, off);
            const int oq = __shfl_xor(wq, off);
            if (ok2 < key || (ok2 == key && oq < wq)) { key = ok2; wq = oq; }
        }
        const long long cur = chosen(cur_mk, cur_td, cur_en);
        const bool take = key != 0x7fffffffffffffffLL && (a.accept == 2 || key < cur || (key == cur && a.accept == 1));
        int t_kind = 0, t_u = 0, t_third = 0;
        if (take) {                                                      // (the same in every lane)
            t_kind = __shfl(kind, wq); t_u = __shfl(u, wq); t_third = __shfl(third, wq);
            const int e_kind = __shfl(mv.kind, wq), pu = __shfl(mv.pu, wq), pw = __shfl(mv.pw, wq), pv = __shfl(mv.pv, wq);
            cur_mk = __shfl(mk, wq); cur_td = __shfl(td, wq);
            if constexpr (DYN) cur_en = __shfl(en, wq);
            const int w_a = __shfl(id_a, wq), w_b = __shfl(id_b, wq);
            __syncthreads();                                             // every lane has read the rows of its candidate
            if (a.accept == 2 && q == 0) {
                const long long rel = (long long)t + 1 + a.tenure;
                const int32_t v = (int32_t)(rel < 0x7fffffffLL ? rel : 0x7fffffffLL);
                until[w_a] = v;
                if (w_b >= 0) until[w_b] = v;
            }
            if (e_kind == 1) {
                if (q == 0) rows[(size_t)t_u * 5 + 2] = t_third;
            } else if (e_kind != 0) {
                // rows pu + 1 .. pw one place down, rows pw + 1 .. pv - 1 one place up, old rows pv and pu between them
                int ra[5], rb[5], x[5];
                for (int c = 0; c < 5; ++c) { ra[c] = rows[(size_t)pu * 5 + c]; rb[c] = rows[(size_t)pv * 5 + c]; }
                __syncthreads();
                for (int base = pu; base < pw; base += 64) {
                    const int i = base + q;
                    if (i < pw) for (int c = 0; c < 5; ++c) x[c] = rows[(size_t)(i + 1) * 5 + c];
                    __syncthreads();
                    if (i < pw) for (int c = 0; c < 5; ++c) rows[(size_t)i * 5 + c] = x[c];
                    __syncthreads();
                }
                for (int top = pv; top >= pw + 2; top -= 64) {
                    const int i = top - q;
                    if (i >= pw + 2) for (int c = 0; c < 5; ++c) x[c] = rows[(size_t)(i - 1) * 5 + c];
                    __syncthreads();
                    if (i >= pw + 2) for (int c = 0; c < 5; ++c) rows[(size_t)i * 5 + c] = x[c];
                    __syncthreads();
                }
                if (q == 0) for (int c = 0; c < 5; ++c) { rows[(size_t)pw * 5 + c] = rb[c]; rows[(size_t)(pw + 1) * 5 + c] = ra[c]; }
            }
            ++taken;
            __syncthreads();
            if (a.accept == 2 && (FRONT ? chosen(cur_mk, cur_td, cur_en) < chosen(best_mk, best_td, best_en)
                                        : (DYN && a.col == 2 ? cur_en < best_en : (a.col ? cur_td < best_td : cur_mk < best_mk)))) { best_mk = cur_mk; best_td = cur_td; best_en = cur_en; write_out(); }
        }
        if (q == 0) {
            a.history[(size_t)(t + 1) * N + env] = chosen(cur_mk, cur_td, cur_en);
            if (a.trace) { int32_t *o = a.trace + ((size_t)t * N + env) * 3; o[0] = t_kind; o[1] = t_u; o[2] = t_third; }
        }
    }
    if (a.accept != 2) {
        best_mk = cur_mk; best_td = cur_td; best_en = cur_en;
        if (a.rounds > 0) write_out();
    }
    if (q == 0) {
        a.status[env] = 0; a.accepted[env] = taken; a.objective[NO * (size_t)env] = best_mk; a.objective[NO * (size_t)env + 1] = best_td;
        if constexpr (DYN) a.objective[NO * (size_t)env + 2] = best_en;
    }
    if constexpr (FRONT) {                                               // the archive as it stands; free slots' plans cleared
        const bool held = q < F && fsrc[2 * q + 1] != -1;
        if (q < F) {
            for (int c = 0; c < NO; ++c) a.front_obj[((size_t)env * F + q) * NO + c] = held ? fobj[q * NO + c] : -1;
            a.front_src[((size_t)env * F + q) * 2] = fsrc[2 * q]; a.front_src[((size_t)env * F + q) * 2 + 1] = fsrc[2 * q + 1];
        }
        const unsigned long long heldm = __ballot(held);
        if (q == 0) { a.front_count[env] = __popcll(heldm); a.front_dropped[env] = dropped; }
        if (fplan)
            for (int s = 0; s < F; ++s)
                if (!((heldm >> s) & 1ULL))
                    for (int i = q; i < cap * 3; i += 64) fplan[(size_t)s * cap * 3 + i] = -1;
    }
}


// ---- fjsp_schedule_evolve: a genetic algorithm on explicit schedules, every generation of every env in ONE launch.  One
// 64-lane workgroup owns one env, lane q owns individual q and decodes it on its own banked state (G = 64, the decoder's
// layout and text).  Beside the states the env keeps in LDS the job set of every lane's crossover (one bit per job, words
// banked like the state) and two rows of 64 keys, written in turn, so that one barrier per generation hands both the keys
// and the children on.  The population lives in global memory and goes to and fro between pop_out and work (generation 1
// reads pop): a child is written by its lane with plain stores and read in the next generation, after the workgroup's
// barrier, with plain loads by whichever lanes drew it as a parent -- a hand-off inside one workgroup, so the barrier's
// workgroup-scope release / acquire is all it needs; none of the three pointers is const __restrict__.
//   A child does not exist before it is decoded: the accessor below merges its parents' rows while decode_plan asks for
//   them, the fix puts the mutated row on its machine once the decode knows the row's stage, and the sink writes the row
//   into the other buffer.  The least (key, index) is the search kernel's butterfly; the tournament reads keys from LDS.
struct EvolveArgs {
    const int32_t *pop;      // i32[N][P][cap][3]
    int32_t *pop_out, *work; // i32[N][P][cap][3] each
    const int64_t *weights;  // i64[N][NO]
    int64_t *pop_obj;        // i64[N][P][NO]
    int32_t *best_plan;      // i32[N][cap][3]
    int64_t *objective;      // i64[N][NO]
    int64_t *history;        // i64[generations + 1][N]
    int32_t *status;         // i32[N]
    int32_t *trace;          // i32[generations][N][P][3], nullable
    const uint2 *kinds;      // [n_inst][KP + 1]
    unsigned long long seed; // of the evolve stream (the caller's seed ^ FJSP_EVOLVE_STREAM)
    long long first_env;
    int P, generations, mut_rate, cap, JW;
};

// words of a lane's job set; words of LDS of an env: the 64 states (states = state_words or dyn_state_words), the 64 job
// sets, two rows of 64 keys (i64)
__host__ __device__ inline int evolve_set_words(int JW) { return (JW + 31) / 32; }
__host__ __device__ inline size_t evolve_words(int states, int JW) { return (size_t)(states + evolve_set_words(JW)) * 64 + 2 * 64 * 2; }

// The lane's placement policy in the text of an env (fjsp_evolve_env.inc): none, or a Gaps object on slot q of the
// workgroup's part of the workspace, whose count is one decode's
template <bool ACTIVE> __device__ __forceinline__ auto evolve_gaps(uint2 *ws, int q) {
    if constexpr (ACTIVE) return Gaps{ws + q, 64, 0};
    else return NoGaps{};
}
__device__ __forceinline__ Gaps *evolve_gaps_ptr(Gaps &g) { return &g; }
__device__ __forceinline__ NoGaps *evolve_gaps_ptr(NoGaps &) { return nullptr; }
__device__ __forceinline__ void evolve_gaps_reset(Gaps *g) { g->inserted = 0; }
__device__ __forceinline__ void evolve_gaps_reset(NoGaps *) {}
__device__ __forceinline__ int evolve_gaps_count(const Gaps *g) { return g->inserted; }
__device__ __forceinline__ int evolve_gaps_count(const NoGaps *) { return 0; }

// The text of one env is fjsp_evolve_env.inc, included by both kernels: it stands IN the kernel, because as a device
// function that both call (by reference or by value, the env passed or read from blockIdx) schedule_evolve_kernel<false>
// and <true> no longer compiled to the instructions they had (tools/isa_compare.py).  It reads DYN, ACTIVE, b, a, env,
// ws (the workgroup's part of the workspace), ins (nullable: the counts) and leaves an env by FJSP_EVOLVE_DONE.
template <bool DYN>
__global__ __launch_bounds__(64) void schedule_evolve_kernel(DevBatch b, EvolveArgs a) {
    constexpr bool ACTIVE = false;
    const int env = (int)blockIdx.x;
    uint2 *const ws = nullptr;
    int32_t *const ins = nullptr;
#define FJSP_EVOLVE_DONE return
#include "fjsp_evolve_env.inc"
#undef FJSP_EVOLVE_DONE
}

// fjsp_schedule_evolve_active: a bounded grid, as schedule_decode_active_kernel's.  Workgroup w evolves the envs w, w +
// gridDim.x, ... one after the other, every lane's intervals in its slot of the workgroup's own cap x 64 entries of the
// workspace (the index is the workgroup's, not the env's; an entry is read only behind a tail word that the same decode
// reset, so nothing an earlier env, call or entry left there is looked at).
//   What one env leaves in LDS for the next: a lane's state words and its job set are read and written by that lane alone
//   (state_at and jset are indexed by q), so program order covers them.  The two key rows are the only words a lane reads
//   that another wrote: generation t reads row (t - 1) & 1 and is closed by the generation's barrier; behind the last of
//   them (T = 0: behind the barrier that follows keys[q]) no lane reads a key again -- the final least() runs on
//   registers -- and every lane still passes the barrier in front of the best_plan copy before it goes on.  So the first
//   write of the next env to a key row comes after two barriers that every lane passed after its last read.  An env with
//   a status is left before it has written or read a key, and its predecessor's reads ended as said; it passes no
//   barrier, which is sound because the status is the same in every lane and no lane waits at one.  In global memory
//   an env touches only its own rows of every array.
__global__ __launch_bounds__(64) void schedule_evolve_active_kernel(DevBatch b, EvolveArgs a, uint2 *d_ws, int32_t *ins) {
    constexpr bool DYN = false, ACTIVE = true;
    uint2 *const ws = d_ws + (size_t)blockIdx.x * (size_t)a.cap * 64;
    for (int env = (int)blockIdx.x; env < b.N; env += (int)gridDim.x) {
#define FJSP_EVOLVE_DONE continue
#include "fjsp_evolve_env.inc"
#undef FJSP_EVOLVE_DONE
    }
}

// candidates per workgroup, 0 = the state of 32 candidates does not fit the LDS of a CU
int decode_group(size_t bytes) {
    for (int G = 256; G >= 64; G >>= 1)
        if (G * bytes <= kLdsTwo) return G;
    if (64 * bytes <= kLdsCu) return 64;
    return 32 * bytes <= kLdsCu ? 32 : 0;
}
int decode_group(const DevBatch &b) { return decode_group((size_t)state_words(b.jcap, b.MP) * 4); }
size_t dyn_state_bytes(const DevBatch &b) { return (size_t)dyn_state_words(b.jcap, b.MP) * 4; }
// BW of the MO_DFJSP kernels: the windows from i_bk to the record's end -- no window index reaches past the record, whatever
// i_bkoff holds

}  // namespace

extern "C" int fjsp_schedule_decode_capacity(const fjsp_env *e) { return e ? e->ops_max : 0; }

extern "C" int fjsp_schedule_decode_group(const fjsp_env *e) {
    return (e && e->b.variant != FJSP_VARIANT_MO_DFJSP) ? decode_group(e->b) : 0;
}

// fjsp_schedule_decode (dyn false) and fjsp_schedule_decode_dyn (dyn true): each takes the handles the other refuses
static int schedule_decode(bool dyn, fjsp_env *e, const int32_t *d_plan, int32_t q_plans, const int32_t *d_moves, int32_t n_cand,
                           int64_t *d_objective, int32_t *d_status, int32_t *d_table, int32_t *d_len, void *stream) {
    const std::string fn = dyn ? "fjsp_schedule_decode_dyn" : "fjsp_schedule_decode";
    if (!e || !d_plan || !d_objective || !d_status) { set_error(fn + ": null env, plan, objective or status pointer"); return FJSP_E_ARG; }
    if (n_cand < 1 || (q_plans != 1 && q_plans != n_cand)) { set_error(fn + ": needs n_cand >= 1 and q_plans = 1 or n_cand"); return FJSP_E_ARG; }
    if ((e->b.variant == FJSP_VARIANT_MO_DFJSP) != dyn) {
        set_error(dyn ? fn + ": decodes MO_DFJSP batches only (breakdown shifts and energy): fjsp_schedule_decode decodes the others"
                      : fn + ": MO_DFJSP batches are not decoded here (breakdown shifts and energy): fjsp_schedule_decode_dyn decodes them");
        return FJSP_E_UNSUPPORTED;
    }
    if (e->gen_failed) { set_error(fn + ": the last regenerate of this handle failed"); return FJSP_E_STATE; }
    const DevBatch &b = e->b;
    const size_t bytes = dyn ? dyn_state_bytes(b) : (size_t)state_words(b.jcap, b.MP) * 4;
    const int G = decode_group(bytes);
    if (G == 0) {
        set_error(fn + ": a candidate's state (5 bytes per job of the largest instance, rounded up to 16 jobs, + " + (dyn ? "8" : "4") +
                  " per machine: " + std::to_string(bytes) + " bytes) exceeds 5120 bytes");
        return FJSP_E_UNSUPPORTED;
    }
    const long long total = (long long)b.N * (long long)n_cand;
    if (e->ops_max <= 0 || total > 0x7fffffffLL) { set_error(fn + ": no operations, or more than 2^31 - 1 candidates"); return FJSP_E_ARG; }
    DeviceGuard guard(e->device);
    if (!e->d_decode_kinds && !dev_alloc(e, (size_t)b.n_inst * (size_t)(b.KP + 1) * sizeof(uint2), &e->d_decode_kinds, "hipMalloc (decode kind table)")) return FJSP_E_HIP;
    hipStream_t st = (hipStream_t)stream;
    if (launch(decode_kinds_kernel, dim3((unsigned)((b.n_inst + 63) / 64)), dim3(64), 0, st, b, e->d_decode_kinds) != 0) {
        set_error("decode_kinds_kernel launch failed"); return FJSP_E_HIP;
    }
    const DecodeArgs a{d_plan, d_moves, d_objective, d_status, d_table, d_len, e->d_decode_kinds, total, (int)n_cand, (int)q_plans, e->ops_max, G, b.jcap};
    const dim3 grid((unsigned)((total + G - 1) / G)), block((unsigned)(G < 64 ? 64 : G));
    const int rc = dyn ? launch(schedule_decode_dyn_kernel, grid, block, bytes * (size_t)G, st, b, a, dyn_windows(b))
                       : launch(schedule_decode_kernel, grid, block, bytes * (size_t)G, st, b, a);
    if (rc != 0) { set_error(std::string(dyn ? "schedule_decode_dyn_kernel" : "schedule_decode_kernel") + " launch failed"); return FJSP_E_HIP; }
    return FJSP_OK;
}

extern "C" int fjsp_schedule_decode(fjsp_env *e, const int32_t *d_plan, int32_t q_plans, const int32_t *d_moves, int32_t n_cand,
                                    int64_t *d_objective, int32_t *d_status, int32_t *d_table, int32_t *d_len, void *stream) {
    return schedule_decode(false, e, d_plan, q_plans, d_moves, n_cand, d_objective, d_status, d_table, d_len, stream);
}

// workgroups of fjsp_schedule_decode_active's grid, each with cap x G entries of 8 bytes: as many as the workspace bound
// pays for, at least one, at most FJSP_DECODE_ACTIVE_MAX_GROUPS
static int active_groups(const fjsp_env *e, int G) {
    const long long per = 8LL * (long long)e->ops_max * (long long)G;
    const long long n = per > 0 ? (long long)FJSP_DECODE_ACTIVE_WORKSPACE_BYTES / per : 0;
    return (int)(n < 1 ? 1 : (n > FJSP_DECODE_ACTIVE_MAX_GROUPS ? FJSP_DECODE_ACTIVE_MAX_GROUPS : n));
}

extern "C" int fjsp_schedule_decode_active_group(const fjsp_env *e) { return fjsp_schedule_decode_group(e); }

extern "C" int fjsp_schedule_decode_active_resident(const fjsp_env *e) {
    const int G = fjsp_schedule_decode_group(e);
    return (G > 0 && e->ops_max > 0) ? active_groups(e, G) * G : 0;
}

extern "C" int fjsp_schedule_decode_active(fjsp_env *e, const int32_t *d_plan, int32_t q_plans, const int32_t *d_moves, int32_t n_cand,
                                           int64_t *d_objective, int32_t *d_status, int32_t *d_table, int32_t *d_len, int32_t *d_inserted,
                                           void *stream) {
    const std::string fn = "fjsp_schedule_decode_active";
    if (!e || !d_plan || !d_objective || !d_status) { set_error(fn + ": null env, plan, objective or status pointer"); return FJSP_E_ARG; }
    if (n_cand < 1 || (q_plans != 1 && q_plans != n_cand)) { set_error(fn + ": needs n_cand >= 1 and q_plans = 1 or n_cand"); return FJSP_E_ARG; }
    if (e->b.variant == FJSP_VARIANT_MO_DFJSP) {
        set_error(fn + ": MO_DFJSP batches are not decoded here (an insertion under breakdown shifts is not defined): fjsp_schedule_decode_dyn decodes them");
        return FJSP_E_UNSUPPORTED;
    }
    if (e->gen_failed) { set_error(fn + ": the last regenerate of this handle failed"); return FJSP_E_STATE; }
    const DevBatch &b = e->b;
    const size_t bytes = (size_t)state_words(b.jcap, b.MP) * 4;
    const int G = decode_group(bytes);
    if (G == 0) {
        set_error(fn + ": a candidate's state (5 bytes per job of the largest instance, rounded up to 16 jobs, + 4 per machine: " +
                  std::to_string(bytes) + " bytes) exceeds 5120 bytes");
        return FJSP_E_UNSUPPORTED;
    }
    const long long total = (long long)b.N * (long long)n_cand;
    if (e->ops_max <= 0 || total > 0x7fffffffLL) { set_error(fn + ": no operations, or more than 2^31 - 1 candidates"); return FJSP_E_ARG; }
    DeviceGuard guard(e->device);
    if (!e->d_decode_kinds && !dev_alloc(e, (size_t)b.n_inst * (size_t)(b.KP + 1) * sizeof(uint2), &e->d_decode_kinds, "hipMalloc (decode kind table)")) return FJSP_E_HIP;
    const int groups = active_groups(e, G);
    if (!e->d_active_ws && !dev_alloc(e, (size_t)groups * (size_t)e->ops_max * (size_t)G * sizeof(uint2), &e->d_active_ws, "hipMalloc (active decode workspace)")) return FJSP_E_HIP;
    hipStream_t st = (hipStream_t)stream;
    if (launch(decode_kinds_kernel, dim3((unsigned)((b.n_inst + 63) / 64)), dim3(64), 0, st, b, e->d_decode_kinds) != 0) {
        set_error("decode_kinds_kernel launch failed"); return FJSP_E_HIP;
    }
    const DecodeArgs a{d_plan, d_moves, d_objective, d_status, d_table, d_len, e->d_decode_kinds, total, (int)n_cand, (int)q_plans, e->ops_max, G, b.jcap};
    const long long need = (total + G - 1) / G;
    const dim3 grid((unsigned)(need < groups ? need : groups)), block((unsigned)(G < 64 ? 64 : G));
    if (launch(schedule_decode_active_kernel, grid, block, bytes * (size_t)G, st, b, a, e->d_active_ws, d_inserted) != 0) {
        set_error("schedule_decode_active_kernel launch failed"); return FJSP_E_HIP;
    }
    return FJSP_OK;
}

extern "C" int fjsp_schedule_decode_dyn_group(const fjsp_env *e) {
    return (e && e->b.variant == FJSP_VARIANT_MO_DFJSP) ? decode_group(dyn_state_bytes(e->b)) : 0;
}

extern "C" int fjsp_schedule_decode_dyn(fjsp_env *e, const int32_t *d_plan, int32_t q_plans, const int32_t *d_moves, int32_t n_cand,
                                        int64_t *d_objective, int32_t *d_status, int32_t *d_table, int32_t *d_len, void *stream) {
    return schedule_decode(true, e, d_plan, q_plans, d_moves, n_cand, d_objective, d_status, d_table, d_len, stream);
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

extern "C" int fjsp_schedule_search_lds(const fjsp_env *e) {
    if (!e || e->b.variant == FJSP_VARIANT_MO_DFJSP || e->ops_max <= 0) return 0;
    const size_t bytes = search_words(e->b.jcap, e->b.MP, e->ops_max) * 4;
    return bytes <= kLdsCu ? (int)bytes : 0;
}

extern "C" int fjsp_schedule_search_dyn_lds(const fjsp_env *e) {
    if (!e || e->b.variant != FJSP_VARIANT_MO_DFJSP || e->ops_max <= 0) return 0;
    const size_t bytes = search_dyn_words(e->b.jcap, e->b.MP, e->ops_max) * 4;
    return bytes <= kLdsCu ? (int)bytes : 0;
}

extern "C" int fjsp_search_draws(uint64_t seed, int64_t env, uint32_t first, int32_t n, uint64_t *h_out) {
    if (n < 0 || (n > 0 && !h_out)) { set_error("fjsp_search_draws: needs n >= 0 and an output array"); return FJSP_E_ARG; }
    const uint64_t sg = gen::draw(seed ^ FJSP_SEARCH_STREAM, (uint32_t)env);
    for (int32_t i = 0; i < n; ++i) h_out[i] = gen::draw(sg, first + (uint32_t)i);
    return FJSP_OK;
}

// fjsp_schedule_search (dyn false) and fjsp_schedule_search_dyn (dyn true, neighbourhood 0): each takes the handles the
// other refuses
static int schedule_search(bool dyn, fjsp_env *e, const int32_t *d_plan, int32_t rounds, int32_t n_cand, int32_t objective, int32_t neighbourhood,
                           int32_t accept, int32_t tenure, uint64_t seed, int64_t first_env, int32_t *d_plan_out, int64_t *d_objective,
                           int64_t *d_history, int32_t *d_accepted, int32_t *d_status, int32_t *d_trace, void *stream) {
    const std::string fn = dyn ? "fjsp_schedule_search_dyn" : "fjsp_schedule_search";
    if (!e || !d_plan || !d_plan_out || !d_objective || !d_history || !d_accepted || !d_status) {
        set_error(fn + ": null env, plan or output pointer"); return FJSP_E_ARG;
    }
    if ((e->b.variant == FJSP_VARIANT_MO_DFJSP) != dyn) {
        set_error(dyn ? fn + ": searches MO_DFJSP batches only (breakdown shifts and energy): fjsp_schedule_search searches the others"
                      : fn + ": MO_DFJSP batches are not searched here (breakdown shifts and energy): fjsp_schedule_search_dyn searches them");
        return FJSP_E_UNSUPPORTED;
    }
    if (e->gen_failed) { set_error(fn + ": the last regenerate of this handle failed"); return FJSP_E_STATE; }
    if (n_cand < 1 || n_cand > 64 || rounds < 0 || tenure < 0) { set_error(fn + ": needs n_cand in 1..64, rounds >= 0 and tenure >= 0"); return FJSP_E_ARG; }
    if (objective < 0 || objective > (dyn ? 2 : 1) || neighbourhood < 0 || neighbourhood > 2 || accept < 0 || accept > 2) {
        set_error(dyn ? fn + ": objective and accept are 0, 1 or 2" : fn + ": objective is 0 or 1, neighbourhood and accept are 0, 1 or 2");
        return FJSP_E_ARG;
    }
    if (neighbourhood != 0 && objective != 0) { set_error(fn + ": the critical neighbourhoods follow the makespan: objective must be 0"); return FJSP_E_ARG; }
    if (3ULL * (unsigned long long)rounds * (unsigned long long)n_cand > 0xFFFFFFFFULL) {
        set_error(fn + ": 3 x rounds x n_cand draws per env exceed 2^32 - 1"); return FJSP_E_ARG;
    }
    const DevBatch &b = e->b;
    if (e->ops_max <= 0) { set_error(fn + ": no operations"); return FJSP_E_ARG; }
    const size_t lds = (dyn ? search_dyn_words(b.jcap, b.MP, e->ops_max) : search_words(b.jcap, b.MP, e->ops_max)) * 4;
    if (lds > kLdsCu) {
        set_error(fn + ": an env's working set (64 candidate states of " + std::to_string((dyn ? dyn_state_words(b.jcap, b.MP) : state_words(b.jcap, b.MP)) * 4) +
                  " bytes and " + (dyn ? "24" : "61") + " bytes per operation: " + std::to_string(lds) + " bytes) exceeds the " + std::to_string(kLdsCu) +
                  " bytes of a CU's LDS");
        return FJSP_E_UNSUPPORTED;
    }
    DeviceGuard guard(e->device);
    if (!e->d_decode_kinds && !dev_alloc(e, (size_t)b.n_inst * (size_t)(b.KP + 1) * sizeof(uint2), &e->d_decode_kinds, "hipMalloc (decode kind table)")) return FJSP_E_HIP;
    hipStream_t st = (hipStream_t)stream;
    if (launch(decode_kinds_kernel, dim3((unsigned)((b.n_inst + 63) / 64)), dim3(64), 0, st, b, e->d_decode_kinds) != 0) {
        set_error("decode_kinds_kernel launch failed"); return FJSP_E_HIP;
    }
    const SearchArgs a{d_plan, d_plan_out, d_objective, d_history, d_accepted, d_status, d_trace, e->d_decode_kinds, seed ^ FJSP_SEARCH_STREAM,
                       (long long)first_env, (int)rounds, (int)n_cand, (int)objective, (int)neighbourhood, (int)accept, (int)tenure, e->ops_max, b.jcap};
    const int rc = dyn ? launch(schedule_search_kernel<true>, dim3((unsigned)b.N), dim3(64), lds, st, b, a)
                       : launch(schedule_search_kernel<false>, dim3((unsigned)b.N), dim3(64), lds, st, b, a);
    if (rc != 0) { set_error(std::string(dyn ? "schedule_search_kernel<true>" : "schedule_search_kernel<false>") + " launch failed"); return FJSP_E_HIP; }
    return FJSP_OK;
}

extern "C" int fjsp_schedule_search(fjsp_env *e, const int32_t *d_plan, int32_t rounds, int32_t n_cand, int32_t objective, int32_t neighbourhood,
                                    int32_t accept, int32_t tenure, uint64_t seed, int64_t first_env, int32_t *d_plan_out, int64_t *d_objective,
                                    int64_t *d_history, int32_t *d_accepted, int32_t *d_status, int32_t *d_trace, void *stream) {
    return schedule_search(false, e, d_plan, rounds, n_cand, objective, neighbourhood, accept, tenure, seed, first_env, d_plan_out, d_objective,
                           d_history, d_accepted, d_status, d_trace, stream);
}

extern "C" int fjsp_schedule_search_dyn(fjsp_env *e, const int32_t *d_plan, int32_t rounds, int32_t n_cand, int32_t objective, int32_t accept,
                                        int32_t tenure, uint64_t seed, int64_t first_env, int32_t *d_plan_out, int64_t *d_objective,
                                        int64_t *d_history, int32_t *d_accepted, int32_t *d_status, int32_t *d_trace, void *stream) {
    return schedule_search(true, e, d_plan, rounds, n_cand, objective, 0, accept, tenure, seed, first_env, d_plan_out, d_objective, d_history,
                           d_accepted, d_status, d_trace, stream);
}

// bytes of an env's working set in fjsp_schedule_search_front, whatever the limit (the kernel lays LDS out by the same words)
static size_t search_front_bytes(const fjsp_env *e, int cap_front) {
    const DevBatch &b = e->b;
    const bool dyn = b.variant == FJSP_VARIANT_MO_DFJSP;
    return search_front_words(dyn ? dyn_state_words(b.jcap, b.MP) : state_words(b.jcap, b.MP), e->ops_max, cap_front, dyn ? 3 : 2) * 4;
}

extern "C" int fjsp_schedule_search_front_lds(const fjsp_env *e, int32_t cap_front) {
    if (!e || e->ops_max <= 0 || cap_front < 1 || cap_front > 64) return 0;
    const size_t bytes = search_front_bytes(e, cap_front);
    return bytes <= kLdsCu ? (int)bytes : 0;
}

extern "C" int fjsp_schedule_search_front(fjsp_env *e, const int32_t *d_plan, int32_t rounds, int32_t n_cand, const int64_t *d_weights,
                                          int32_t accept, int32_t tenure, uint64_t seed, int64_t first_env, int32_t cap_front,
                                          int32_t *d_plan_out, int64_t *d_objective, int64_t *d_history, int32_t *d_accepted, int32_t *d_status,
                                          int32_t *d_trace, int64_t *d_front_obj, int32_t *d_front_src, int32_t *d_front_plan,
                                          int32_t *d_front_count, int32_t *d_front_dropped, void *stream) {
    const std::string fn = "fjsp_schedule_search_front";
    if (!e || !d_plan || !d_weights || !d_plan_out || !d_objective || !d_history || !d_accepted || !d_status || !d_front_obj || !d_front_src ||
        !d_front_count || !d_front_dropped) {
        set_error(fn + ": null env, plan, weights or output pointer"); return FJSP_E_ARG;
    }
    if (e->gen_failed) { set_error(fn + ": the last regenerate of this handle failed"); return FJSP_E_STATE; }
    if (n_cand < 1 || n_cand > 64 || cap_front < 1 || cap_front > 64 || rounds < 0 || tenure < 0) {
        set_error(fn + ": needs n_cand and cap_front in 1..64, rounds >= 0 and tenure >= 0"); return FJSP_E_ARG;
    }
    if (accept < 0 || accept > 2) { set_error(fn + ": accept is 0, 1 or 2"); return FJSP_E_ARG; }
    if (3ULL * (unsigned long long)rounds * (unsigned long long)n_cand > 0xFFFFFFFFULL) {
        set_error(fn + ": 3 x rounds x n_cand draws per env exceed 2^32 - 1"); return FJSP_E_ARG;
    }
    const DevBatch &b = e->b;
    if (e->ops_max <= 0) { set_error(fn + ": no operations"); return FJSP_E_ARG; }
    const bool dyn = b.variant == FJSP_VARIANT_MO_DFJSP;
    const int NO = dyn ? 3 : 2;
    const size_t lds = search_front_bytes(e, cap_front);
    if (lds > kLdsCu) {
        set_error(fn + ": an env's working set (64 candidate states of " + std::to_string((dyn ? dyn_state_words(b.jcap, b.MP) : state_words(b.jcap, b.MP)) * 4) +
                  " bytes, 24 bytes per operation, " + std::to_string(8 * NO + 8) + " per archive slot and " + std::to_string(64 * (8 * NO + 4)) +
                  " more: " + std::to_string(lds) + " bytes) exceeds the " + std::to_string(kLdsCu) + " bytes of a CU's LDS");
        return FJSP_E_UNSUPPORTED;
    }
    DeviceGuard guard(e->device);
    if (!e->d_decode_kinds && !dev_alloc(e, (size_t)b.n_inst * (size_t)(b.KP + 1) * sizeof(uint2), &e->d_decode_kinds, "hipMalloc (decode kind table)")) return FJSP_E_HIP;
    hipStream_t st = (hipStream_t)stream;
    if (launch(decode_kinds_kernel, dim3((unsigned)((b.n_inst + 63) / 64)), dim3(64), 0, st, b, e->d_decode_kinds) != 0) {
        set_error("decode_kinds_kernel launch failed"); return FJSP_E_HIP;
    }
    const FrontArgs a{{d_plan, d_plan_out, d_objective, d_history, d_accepted, d_status, d_trace, e->d_decode_kinds, seed ^ FJSP_SEARCH_STREAM,
                       (long long)first_env, (int)rounds, (int)n_cand, 0, 0, (int)accept, (int)tenure, e->ops_max, b.jcap},
                      d_weights, d_front_obj, d_front_src, d_front_plan, d_front_count, d_front_dropped, (int)cap_front};
    const int rc = dyn ? launch(schedule_search_kernel<true, FrontArgs>, dim3((unsigned)b.N), dim3(64), lds, st, b, a)
                       : launch(schedule_search_kernel<false, FrontArgs>, dim3((unsigned)b.N), dim3(64), lds, st, b, a);
    if (rc != 0) { set_error(std::string(dyn ? "schedule_search_kernel<true, FrontArgs>" : "schedule_search_kernel<false, FrontArgs>") + " launch failed"); return FJSP_E_HIP; }
    return FJSP_OK;
}

// bytes of an env's working set in fjsp_schedule_evolve, whatever the limit (the kernel lays LDS out by the same words)
static size_t evolve_bytes(const fjsp_env *e) {
    const DevBatch &b = e->b;
    return evolve_words(b.variant == FJSP_VARIANT_MO_DFJSP ? dyn_state_words(b.jcap, b.MP) : state_words(b.jcap, b.MP), b.jcap) * 4;
}

extern "C" int fjsp_schedule_evolve_lds(const fjsp_env *e) {
    if (!e || e->ops_max <= 0) return 0;
    const size_t bytes = evolve_bytes(e);
    return bytes <= kLdsCu ? (int)bytes : 0;
}

extern "C" int fjsp_schedule_evolve_active_resident(const fjsp_env *e) { return fjsp_schedule_decode_active_resident(e) / 64; }

// fjsp_schedule_evolve (active false) and fjsp_schedule_evolve_active: one set of checks, in one order
static int schedule_evolve(bool active, fjsp_env *e, const int32_t *d_pop, int32_t pop, int32_t generations, const int64_t *d_weights,
                           int32_t mut_rate, uint64_t seed, int64_t first_env, int32_t *d_pop_out, int32_t *d_work, int64_t *d_pop_obj,
                           int32_t *d_best_plan, int64_t *d_objective, int64_t *d_history, int32_t *d_status, int32_t *d_trace,
                           int32_t *d_pop_inserted, void *stream) {
    const std::string fn = active ? "fjsp_schedule_evolve_active" : "fjsp_schedule_evolve";
    if (!e || !d_pop || !d_weights || !d_pop_out || !d_work || !d_pop_obj || !d_best_plan || !d_objective || !d_history || !d_status) {
        set_error(fn + ": null env, population, weights or output pointer"); return FJSP_E_ARG;
    }
    if (e->gen_failed) { set_error(fn + ": the last regenerate of this handle failed"); return FJSP_E_STATE; }
    if (pop < 1 || pop > 64 || generations < 0 || mut_rate < 0 || mut_rate > 65536) {
        set_error(fn + ": needs pop in 1..64, generations >= 0 and mut_rate in 0..65536"); return FJSP_E_ARG;
    }
    if ((unsigned long long)generations * (unsigned long long)pop > 0xFFFFFFFFULL) {
        set_error(fn + ": generations x pop children per env exceed 2^32 - 1"); return FJSP_E_ARG;
    }
    const DevBatch &b = e->b;
    if (e->ops_max <= 0) { set_error(fn + ": no operations"); return FJSP_E_ARG; }
    const bool dyn = b.variant == FJSP_VARIANT_MO_DFJSP;
    if (active && dyn) {
        set_error(fn + ": MO_DFJSP batches are not decoded here (an insertion under breakdown shifts is not defined): fjsp_schedule_evolve evolves them");
        return FJSP_E_UNSUPPORTED;
    }
    const size_t lds = evolve_bytes(e);
    if (lds > kLdsCu) {
        set_error(fn + ": an env's working set (64 individuals' states of " + std::to_string((dyn ? dyn_state_words(b.jcap, b.MP) : state_words(b.jcap, b.MP)) * 4) +
                  " bytes, 64 job sets of " + std::to_string(evolve_set_words(b.jcap) * 4) + " and 1024 more: " + std::to_string(lds) + " bytes) exceeds the " +
                  std::to_string(kLdsCu) + " bytes of a CU's LDS");
        return FJSP_E_UNSUPPORTED;
    }
    // (a working set within the limit has decode_group >= 64, so at least one env is resident)
    const int resident = active ? fjsp_schedule_evolve_active_resident(e) : 0;
    if (active && resident < 1) { set_error(fn + ": the workspace of fjsp_schedule_decode_active holds no env of 64 individuals"); return FJSP_E_UNSUPPORTED; }
    DeviceGuard guard(e->device);
    if (!e->d_decode_kinds && !dev_alloc(e, (size_t)b.n_inst * (size_t)(b.KP + 1) * sizeof(uint2), &e->d_decode_kinds, "hipMalloc (decode kind table)")) return FJSP_E_HIP;
    if (active && !e->d_active_ws) {                                     // decode_active's workspace, at decode_active's size
        const int G = decode_group(b);
        if (!dev_alloc(e, (size_t)active_groups(e, G) * (size_t)e->ops_max * (size_t)G * sizeof(uint2), &e->d_active_ws, "hipMalloc (active decode workspace)")) return FJSP_E_HIP;
    }
    hipStream_t st = (hipStream_t)stream;
    if (launch(decode_kinds_kernel, dim3((unsigned)((b.n_inst + 63) / 64)), dim3(64), 0, st, b, e->d_decode_kinds) != 0) {
        set_error("decode_kinds_kernel launch failed"); return FJSP_E_HIP;
    }
    const EvolveArgs a{d_pop, d_pop_out, d_work, d_weights, d_pop_obj, d_best_plan, d_objective, d_history, d_status, d_trace, e->d_decode_kinds,
                       seed ^ FJSP_EVOLVE_STREAM, (long long)first_env, (int)pop, (int)generations, (int)mut_rate, e->ops_max, b.jcap};
    if (active) {
        if (launch(schedule_evolve_active_kernel, dim3((unsigned)(b.N < resident ? b.N : resident)), dim3(64), lds, st, b, a, e->d_active_ws, d_pop_inserted) != 0) {
            set_error("schedule_evolve_active_kernel launch failed"); return FJSP_E_HIP;
        }
        return FJSP_OK;
    }
    const int rc = dyn ? launch(schedule_evolve_kernel<true>, dim3((unsigned)b.N), dim3(64), lds, st, b, a)
                       : launch(schedule_evolve_kernel<false>, dim3((unsigned)b.N), dim3(64), lds, st, b, a);
    if (rc != 0) { set_error(std::string(dyn ? "schedule_evolve_kernel<true>" : "schedule_evolve_kernel<false>") + " launch failed"); return FJSP_E_HIP; }
    return FJSP_OK;
}

extern "C" int fjsp_schedule_evolve(fjsp_env *e, const int32_t *d_pop, int32_t pop, int32_t generations, const int64_t *d_weights,
                                    int32_t mut_rate, uint64_t seed, int64_t first_env, int32_t *d_pop_out, int32_t *d_work,
                                    int64_t *d_pop_obj, int32_t *d_best_plan, int64_t *d_objective, int64_t *d_history, int32_t *d_status,
                                    int32_t *d_trace, void *stream) {
    return schedule_evolve(false, e, d_pop, pop, generations, d_weights, mut_rate, seed, first_env, d_pop_out, d_work, d_pop_obj, d_best_plan,
                           d_objective, d_history, d_status, d_trace, nullptr, stream);
}

extern "C" int fjsp_schedule_evolve_active(fjsp_env *e, const int32_t *d_pop, int32_t pop, int32_t generations, const int64_t *d_weights,
                                           int32_t mut_rate, uint64_t seed, int64_t first_env, int32_t *d_pop_out, int32_t *d_work,
                                           int64_t *d_pop_obj, int32_t *d_best_plan, int64_t *d_objective, int64_t *d_history,
                                           int32_t *d_status, int32_t *d_trace, int32_t *d_pop_inserted, void *stream) {
    return schedule_evolve(true, e, d_pop, pop, generations, d_weights, mut_rate, seed, first_env, d_pop_out, d_work, d_pop_obj, d_best_plan,
                           d_objective, d_history, d_status, d_trace, d_pop_inserted, stream);
}
