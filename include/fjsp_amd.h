/*
 * include/fjsp_amd.h -- C ABI of libfjsp_amd.so (MI355X / gfx950).
 *
 * The reference (Linshan-Ding/Deep_Reinforcement_Learning_for_FJSP) has no FFI:
 * its boundary is the duck-typed Python protocol  Env(...).reset() / .step(a)
 * plus a handful of attributes.  This header is what a
 * binding for that protocol binds to; each entry point cites the reference
 * function it replaces (paths relative to the reference root).  Plain pointers
 * and sizes only -- no torch / HIP types in the signatures (streams are passed
 * as void*, i.e. a hipStream_t; NULL = the default stream).
 *
 * Conventions
 *   - every function returns 0 on success or a negative FJSP_E_* code;
 *     fjsp_last_error() returns a thread-local message for the last failure;
 *   - "h_" pointers are host memory, "d_" pointers are device (HBM) memory
 *     owned by the caller unless stated otherwise;
 *   - k = koff[r] + j is the r-major operation-type index (kind_task_tuple
 *     order, environments/SO_DFJSP_instance_read.py:25);
 *   - the device entry points are asynchronous on the given stream and do not
 *     synchronise, with one exception: for batches with order arrivals
 *     (instances with more than one order, FJSP_VARIANT_MO_DFJSP)
 *     fjsp_env_step / fjsp_env_rollout synchronise once per step to solve
 *     the fluid LPs of the environments an order reached (SO_FJSSP.py:218-231);
 *     per-env errors are reported in the status array (fjsp_env_read), not
 *     by aborting the batch.
 */
#ifndef FJSP_AMD_H
#define FJSP_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FJSP_ABI_VERSION 1

enum {
    FJSP_OK = 0,
    FJSP_E_ARG = -1,        /* bad argument                                            */
    FJSP_E_IO = -2,         /* file missing / unparsable                               */
    FJSP_E_FORMAT = -3,     /* instance violates a format assumption                   */
    FJSP_E_LP = -4,         /* fluid LP failed                                         */
    FJSP_E_UNSUPPORTED = -5,/* instance outside what the kernels handle (K, M, jobs)   */
    FJSP_E_HIP = -6,        /* HIP runtime error (no device, launch failure, ...)      */
    FJSP_E_STATE = -7       /* call order violated (e.g. fluid solution missing)       */
};

/* per-env status bits written by the kernels (fjsp_env_status) */
enum {
    FJSP_ST_BAD_TASK_RULE = 1,    /* MyError, SO_FJSSP.py:297                          */
    FJSP_ST_BAD_MACHINE_RULE = 2, /* MyError, SO_FJSSP.py:321                          */
    FJSP_ST_STEP_AFTER_DONE = 4,  /* reference: undefined (ValueError on max([]))      */
    FJSP_ST_NO_EVENT = 8,         /* reference: ValueError min([]) at SO_FJSSP.py:207  */
    FJSP_ST_SCHEDULE_OVERFLOW = 16 /* a dispatch record had no slot left (never expected:
                                      the table holds every operation of the instance) */
};

/* environment variants sharing the SO_FJSSP skeleton */
enum {
    FJSP_VARIANT_SO_FJSSP = 0,          /* environments/SO_FJSSP.py (pair action [6,5], 20-dim state) */
    FJSP_VARIANT_SO_SFJSP = 1,          /* environments/SO_SFJSP.py (flat 20 = 4x5, 18-dim state, makespan)  */
    FJSP_VARIANT_MO_FJSSP_DISCRETES = 2,/* environments/MO_FJSSP_discretes.py (flat 18, 25-dim state)  */
    FJSP_VARIANT_SO_DFJSP = 5,          /* environments/SO_DFJSP.py (agents/DA3C's environment): SO_FJSSP.py over
                                           class_FJSP.py -- job due date = the order's delivery time (class_FJSP.py:229),
                                           Machine.gap_ave without the 1e-18 (:159); same actions, state and kernels */
    FJSP_VARIANT_MO_DFJSP = 4           /* environments/MO_DFJSP_breakdown.py (and MO_DFJSP.py = no breakdown windows):
                                           pair action [12,10], 30-dim state, order arrivals, machine breakdowns,
                                           energy; needs instances with machine data (fjsp_instances_set_dynamic
                                           or a machine_data.csv) */
};

const char *fjsp_last_error(void);
int fjsp_abi_version(void);

/* ------------------------------------------------------------------------- *
 * Host side: instance sets (replaces Data / Instance / FJSP.__init__ / fluid_model)
 * ------------------------------------------------------------------------- */
typedef struct fjsp_instances fjsp_instances;

/* Parameters of the synthetic generator (environments/Instance_generate.py:19-94).
 * The reference generator is unseeded; this one is a counter-based splitmix64
 * stream so instance i of a batch is a pure function of (seed, params). */
typedef struct {
    int32_t R_min, R_max;     /* kinds                     (:42  U{3..12})            */
    int32_t J_min, J_max;     /* ops per kind              (:46  U{3..5})             */
    int32_t M;                /* machines                  (constructor argument)     */
    int32_t p_min, p_max;     /* processing time           (:50  U{40..400})          */
    int32_t N_min, N_max;     /* jobs per kind per order   (:54  U{5..50})            */
    int32_t S;                /* orders                    (constructor argument)     */
    double  DDT;              /* due-date tightness        (constructor argument)     */
    double  t_si_min, t_si_max; /* order inter-arrival     (:58  U(100,200))          */
} fjsp_gen_params;

/* The generator's parameters with the machine count and the due-date tightness drawn PER INSTANCE, as the reference's
 * training loops do (MPPPO.py:149-154 M = randint(10, 20), DDQN.py:99-104 M = randint(3, 8); both DDT = uniform(0.5, 1.5)).
 * The instance of seed s under ranges q is fjsp_instances_generate(s, p), p = q.base with
 *     p.M   = randint(M_min, M_max)       draw 0 \  of an auxiliary splitmix64 stream seeded s ^ FJSP_GEN_AUX_STREAM:
 *     p.DDT = uniform(DDT_min, DDT_max)   draw 1 /  a + (int)(((z >> 32) * (b - a + 1)) >> 32) and a + (b - a) * ((z >> 11) * 2^-53)
 * Both draws are always taken; the main stream of seed s is untouched, so a point range (M_min == M_max, DDT_min ==
 * DDT_max) gives the instances of the fixed parameter set. */
#define FJSP_GEN_AUX_STREAM 0xD1B54A32D192ED03ULL
typedef struct {
    fjsp_gen_params base;      /* base.M and base.DDT are not read */
    int32_t M_min, M_max;      /* machines per instance:  U{M_min..M_max}      */
    double  DDT_min, DDT_max;  /* due-date tightness:     U(DDT_min, DDT_max)  */
} fjsp_gen_ranges;

/* ... and the number of orders, as the reference's DA3C / HMPSAC loops draw it (DA3C_double_actor.py:243-248,
 * A3C_v5.1.py:245-250: S = randint(1, 5)).  The instance of seed s under q is fjsp_instances_generate(s, p), p = q.r.base
 * with p.M and p.DDT as under q.r and
 *     p.S   = randint(S_min, S_max)       draw 2 of the same auxiliary stream, the integer formula above
 * THE CONTRACT: all three draws are always taken, draws 0 and 1 are those of fjsp_gen_ranges and the main stream of seed s is
 * untouched, so a point range in all three (M_min == M_max, DDT_min == DDT_max, S_min == S_max) gives exactly the
 * instances of fjsp_instances_generate with that fixed parameter set.
 * FJSP_GEN_MAX_ORDERS: the most orders a batch generated on the device can draw (fjsp_env_create_generated_orders; the
 * reference draws at most 6); it sizes the generator kernel's per-order arrays. */
#define FJSP_GEN_MAX_ORDERS 16
typedef struct {
    fjsp_gen_ranges r;         /* r.base.S is not read */
    int32_t S_min, S_max;      /* orders per instance:    U{S_min..S_max}      */
} fjsp_gen_orders;

/* ... and the machine data of a dynamic multi-objective shop (FJSP_VARIANT_MO_DFJSP): processing power per eligible pair,
 * idle power per machine, breakdown windows per machine.  The reference's generator draws powers U{10..200}, idle powers
 * U{1..9} and no windows (Instance_generate.py:61-66; its Python stream is pinned nowhere, so this stream is the library's
 * own).  The machine data of instance s (M machines, K operation types) are draws of the splitmix64 stream seeded
 * s ^ FJSP_GEN_MACHINE_STREAM, each at a position that is a pure function of its indices (the integer formula above):
 *     idle power of machine m         U{idle_min..idle_max}   draw m
 *     window count of machine m       U{0..W_max}             draw M + m
 *     power of pair (k, m)            U{pw_min..pw_max}       draw 2M + k*M + m   (reserved for an ineligible pair too: its power is 0)
 *     gap of window w of machine m    U{gap_min..gap_max}     draw 2M + K*M + 2*(m*W_max + w)
 *     length of that window           U{len_min..len_max}     the draw behind its gap
 * Window w starts at the end of window w - 1 (0 for the first) plus its gap and ends at its start plus its length, so the
 * windows of a machine are sorted, disjoint and non-empty; powers and idle powers do not depend on W_max.  All draws of an
 * instance are always reserved; the main and the auxiliary stream of s are untouched.
 * FJSP_GEN_MAX_WINDOWS: the largest W_max (32 machines x 2047 windows index the record's u16 window offsets). */
#define FJSP_GEN_MACHINE_STREAM 0xA0761D6478BD642FULL
#define FJSP_GEN_MAX_WINDOWS 2047
typedef struct {
    int32_t pw_min, pw_max;     /* processing power of an eligible pair */
    int32_t idle_min, idle_max; /* idle power of a machine */
    int32_t W_max;              /* most breakdown windows of a machine, 0 = none */
    int32_t gap_min, gap_max;   /* working time in front of a window */
    int32_t len_min, len_max;   /* length of a window */
} fjsp_gen_machine;

/* An MO_DFJSP instance: the shop of a fjsp_gen_orders and its machine data.  MO_DFJSP cannot play an instance with a machine
 * that no operation is eligible on (Machine.gap_ave divides by zero in the reference), so such an instance is drawn again:
 * attempt j of instance s is the WHOLE instance (M, DDT, S, the shop, the machine data) of seed s_j, with s_0 = s and, for
 * j > 0, s_j = draw j - 1 of the splitmix64 stream seeded s ^ FJSP_GEN_REDRAW_STREAM (never s + j, which is a neighbour's
 * seed).  The instance is the first attempt in which every machine has an eligible operation; after `redraws` further
 * attempts (0 ... FJSP_GEN_MAX_REDRAWS) the instance fails with FJSP_E_UNSUPPORTED. */
#define FJSP_GEN_REDRAW_STREAM 0xE7037ED1A0B428DBULL
#define FJSP_GEN_MAX_REDRAWS 16
typedef struct {
    fjsp_gen_orders o;
    fjsp_gen_machine m;
    int32_t redraws;
} fjsp_gen_dynamic;

int  fjsp_instances_create(int32_t n, fjsp_instances **out);
void fjsp_instances_destroy(fjsp_instances *s);
int  fjsp_instances_count(const fjsp_instances *s);

/* Data(path, file_name): environments/SO_DFJSP_instance_read.py:6-89
 * (based_data.csv / process_data.csv / order_data.csv; numbers via the
 * reference's `\d+` extraction, so DDT "0.5" parses to 0). */
int fjsp_instances_load_csv(fjsp_instances *s, int32_t i, const char *path, const char *file_name);
/* Instance(DDT, M, S): environments/Instance_generate.py:24-94, seeded. */
int fjsp_instances_generate(fjsp_instances *s, int32_t i, uint64_t seed, const fjsp_gen_params *prm);
/* The parameter set that instance `seed` is generated with under ranges q (see fjsp_gen_ranges).  FJSP_E_ARG for
 * M_min <= 0, M_max < M_min, non-finite DDT bounds or DDT_max < DDT_min; the message names the bound. */
int fjsp_gen_draw(const fjsp_gen_ranges *q, uint64_t seed, fjsp_gen_params *out);
/* fjsp_gen_draw, then fjsp_instances_generate with what it drew. */
int fjsp_instances_generate_drawn(fjsp_instances *s, int32_t i, uint64_t seed, const fjsp_gen_ranges *q);
/* The same with the number of orders drawn as well (see fjsp_gen_orders).  FJSP_E_ARG for the bounds fjsp_gen_draw refuses,
 * S_min < 1, S_max < S_min, and order intervals (r.base.t_si_min / t_si_max) that are not finite, negative or max < min; the
 * message names the bound. */
int fjsp_gen_draw_orders(const fjsp_gen_orders *q, uint64_t seed, fjsp_gen_params *out);
/* fjsp_gen_draw_orders, then fjsp_instances_generate with what it drew. */
int fjsp_instances_generate_orders(fjsp_instances *s, int32_t i, uint64_t seed, const fjsp_gen_orders *q);
/* The MO_DFJSP instance of `seed` under q (see fjsp_gen_dynamic).  fjsp_gen_dynamic_seed: the seed of the first attempt in
 * which every machine has an eligible operation, in *used (== seed where attempt 0 is playable); FJSP_E_UNSUPPORTED, the
 * message naming the seed, when none of the 1 + q->redraws attempts is.  fjsp_gen_draw_dynamic: the parameter set of that
 * seed (fjsp_gen_draw_orders of it).  fjsp_instances_generate_dynamic: fjsp_instances_generate_orders of that seed plus the
 * machine data of the stream above (fjsp_instances_get_dynamic reads them); its failure names the instance as well.
 * FJSP_E_ARG, the message naming the field: the bounds fjsp_gen_draw_orders refuses, a machine range with max < min,
 * pw_min < 1, idle_min < 0, W_max < 0, gap_min < 1, len_min < 1, redraws < 0.  FJSP_E_UNSUPPORTED, likewise: W_max >
 * FJSP_GEN_MAX_WINDOWS, redraws > FJSP_GEN_MAX_REDRAWS, pw_max > 65535, pw_max x p_max > 2^31 - 1 (the energy of one
 * operation), W_max x (gap_max + len_max) > 2^31 - 1 (the end of a machine's last window). */
int fjsp_gen_dynamic_seed(const fjsp_gen_dynamic *q, uint64_t seed, uint64_t *used);
int fjsp_gen_draw_dynamic(const fjsp_gen_dynamic *q, uint64_t seed, fjsp_gen_params *out);
int fjsp_instances_generate_dynamic(fjsp_instances *s, int32_t i, uint64_t seed, const fjsp_gen_dynamic *q);
/* Raw arrays (same meaning as the fjsp_instances_get outputs). */
int fjsp_instances_set_raw(fjsp_instances *s, int32_t i, int32_t R, int32_t M, int32_t S,
                           const int32_t *Jr, const int32_t *p /*[K*M] k-major, 0 = ineligible*/,
                           const int32_t *elig_n /*[K]*/, const int32_t *elig_list /*[K*M] file order*/,
                           const int32_t *count /*[S*R]*/, const int32_t *arrive /*[S]*/,
                           const int32_t *delivery /*[S]*/, double ddt);
/* dims[0..5] = R, M, K, S, jobs of order 0, total jobs over all orders */
int fjsp_instances_dims(const fjsp_instances *s, int32_t i, int32_t dims[6]);
/* Any output pointer may be NULL. */
int fjsp_instances_get(const fjsp_instances *s, int32_t i, int32_t *Jr, int32_t *p, int32_t *elig_n,
                       int32_t *elig_list, int32_t *count, int32_t *arrive, int32_t *delivery,
                       double *ddt, double *x /*[K*M] k-major, fluid solution or zeros*/);

/* Dynamic multi-objective folders (environments/MO_DFJSP_instance_read.py:6-108: process_data.csv carries a
 * power column, machine_data.csv the idle power and the breakdown windows of every machine); load_csv reads
 * them when machine_data.csv exists.  dims[0] = 1 if present, dims[1] = total number of breakdown windows.
 * power[K*M] k-major (0 = ineligible), idle_power[M], bk_n[M] windows per machine, bk[2*total] flattened
 * (start, end) pairs machine-major in file order. */
int fjsp_instances_dynamic_dims(const fjsp_instances *s, int32_t i, int32_t dims[2]);
int fjsp_instances_get_dynamic(const fjsp_instances *s, int32_t i, int32_t *power, int32_t *idle_power,
                               int32_t *bk_n, int32_t *bk);
int fjsp_instances_set_dynamic(fjsp_instances *s, int32_t i, const int32_t *power, const int32_t *idle_power,
                               const int32_t *bk_n, const int32_t *bk);

/* FJSP.fluid_model() for the reset-time state (environments/class_FJSSP.py:246-280):
 * solves the fluid LP of instances [first, first+n) with the library's own
 * deterministic vertex simplex on n_threads host threads and stores x. */
int fjsp_instances_solve_fluid(fjsp_instances *s, int32_t first, int32_t n, int32_t n_threads);
/* Override the stored fluid solution (x is an INPUT of the accelerated path). */
int fjsp_instances_set_x(fjsp_instances *s, int32_t i, const double *x /*[K*M] k-major*/);
/* One fluid LP for an arbitrary live state (class_FJSSP.py:246-280):
 * Q[k] = fluid_unprocessed_number_start, n_now[k] = fluid_number. */
int fjsp_fluid_lp(int32_t R, int32_t M, const int32_t *Jr, const int32_t *p /*[K*M]*/,
                  const int32_t *Q /*[K]*/, const int32_t *n_now /*[K]*/,
                  double *x /*[K*M]*/, double *objective);

/* ------------------------------------------------------------------------- *
 * Device side: a batch of N environments resident in HBM
 * ------------------------------------------------------------------------- */
typedef struct fjsp_env fjsp_env;

/* FJSP.__init__ + SO_FJSSP_Environment.__init__ (class_FJSSP.py:151-171,
 * SO_FJSSP.py:14-48) for N envs: env e uses instance (first + e % n_inst).
 * Packs the padded struct-of-arrays, uploads it to `device`, runs the
 * fluid-table kernel (update_fluid_parameter, class_FJSSP.py:282-306) and one
 * internal reset that caches every instance's reset observation; the envs are
 * then left in the "done" state, so a step before fjsp_env_reset is flagged
 * FJSP_ST_STEP_AFTER_DONE (or starts a fresh episode with autoreset).
 * variant: FJSP_VARIANT_*; FJSP_VARIANT_MO_DFJSP needs instances with machine data. */
int  fjsp_env_create(const fjsp_instances *s, int32_t first, int32_t n_inst, int32_t n_envs,
                     int32_t variant, int32_t device, uint64_t rng_seed, fjsp_env **out);
/* fjsp_env_create with the kernel family chosen by the caller instead of the environment (fjsp_env_kernel_family):
 * family -1 = as fjsp_env_create (row kernels where the batch fits them unless FJSP_STEP_IMPL=wave), 0 = one wave per
 * environment, 1 = the row kernels (FJSP_E_UNSUPPORTED if the batch does not fit them).  The environment variable is
 * not read for 0 and 1: a batch that must match another one's family (a snapshot's fingerprint) is made this way. */
int  fjsp_env_create_family(const fjsp_instances *s, int32_t first, int32_t n_inst, int32_t n_envs, int32_t variant,
                            int32_t device, uint64_t rng_seed, int32_t family, fjsp_env **out);
/* A batch whose instances are generated, and their fluid LPs solved, ON THE DEVICE (csrc/fjsp_generate.hip): instance i is
 * what fjsp_instances_generate(seed_base + i, prm) + fjsp_instances_solve_fluid + fjsp_env_create_family give, record
 * for record (x bit for bit; DEVIATION: the two pow-derived entries of the MO_FJSSP_discretes static state are d * d on
 * the device, as the observation's already are).  The handle owns its instance records, sized from the parameters' worst
 * case (R_max x J_max operation types, R_max x N_max jobs), so kernel family, builds and schedule capacity never change:
 * fjsp_env_regenerate refills the records in place from other seeds -- no host instance set, no instance upload, no device allocation --
 * and leaves every env as a create leaves it (done; env random streams restarted from rng_seed; recorded schedule cleared).
 * One order only: prm->S > 1 and FJSP_VARIANT_MO_DFJSP are FJSP_E_UNSUPPORTED here (several orders:
 * fjsp_env_create_generated_orders below; MO_DFJSP needs machine data: fjsp_env_create_generated_dynamic below).  Bad parameters (the checks of fjsp_instances_generate), an unknown variant, n_inst <= 0 or n_envs <= 0:
 * FJSP_E_ARG; a worst case outside the kernels' limits: FJSP_E_UNSUPPORTED; all before the first HIP call.
 * An LP whose tableau fits the LDS of a CU is solved by the device simplex, the others by the host's on
 * fjsp_env_set_lp_threads threads; FJSP_LP_IMPL=host sends all to the host, =device refuses (FJSP_E_UNSUPPORTED) when one
 * does not fit, =global sends those that do not fit but stay within 256 rows x 1536 columns to the device simplex with its
 * tableau in global memory (csrc/fjsp_lp_global.hip) and only the rest to the host.  All are pivot for pivot the same, so
 * x does not depend on the route.
 * A failing instance (SO_DFJSP: a machine without eligible operation, FJSP_E_UNSUPPORTED; an LP failure, FJSP_E_LP) is
 * named with its seed in fjsp_last_error; after a failed fjsp_env_regenerate reset, step, rollout, the policy launches, read,
 * schedule, snapshots, fjsp_env_fluid_tables and fjsp_env_instance_read return FJSP_E_STATE until a later one succeeds.  fjsp_env_regenerate on any other handle: FJSP_E_STATE.  Both synchronise.
 * Snapshots: the fingerprint of such a handle is (prm, n_inst, seed_base, SO_DFJSP or not), so a snapshot taken before a regenerate onto
 * other seeds is refused after it. */
int  fjsp_env_create_generated(const fjsp_gen_params *prm, int32_t n_inst, int32_t n_envs, int32_t variant, int32_t device,
                               uint64_t rng_seed, int32_t family, uint64_t seed_base, fjsp_env **out);
/* fjsp_env_create_generated with M and DDT drawn per instance (fjsp_gen_ranges): instance i is what
 * fjsp_instances_generate_drawn(seed_base + i, q) + fjsp_instances_solve_fluid + fjsp_env_create_family give.  The handle is
 * sized over the ranges: sizes, kernel family (the row kernels iff M_max <= 8 and the batch fits them otherwise), builds and
 * schedule capacity from M_max, the 32-bit clock bound from DDT_max / (2 M_min); InstHeader.M, the LP tableau and its route
 * are the instance's own.  fjsp_env_regenerate, fjsp_env_generated_stats / _times, fjsp_env_instance_read (dims[1] and *ddt
 * are the instance's own M and DDT), snapshots, schedule recording and the decoders work on such a handle as on a
 * fixed-parameter one; its snapshot fingerprint mixes the ranges and a tag, so it never matches a fixed-parameter handle's.
 * FJSP_E_ARG: M_min <= 0, M_max < M_min, non-finite DDT bounds, DDT_max < DDT_min, the checks of fjsp_env_create_generated on
 * base; FJSP_E_UNSUPPORTED: M_max > 32, base.S > 1, MO_DFJSP, a worst case outside the kernels' limits; all before the
 * first HIP call, the message naming the bound. */
int  fjsp_env_create_generated_ranges(const fjsp_gen_ranges *q, int32_t n_inst, int32_t n_envs, int32_t variant, int32_t device,
                                      uint64_t rng_seed, int32_t family, uint64_t seed_base, fjsp_env **out);
/* ... and with the number of orders drawn per instance (fjsp_gen_orders): instance i is what
 * fjsp_instances_generate_orders(seed_base + i, q) + fjsp_instances_solve_fluid + fjsp_env_create_family give, record for
 * record, x bit for bit.  The generator kernel and the host generator compile one text (csrc/fjsp_gen_stream.h): the S x R job counts order-major,
 * then the S - 1 arrival intervals, arrival times as truncated running sums, delivery times arrive + gap sorted ascending.
 * The handle is sized for S_max, M_max and the worst case (R_max N_max S_max jobs, R_max J_max N_max S_max operations); it
 * is a multi-order handle -- per-env fluid tables, order-arrival LPs -- iff S_max > 1, and an instance that drew S = 1 plays
 * on it as a one-order instance.  The arrival service (device simplex in LDS, in global memory, or the host) is chosen
 * once, at create, from the parameters' worst tableau (R_max kinds of J_max operations, every pair eligible on M_max
 * machines) by the rule of fjsp_env_create and FJSP_LP_IMPL; a host or asynchronous service reads a host mirror of the
 * records' heads that every fjsp_env_regenerate refills.  fjsp_env_regenerate on such a handle is FJSP_E_STATE while envs
 * are parked in the asynchronous service; it empties the memo of solved arrival LPs and leaves fjsp_env_lp_solves and the
 * device pivot counters running.  fjsp_env_instance_read gives dims[3] = the instance's own S, count[S * R], arrive[S],
 * delivery[S]; fjsp_env_generated_stats*, snapshots (the fingerprint also mixes a tag, S_min, S_max and the interval
 * bounds) and schedule recording work as on the other generated handles; the policy launches refuse a multi-order handle.
 * FJSP_VARIANT_SO_FJSSP and _SO_DFJSP for any S_max; _SO_SFJSP and _MO_FJSSP_DISCRETES only with S_max == 1 (then as
 * fjsp_env_create_generated_ranges), else FJSP_E_UNSUPPORTED; _MO_DFJSP: FJSP_E_UNSUPPORTED.  FJSP_E_ARG: the bounds
 * fjsp_gen_draw_orders refuses and those of fjsp_env_create_generated_ranges; FJSP_E_UNSUPPORTED: S_max >
 * FJSP_GEN_MAX_ORDERS, a worst case outside the kernels' limits (the 32-bit clock bound counts the last arrival,
 * (S_max - 1) t_si_max, and the work of all orders); all before the first HIP call, the message naming the bound. */
int  fjsp_env_create_generated_orders(const fjsp_gen_orders *q, int32_t n_inst, int32_t n_envs, int32_t variant, int32_t device,
                                      uint64_t rng_seed, int32_t family, uint64_t seed_base, fjsp_env **out);
/* A FJSP_VARIANT_MO_DFJSP batch generated on the device (fjsp_gen_dynamic): instance i is what
 * fjsp_instances_generate_dynamic(seed_base + i, q) + fjsp_instances_solve_fluid + fjsp_env_create give -- the shop, the
 * machine data (generate_machine_kernel: the record's powers, idle powers and breakdown windows are byte for byte what the
 * host packs), x bit for bit, and so the episodes.  The redraw loop runs in the generator kernel, bounded by q->redraws;
 * an instance without a playable attempt fails the call as it fails on the host (FJSP_E_UNSUPPORTED, named with its seed).
 * One wave per environment (the row kernels do not play MO_DFJSP); always a multi-order handle, sized as
 * fjsp_env_create_generated_orders sizes its own plus M_max x W_max breakdown windows per record; the arrival service is chosen and
 * behaves as there (fjsp_env_regenerate, the host mirror, the refusal while envs are parked).  The snapshot fingerprint
 * mixes a tag, the machine ranges and redraws.  Refusals: those of fjsp_instances_generate_dynamic and of
 * fjsp_env_create_generated_orders; FJSP_E_UNSUPPORTED when the 32-bit clock bound fails once it counts every breakdown
 * window (M_max x W_max x len_max); all before the first HIP call, the message naming the bound.
 * fjsp_env_create_generated, _ranges and _orders keep refusing FJSP_VARIANT_MO_DFJSP and name this entry point.
 * fjsp_env_instance_read_dynamic: the machine data of instance i read back from the device, the twin of
 * fjsp_instances_dynamic_dims / _get_dynamic (dims[0] = 1, dims[1] = windows of the instance; bk holds dims[1] (start, end)
 * pairs), and the seed the instance was made of (seed_base + i unless it was drawn again); every output nullable;
 * FJSP_E_STATE on any other handle.  Synchronises. */
int  fjsp_env_create_generated_dynamic(const fjsp_gen_dynamic *q, int32_t n_inst, int32_t n_envs, int32_t device, uint64_t rng_seed,
                                       uint64_t seed_base, fjsp_env **out);
int  fjsp_env_instance_read_dynamic(fjsp_env *e, int32_t i, int32_t *power, int32_t *idle_power, int32_t *bk_n, int32_t *bk,
                                    uint64_t *seed_used, int32_t dims[2]);
int  fjsp_env_regenerate(fjsp_env *e, uint64_t seed_base, uint64_t rng_seed);
/* fjsp_env_regenerate for some instances of any generated handle: instance i with d_mask[i] != 0 (u8[n_inst], device)
 * becomes the instance of seed seed_base + i, and the envs q with q % n_inst == i are left as fjsp_env_regenerate leaves
 * them -- record zeroed, random stream started over from the handle's rng_seed, recorded dispatches cleared, done.
 * d_mask == NULL: the finished ones -- instance i iff every env that plays it is done, decided on the device.  d_refreshed
 * (u8[n_inst], device, nullable) receives the mask that was applied.  Every other instance record, env record and recorded
 * dispatch keeps its bytes: those envs play on, mid-episode or between order arrivals, as if the call had not happened.
 * An empty mask is FJSP_OK and changes nothing; a full one leaves what fjsp_env_regenerate(e, seed_base, the handle's
 * rng_seed) leaves.  Synchronises; FJSP_E_STATE while envs are parked in the asynchronous service; empties the memo of
 * solved arrival LPs, refills the host mirror's refreshed heads.  fjsp_env_generated_stats* / _times describe the last call
 * of either kind ([0]: instances refreshed); fjsp_env_step_bytes stays the mean over all instances.
 * The handle keeps one seed per instance (fjsp_env_instance_seed: seed_base + i of the call that made it last; every
 * message that names an instance takes its seed from there).  The snapshot fingerprint is a function of these seeds: while
 * they are s + i for one s it is that of fjsp_env_regenerate(s), otherwise it mixes a tag and all of them, so a snapshot
 * taken before a call that changed a seed is refused after it.
 * A failing instance fails the call as it fails fjsp_env_regenerate (same codes, same refusals afterwards).  The instances
 * the failed call was making are remembered: the next fjsp_env_regenerate_masked makes them as well, from its own
 * seed_base and whatever its mask says, and reports them in d_refreshed; a whole fjsp_env_regenerate makes all anyway.
 * A null handle: FJSP_E_ARG; a handle not made by a generated create: FJSP_E_STATE; both before the first HIP call. */
int  fjsp_env_regenerate_masked(fjsp_env *e, const uint8_t *d_mask, uint64_t seed_base, uint8_t *d_refreshed);
int  fjsp_env_instance_seed(const fjsp_env *e, int32_t i, uint64_t *seed);
/* Of the last create_generated / regenerate / regenerate_masked: out[0] instances, [1] LPs solved on the device, [2] on the host, [3] pivots
 * of the device simplex.  fjsp_env_generated_times: milliseconds of its parts -- the generate kernel, the LP launches with
 * their finish kernels, the host route, fluid tables + reset -- and of the whole call.  [0], [1], [3] are HIP-event times on the device route's
 * stream; [2] and [4] are host wall clock, and the host route runs beside the device's LPs, so [2] overlaps [1]: the parts
 * do not add up to [4].  (Five clock readings and four event records per call; tools/time_regenerate.py reads them.) */
int  fjsp_env_generated_stats(const fjsp_env *e, int64_t out[4]);
int  fjsp_env_generated_times(const fjsp_env *e, double out_ms[5]);
/* The same with the third LP route (FJSP_LP_IMPL=global): out[0..3] as fjsp_env_generated_stats ([1] counts the LDS simplex
 * alone), out[4] LPs solved by the global-memory simplex, out[5] its pivots ([3] holds both kernels' pivots);
 * out_ms[0..4] as fjsp_env_generated_times, out_ms[5] the global-memory LP launches with their finish kernels (HIP-event time on
 * their own stream: they run beside [1] and [2]).  out_ms is nullable. */
int  fjsp_env_generated_stats2(const fjsp_env *e, int64_t out[6], double out_ms[6]);
/* Instance i of a generated handle, read back from the device: dims as fjsp_instances_dims, the arrays as
 * fjsp_instances_get; every output nullable.  Synchronises. */
int  fjsp_env_instance_read(fjsp_env *e, int32_t i, int32_t dims[6], int32_t *Jr, int32_t *p, int32_t *elig_n,
                            int32_t *elig_list, int32_t *count, int32_t *arrive, int32_t *delivery, double *ddt, double *x);
void fjsp_env_destroy(fjsp_env *e);
int  fjsp_env_num_envs(const fjsp_env *e);
int  fjsp_env_state_size(const fjsp_env *e);   /* 20 (SO_FJSSP) / 18 (SO_SFJSP) / 25 (MO_FJSSP_discretes) / 30 (MO_DFJSP) */
int  fjsp_env_device(const fjsp_env *e);

/* reset(): SO_FJSSP.py:51-76.  d_mask (u8[N], nullable): reset only envs with
 * mask != 0.  d_state (f64[N][state_size], nullable) receives the state. */
int fjsp_env_reset(fjsp_env *e, const uint8_t *d_mask, double *d_state, void *stream);

/* step(action): SO_FJSSP.py:168-265.  d_actions u8[N][2] = (task rule, machine
 * rule) indices as the reference's action pair (:171-172); for the flat-action
 * variants (SO_SFJSP, MO_FJSSP_discretes) d_actions[..][0] is the flat action;
 * for the MO variant d_mo (f64[N][4] = w0, w1, completion,
 * tardiness; <=0 = None; nullable) carries step()'s extra arguments
 * (MO_FJSSP_discretes.py:88); for FJSP_VARIANT_MO_DFJSP d_mo is f64[N][4] =
 * reward_policy (0 makespan, 1 tardiness, 2 energy, 3 normalised sum),
 * completion, tardiness, energy_consumption (MO_DFJSP_breakdown.py:189,430-447;
 * NULL = policy 1; any other policy value sets FJSP_ST_BAD_TASK_RULE like the
 * reference's MyError).  Outputs (all nullable): d_state f64[N][S],
 * d_reward f64[N], d_done u8[N].  With d_state == NULL the step skips the
 * observation (state_extract, SO_FJSSP.py:78-97: a third of a step's work) -- for
 * callers that pick rules without looking at the state; the environment notes
 * that its remembered v(t-1) is stale and the next call that does return a state
 * rebuilds it first, so states stay identical to the reference's whatever the
 * mix of calls.  Envs already done are left untouched and get
 * FJSP_ST_STEP_AFTER_DONE unless autoreset != 0, in which case a done env is
 * reset first and the step applies to the fresh episode.  * d_actions must be 2-byte aligned (the kernels read an env's pair as one 16-bit word): FJSP_E_ARG otherwise. */
int fjsp_env_step(fjsp_env *e, const uint8_t *d_actions, const double *d_mo, int32_t autoreset,
                  double *d_state, double *d_reward, uint8_t *d_done, void *stream);
/* The same step, also reporting what the rule pair resolved to: d_trace_km
 * i16[N][2] (nullable) = the operation type index k (kind_task_tuple order) and
 * the machine m that task_select / machine_select chose (SO_FJSSP.py:173-174),
 * -1 / -1 for an env that did not step. */
int fjsp_env_step_traced(fjsp_env *e, const uint8_t *d_actions, const double *d_mo, int32_t autoreset,
                         double *d_state, double *d_reward, uint8_t *d_done, int16_t *d_trace_km, void *stream);

/* Asynchronous form of fjsp_env_step for batches with order arrivals (SO_FJSSP.py:218-231, class_MODFJSP.py:240-276:
 * an arrival re-solves the fluid LP on the host).  fjsp_env_step waits for those LPs inside every call; here an env
 * that reaches an arrival PARKS while the rest of the batch keeps stepping: its LP inputs travel to the host, a worker
 * pool solves them, and a later call uploads the solution and finishes the parked step (arrival_kernel).
 * d_ready u8[N]: 1 = this call completed a step of env i (d_state / d_reward / d_done row i are that step's), 0 = the
 * env is parked and its row is untouched.  WHICH ACTION A PARKED STEP APPLIES: the one presented in the call where the
 * env parked (the first call that returns ready = 0 for it) -- that call already ran the step up to the arrival.  Calls
 * made while it stays parked, and the call in which it resumes (ready = 1 again), do not look at its action at all: the
 * resumed row is the result of the action of the parking call.  A caller that records transitions must therefore keep
 * (state, action) of the parking call and pair them with the row that comes back with ready = 1; resampling a
 * stochastic policy for an env that shows ready = 0 has no effect on the environment.  An env's own trajectory is the
 * one fjsp_env_step produces for the sequence of its APPLIED actions (parity is per env); only the interleaving across
 * envs differs.  fjsp_env_arrivals_flush waits for every parked env and finishes its step (rows + ready = 1);
 * it must run before fjsp_env_step / _reset / _rollout / destroy are used on the batch again (they return
 * FJSP_E_STATE while envs are parked; so does fjsp_env_read).  fjsp_env_parked: parked envs as last seen by the host.
 * DEVIATION from the reference's protocol (a single-threaded reset()/step() object): this service
 * runs a dispatcher thread and a pool of LP worker threads inside the library for as long as the batch lives.  They touch
 * only the batch's own staging buffers, never call back into the caller and are joined by fjsp_env_destroy; a caller that
 * forks must do so before the first fjsp_env_step_async.  The blocking fjsp_env_step uses host threads only inside the
 * call (and none at all when the LPs run on the device, fjsp_env_lp_on_device).
 * The worker pool is built by the first fjsp_env_step_async of a batch and reads fjsp_env_set_lp_threads once, there:
 * call fjsp_env_set_lp_threads BEFORE the first fjsp_env_step_async for it to size the pool (later calls change only
 * the blocking service's thread count).
 * FJSP_ASYNC_RING=n (1 ... 32; unset or anything else: 32), read when the batch is created: how many launches' parked
 * envs the service keeps in flight at once.  A call that finds all n batches in flight waits for the oldest ones (their
 * LPs, upload and arrival_kernel) before it launches; trajectories do not depend on n, only the interleaving does.
 * n = 1 makes that wait deterministic -- every call after one that parked an env waits -- and is meant for tests.
 * fjsp_env_async_stats: host-side counters of the batch's asynchronous service since it was created (no device access,
 * no synchronisation): out[0] = launches whose parked envs (>= 1) were handed to the workers, out[1] = those of them
 * that parked more than 64 envs and fetched the rest with a second copy, out[2] = fjsp_env_step_async calls that found
 * no free batch and waited, out[3] = the most envs one launch parked.  All zero before the first fjsp_env_step_async
 * and on batches without order arrivals.  FJSP_E_ARG: a null argument. */
int fjsp_env_step_async(fjsp_env *e, const uint8_t *d_actions, const double *d_mo, int32_t autoreset, double *d_state,
                        double *d_reward, uint8_t *d_done, uint8_t *d_ready, void *stream);
int fjsp_env_arrivals_flush(fjsp_env *e, const double *d_mo, double *d_state, double *d_reward, uint8_t *d_done,
                            uint8_t *d_ready, void *stream);
int64_t fjsp_env_parked(const fjsp_env *e);
int fjsp_env_async_stats(const fjsp_env *e, int64_t out[4]);
/* Order-arrival LPs answered from the per-batch memo of (instance, Q, n_now) -> x (a pure function: same bits as a solve). */
int64_t fjsp_env_lp_cache_hits(fjsp_env *e);

/* T fused steps in ONE launch (rule-sweep harnesses, MO_DFJSP.py:481-518 style):
 * d_actions u8[T][N][2]; d_mo as in fjsp_env_step (constant over the T steps);
 * envs that finish early idle (no autoreset).
 * Trace outputs (nullable): d_trace_km i16[T][N][2] = chosen (k, m) or -1,
 * d_reward f64[T][N], d_state_last f64[N][S].  With d_state_last == NULL the
 * fused kernel skips the observation altogether (rule sweeps read makespan /
 * tardiness / energy only); as in fjsp_env_step the next call that returns a
 * state rebuilds the remembered v(t-1) first. */
int fjsp_env_rollout(fjsp_env *e, const uint8_t *d_actions, const double *d_mo, int32_t T, int16_t *d_trace_km,
                     double *d_reward, double *d_state_last, void *stream);

/* Read-back of the attributes agents / harnesses read, device
 * pointers, any may be NULL: delay_time_sum i64[N], makespan = max machine
 * time_end i32[N], completion_time i32[N], step_time i32[N], step_count i32[N],
 * done u8[N], status u32[N] (FJSP_ST_* bits, sticky until reset). */
int fjsp_env_read(fjsp_env *e, int64_t *d_delay_time_sum, int32_t *d_makespan, int32_t *d_completion,
                  int32_t *d_step_time, int32_t *d_step_count, uint8_t *d_done, uint32_t *d_status,
                  void *stream);
/* machine_dict[m].time_end: i32[N][M_max] (SO_FJSSP.py:426). */
int fjsp_env_machine_time_end(fjsp_env *e, int32_t *d_tend, int32_t m_stride, void *stream);
/* energy_consumption i64[N] of a FJSP_VARIANT_MO_DFJSP batch (MO_DFJSP_breakdown.py:253-256). */
int fjsp_env_energy(fjsp_env *e, int64_t *d_energy, void *stream);
/* The dispatched schedule (SO_FJSSP.py:176-196: task.time_begin / machine / time_end and machine.task_list, with the
 * breakdown shifts of MO_DFJSP_breakdown.py:203-247).  While recording is on, every dispatch -- fjsp_env_step(_traced),
 * fjsp_env_step_async (in the call where the step dispatched, before it parks), fjsp_env_rollout and
 * fjsp_env_rollout_policy, both kernel families -- stores one 16-byte record in slot step_count of its env; the plain
 * kernels run while it is off.  The table always holds each env's CURRENT episode: after a step that returns done it
 * holds the finished one until the env is reset, explicitly or by autoreset at its next step, so callers that use
 * autoreset read it after the done step.
 *
 * fjsp_env_record_schedule: on != 0 allocates the [cap][N] record table (cap = operations of the largest instance of the
 * batch, sum over orders and kinds of count[s][r] * J_r, orders that arrive later included) and selects the recording
 * kernels; on == 0 frees it.  FJSP_E_STATE if any env is mid-episode (call after create or when every env is done).
 * Synchronises the device first, so steps still queued on any stream are taken into account. */
int fjsp_env_record_schedule(fjsp_env *e, int32_t on);
/* cap (slots per env), 0 when recording is off. */
int fjsp_env_schedule_capacity(const fjsp_env *e);
/* SO_FJSSP.py:182-184 per dispatched operation: d_table i32[N][cap][6] = (r, j, n, m, time_begin, time_end) in dispatch
 * order -- kind r, stage j, job number n within kind r (counted over all orders, class_FJSSP.py:212-216), machine m --
 * and -1 past d_len[i]; d_len i32[N] (nullable) = the env's step_count.  Stream-ordered, no host synchronisation.
 * FJSP_E_STATE when recording is off or envs are parked at an order arrival (fjsp_env_arrivals_flush first). */
int fjsp_env_schedule(fjsp_env *e, int32_t *d_table, int32_t *d_len, void *stream);
/* ------------------------------------------------------------------------- *
 * Saved environment states (csrc/fjsp_snapshot.hip): copy, rewind and branch episodes on the device
 * ------------------------------------------------------------------------- */
typedef struct fjsp_snapshot fjsp_snapshot;

/* A snapshot holds n entries; an entry is one env's whole record (the episode state the kernels keep per env) and, if
 * the snapshot was created while `e` was recording its schedule, the env's dispatch records.  It is bound to e's
 * FINGERPRINT, not to e: the record layout, the shape fields of the batch (operation / machine / job paddings, variant,
 * kernel family, number of instances) and a hash of the packed instance slab.  Any batch with the same fingerprint --
 * the same instances played by the same variant and kernel family, whatever its N -- may save into it and load from
 * it; any other batch gets FJSP_E_ARG.
 * Save and load are stream-ordered, do not synchronise with the host and can be captured in a graph.  Both return
 * FJSP_E_STATE while envs are parked in the asynchronous arrival service (fjsp_env_arrivals_flush first) and once the
 * batch's arrival service has failed.
 * RANDOM RULES: an env draws random.choice from the stream of its SLOT (rng_seed + env * 1000003, with the draw counter
 * in its record).  An entry loaded into another slot, or into a batch with another rng_seed or first env, continues on
 * that slot's stream: only a load into the same global env id replays the random rules bit for bit.  Deterministic
 * rules replay exactly wherever the entry is loaded.
 *
 * fjsp_snapshot_create: n entries, sized for e's layout, plus cap dispatch records per entry if e records at that
 * moment (fjsp_env_record_schedule). */
int  fjsp_snapshot_create(const fjsp_env *e, int32_t n, fjsp_snapshot **out);
void fjsp_snapshot_destroy(fjsp_snapshot *s);
int  fjsp_snapshot_size(const fjsp_snapshot *s);        /* n */
int  fjsp_snapshot_capacity(const fjsp_snapshot *s);    /* dispatch-record slots per entry, 0 = none */
/* entry q <- env d_idx[q] of e (d_idx i32[n], device; NULL: envs 0..n-1, FJSP_E_ARG if n > N), with its dispatch
 * records when e records and s has room for them.  An entry remembers its instance (env % n_inst); an index outside
 * [0, N) leaves an entry that every load refuses and counts as an error (fjsp_snapshot_errors). */
int fjsp_snapshot_save(fjsp_snapshot *s, fjsp_env *e, const int32_t *d_idx, void *stream);
/* env i <- entry d_src[i] for every i with d_src[i] >= 0 (d_src i32[N], device, -1 = keep env i; NULL: entry i for
 * i < n).  The kernel refuses an entry saved from another instance than i % n_inst (or an index >= n): env i is left
 * untouched and the snapshot's device error counter grows.  Nothing is ever written into an env of another instance.
 * If e records its schedule the entries' dispatch records are loaded too; FJSP_E_STATE if the last save into s was
 * from a batch that did not record (s holds no records).  A snapshot with records loads into a batch that does not
 * record; the records are then ignored. */
int fjsp_snapshot_load(fjsp_snapshot *s, fjsp_env *e, const int32_t *d_src, void *stream);
/* Synchronises the device, returns the number of loads refused since the last call (and of bad save indices) in
 * *count, and clears the counter. */
int fjsp_snapshot_errors(fjsp_snapshot *s, int64_t *count);
/* Serialised form (pickling): h_out == NULL -> *nbytes = the size needed; otherwise copies the fingerprint and the
 * buffer into h_out (*nbytes: its size in, the size written out).  Synchronises the device first.
 * fjsp_snapshot_from_host: a new snapshot on e's device from those bytes; FJSP_E_ARG unless e has the fingerprint the
 * bytes were saved with. */
int fjsp_snapshot_to_host(fjsp_snapshot *s, void *h_out, int64_t *nbytes);
int fjsp_snapshot_from_host(const fjsp_env *e, const void *h_in, int64_t nbytes, fjsp_snapshot **out);

/* fluid tables of env i copied to host (tests): rate/arr [K*M] k-major, rate_sum/time_sum [K]. */
int fjsp_env_fluid_tables(fjsp_env *e, int32_t i, double *h_rate, double *h_arr,
                          double *h_rate_sum, double *h_time_sum);
/* Test hook (host build of csrc/fjsp_pyset.h, the code machine_select runs on the
 * device): iteration order of list(set(idle) & set(machines)) as CPython 3.10
 * produces it (SO_FJSSP.py:302-303).  idle_mask bit m = machine m idle;
 * machines[n] in tuple order (ascending != 0: inserted in ascending order).
 * Writes the order to out[], returns its length (or a negative error). */
int fjsp_pyset_and_order(uint32_t idle_mask, const int32_t *machines, int32_t n, int32_t ascending, int32_t *out);
/* HBM bytes the step kernel reads+writes per env-step (algorithmic). */
int64_t fjsp_env_step_bytes(const fjsp_env *e);
/* Which kernel family steps this batch: 0 = one wavefront per environment (csrc/fjsp_kernels.hip: every variant and
 * shape), 1 = one 16-lane row per environment (csrc/fjsp_group.hip: SO_FJSSP / SO_DFJSP / MO_FJSSP_discretes batches of
 * one job per kind, one order, <= 64 operation types, <= 8 machines, <= 15 jobs -- the reference's 10x5 and Brandimarte
 * shapes).  Same results either way; the environment variable FJSP_STEP_IMPL=wave at create time forces 0 (create is
 * where the library reads every FJSP_* variable: what they decide stays with the handle). */
int fjsp_env_kernel_family(const fjsp_env *e);
/* Which build of the row kernels a launch of this batch runs (kernel family 1): decided once, when the batch is created,
 * and stored in the handle, from where the launchers take it and this call reports it: out3 = {early, mpc, resident} of the per-step launch (fused = 0: fjsp_env_step and its kin) or
 * of the fused launch (fused = 1: fjsp_env_rollout).  early: 1 = the small-batch build that requests everything at the top
 * of a step, 0 = the register-lean build; mpc: the machine capacity the kernels were compiled for (5 or 8); resident: 1 =
 * the fused kernel keeps the instance's static tables in LDS (always 0 for fused = 0).  FJSP_GROUP_EARLY /
 * FJSP_GROUP_RESIDENT, as set when the batch was created, are included.  FJSP_E_UNSUPPORTED for a batch of the one-wave-per-environment family. */
int fjsp_env_row_build(const fjsp_env *e, int32_t fused, int32_t *out3);
/* Order arrivals (SO_FJSSP.py:218-231) re-solve the fluid LP on the host, one LP per arriving env, spread
 * over n_threads host threads (0 = default: min(host cores, 16)).  fjsp_env_lp_solves: LPs solved so far. */
int fjsp_env_set_lp_threads(fjsp_env *e, int32_t n_threads);
int64_t fjsp_env_lp_solves(const fjsp_env *e);
/* Where the order-arrival LPs of this batch are solved: 1 = on the device (csrc/fjsp_lp_device.hip; csrc/fjsp_lp_simplex.h: the host simplex of
 * csrc/fjsp_lp.cpp restated pivot for pivot, one workgroup per parked environment, tableau in LDS; fjsp_env_step then never
 * synchronises), 0 = on the host.  Same x either way, bit for bit.  Chosen at create time: the device when the largest tableau
 * of the batch fits a CU's LDS (and is at most 512 columns wide) and the batch has 16384 environments or more -- a single LP is
 * ~6x slower on the device than on a host core, 256 run at once: below that size the host service with its cache of solved
 * LPs is as fast or faster (DESIGN.md has the measurements).  FJSP_LP_IMPL=device / host at create time overrides the size rule.
 * fjsp_env_lp_device_solve (test hook): the device solver on one LP of env's instance -- Q[K], n_now[K] as
 * class_FJSSP.py:234-237 builds them -- x f64[K*M] (k-major) to the host; the batch must have no parked environments.
 * The device stages both as 16-bit counts: a Q[k] or n_now[k] outside 0 ... 65535 is FJSP_E_ARG (never a truncated value);
 * Q[k] = 0 is FJSP_E_LP, as the host solver refuses it, and leaves the handle usable.
 * FJSP_LP_IMPL=global (opt-in): as =device when every tableau fits the LDS rule; otherwise, when every tableau of the batch
 * stays within 256 rows x 1536 columns, 2 = the same service with the simplex of csrc/fjsp_lp_global.hip, whose tableau lives
 * in a scratch pool in global memory (min(n_envs, 256, max(1, 512 MiB / slot)) slots of fjsp_lp_global_bytes each,
 * allocated at create by such a handle alone); otherwise the host.  The test hook, the counters and the error reporting
 * work on such a handle as on 1.
 * fjsp_lp_global_bytes: the slot bytes of the largest tableau an instance of K operation types, M machines, nx eligible
 * pairs and R kinds can need -- (2K + M - R) rows x (nx + 2K + M - R + 2) columns of f64, rounded up to 256 --, or 0 when
 * it has more than 256 rows or 1536 columns (or the arguments make no instance).  Host arithmetic, no HIP call. */
int fjsp_env_lp_on_device(const fjsp_env *e);
int64_t fjsp_lp_global_bytes(int32_t K, int32_t M, int32_t nx, int32_t R);
/* Pivots the device simplex has executed so far, all LPs together (0 when the batch keeps the host service; synchronises). */
int64_t fjsp_env_lp_device_pivots(const fjsp_env *e);
int fjsp_env_lp_device_solve(fjsp_env *e, int32_t env, const int32_t *Q, const int32_t *n_now, double *x);

/* ------------------------------------------------------------------------- *
 * Rollout buffer (on-policy Replay_Buffer, agents/MPPPO/Buffer.py:7-58) in HBM
 * ------------------------------------------------------------------------- */
typedef struct fjsp_rollout fjsp_rollout;

/* Capacity T steps x N envs x state_size; storage f32 like Buffer.py:41-45. */
int  fjsp_rollout_create(int32_t T, int32_t N, int32_t state_size, int32_t device, fjsp_rollout **out);
void fjsp_rollout_destroy(fjsp_rollout *b);
/* add_experience (Buffer.py:19-28): converts the f64 env outputs of one
 * batched step to f32 rows at the write cursor t. `d_active` u8[N] (nullable)
 * = envs that were not done before the step (valid-row mask). */
int fjsp_rollout_append(fjsp_rollout *b, const double *d_state, const uint8_t *d_actions,
                        const double *d_reward, const double *d_next_state, const uint8_t *d_done,
                        const uint8_t *d_active, void *stream);
/* calculate_discounted_returns (agents/MPPPO/MPPPO.py:301-312): reverse scan
 * G_t = r_t + gamma * G_{t+1} per env over valid rows, f64 scan -> f32. */
int fjsp_rollout_returns(fjsp_rollout *b, double gamma, void *stream);
/* The same scan followed by the per-episode normalisation of MPPPO.py:258-261 (normalized: (G - min) / (max - min +
 * 1e-8) over the env's valid rows; standardized: (G - mean) / (unbiased std + 1e-8)) in one launch; d_out
 * f32[len][N] receives the result (0 in rows that are not valid), the buffer's returns the raw scan. */
int fjsp_rollout_returns_normalised(fjsp_rollout *b, double gamma, int32_t normalized, int32_t standardized, float *d_out, void *stream);
/* clear(): Buffer.py:53-55 */
int fjsp_rollout_clear(fjsp_rollout *b);
int fjsp_rollout_len(const fjsp_rollout *b);
/* Device pointers into the buffer (wrapped zero-copy by the PyTorch side):
 * which = 0 states f32[T][N][S], 1 actions f32[T][N][2], 2 rewards f32[T][N],
 * 3 next_states f32[T][N][S], 4 dones f32[T][N], 5 valid f32[T][N], 6 returns f32[T][N]. */
void *fjsp_rollout_ptr(fjsp_rollout *b, int32_t which);

/* The actor of the on-policy agents (ActorNet, agents/MPPPO/MPPPO.py:31-48) at the size of BASELINE config 3:
 * state_size -> 128 -> 128 -> n_actions, Linear + ReLU twice, Linear, softmax.  Device pointers to the f32
 * parameters in torch's layout (weight[out][in] row-major): what nn.Linear holds.  state_size <= 32, hidden == 128,
 * n_actions <= 32. */
typedef struct fjsp_actor_params {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    int32_t state_size, hidden, n_actions;
} fjsp_actor_params;

/* ActorNet.forward (MPPPO.py:44-48) for n states: d_state f64[n][state_size] (converted with `.float()` like
 * MPPPO.py:274) -> d_probs f32[n][n_actions].  The same device code the fused rollout below evaluates in place. */
int fjsp_actor_forward(const fjsp_actor_params *actor, const double *d_state, int32_t n, float *d_probs, void *stream);

/* run_one_policy_network's rollout loop (MPPPO.py:245-252: pick_action_and_log_prob, env.step, save_experience)
 * for T vector steps in ONE launch: the actor is evaluated inside the environment kernel, actions are drawn from
 * the stream of fjsp_policy_sample (same *d_seed, counter = step index: the same actions as the per-step path
 * actor -> fjsp_policy_sample -> fjsp_env_step, bit for bit), and every step's row goes straight into `buf`
 * (as fjsp_rollout_append writes it; rows of envs that had finished are marked invalid, buf's length becomes T).
 * d_state_in f64[N][S]: the states the rollout starts from (what fjsp_env_reset returned); d_flat_actions /
 * d_log_prob f32[T][N]: the sampled action index and its log-probability; d_state_last f64[N][S] receives every
 * env's latest state.  d_mo as in fjsp_env_step.  Every single-order batch that create admits, whatever its operation
 * types (up to 256) and jobs: the workgroup holds as many environments as fit a CU's LDS beside the actor's weights
 * (fjsp_env_policy_build).  FJSP_E_UNSUPPORTED for a batch with order arrivals (their LPs are served between launches) and
 * for an actor of another shape (callers fall back to the per-step loop). */
int fjsp_env_rollout_policy(fjsp_env *e, fjsp_rollout *buf, const fjsp_actor_params *actor, const float *d_epsilon,
                            const uint64_t *d_seed, int32_t pair_div, int32_t T, const double *d_mo, const double *d_state_in,
                            float *d_flat_actions, float *d_log_prob, double *d_state_last, void *stream);

/* Decoding a trained actor (MPPPO.py:245-252 without the buffer, the action of pick_action_and_log_prob :272-284):
 * every env plays from its current state to the end of its episode in ONE launch, the actor inside the environment
 * kernel.  Envs [0, n_greedy) take the first index of the largest probability (torch.argmax over the probabilities
 * fjsp_actor_forward returns); the others draw from the stream of fjsp_policy_sample with epsilon 0 (same *d_seed,
 * counter = step index within this call, env = local index).  An action a is applied as (a / pair_div, a % pair_div),
 * or (a, 0) when pair_div == 0.  d_first u8[N][2] (nullable): the action step 0 applies instead, in the env encoding.
 * Env i starts from row d_state_src[i] of d_state_in f64[n_state_in][S] (d_state_src i32[N] nullable: row i); the
 * rows must be the envs' current states, and d_state_in may be d_state_last only without a map.  An env stops once it
 * is done or carries FJSP_ST_BAD_TASK_RULE / BAD_MACHINE_RULE / NO_EVENT; T (steps, > 0) is an upper bound.
 * Outputs: d_actions_out u8[T][N][2] (nullable) the action applied at each step, rows past an env's end untouched;
 * d_steps_out i32[N] the steps each env took; d_state_last f64[N][S], d_reward_last f64[N], d_done_last u8[N] the
 * state, reward and done flag after each env's last step (an env that took none: its start row, reward untouched).
 * FJSP_E_ARG: null env or output, T <= 0, n_greedy < 0, null d_state_in, pair_div < 0 or not dividing n_actions,
 * null d_seed while an env samples, fewer than N rows without a map.  FJSP_E_UNSUPPORTED where
 * fjsp_env_rollout_policy refuses (actor not state_size <= 32 -> 128 -> 128 -> n_actions <= 32, order arrivals):
 * callers fall back to the per-step loop.  Recording batches record the schedule. */
int fjsp_env_play_policy(fjsp_env *e, const fjsp_actor_params *actor, int32_t pair_div, int32_t n_greedy, const uint64_t *d_seed,
                         int32_t T, const double *d_mo, const double *d_state_in, int32_t n_state_in, const int32_t *d_state_src,
                         const uint8_t *d_first, uint8_t *d_actions_out, int32_t *d_steps_out, double *d_state_last,
                         double *d_reward_last, uint8_t *d_done_last, void *stream);

/* The workgroup fjsp_env_rollout_policy and fjsp_env_play_policy run for this batch with an actor of `state_size` inputs
 * (1..32): out3 = {environments per workgroup (one wavefront each: 16, 8, 4, 2 or 1 -- the most whose LDS slices fit the
 * 160 KB of a CU beside the actor's weights), dynamic LDS bytes of the workgroup, chunks of 64 operation types}.  Decided
 * by the function the two launches decide with.  FJSP_E_UNSUPPORTED, with the text the launches give, for a batch they
 * refuse (order arrivals; a slice that fits no workgroup, which create's own LDS limit rules out); FJSP_E_ARG for a null
 * argument or a state_size outside 1..32. */
int fjsp_env_policy_build(const fjsp_env *e, int32_t state_size, int32_t *out3);

/* The two calls above on a batch WITH order arrivals (SO_FJSSP / SO_DFJSP instances of more than one order), which the
 * one-launch entries refuse: same arguments, same outputs, same actions as the per-step path bit for bit.  The episode
 * is played in segments: a policy launch runs every env until it finishes, reaches T or meets an order arrival; the
 * arrival service (the one fjsp_env_step runs: LP on the device or on the host, then arrival_kernel) finishes the steps
 * that met one, and the next launch goes on from there -- at most S_max launches and S_max - 1 services for a batch whose
 * instances have up to S_max orders, all on `stream`.  With the LPs on the device nothing synchronises; the host LP
 * service synchronises as it does in fjsp_env_step, and the call stops at the first launch in which no env parked.
 * Between segments the play's progress is d_steps_out, the rollout's is scratch owned by the handle.  A failed service
 * marks the handle failed, as in fjsp_env_step.
 * FJSP_E_UNSUPPORTED, fjsp_last_error() saying why: a batch without order arrivals (use the one-launch entry), a
 * FJSP_VARIANT_MO_DFJSP batch (its 12 x 10 actions do not fit the in-kernel actor), an actor of another shape than
 * state_size <= 32 -> 128 -> 128 -> n_actions <= 32, a slice that fits no workgroup.  FJSP_E_ARG as the one-launch entries. */
int fjsp_env_rollout_policy_orders(fjsp_env *e, fjsp_rollout *buf, const fjsp_actor_params *actor, const float *d_epsilon,
                                   const uint64_t *d_seed, int32_t pair_div, int32_t T, const double *d_mo, const double *d_state_in,
                                   float *d_flat_actions, float *d_log_prob, double *d_state_last, void *stream);
int fjsp_env_play_policy_orders(fjsp_env *e, const fjsp_actor_params *actor, int32_t pair_div, int32_t n_greedy, const uint64_t *d_seed,
                                int32_t T, const double *d_mo, const double *d_state_in, int32_t n_state_in, const int32_t *d_state_src,
                                const uint8_t *d_first, uint8_t *d_actions_out, int32_t *d_steps_out, double *d_state_last,
                                double *d_reward_last, uint8_t *d_done_last, void *stream);
/* fjsp_env_policy_build for the two: out4 = {environments per workgroup, dynamic LDS bytes, chunks of 64 operation types,
 * segments = the largest order count of the batch's instances (a generated handle: of its generator's range)}. */
int fjsp_env_policy_orders_build(const fjsp_env *e, int32_t state_size, int32_t *out4);

/* pick_action_and_log_prob (agents/MPPPO/MPPPO.py:272-284) for one vector step in ONE launch: samples
 * Categorical(d_probs[env]) (f32[n][n_actions], the actor's softmax output), applies the epsilon-random
 * override (*d_epsilon, device scalar so that captured graphs can change it), and writes the flat action
 * (d_action f32[n]), its log-probability (d_log_prob f32[n]) and the action in the environment's encoding
 * (d_pair u8[n][2] = (a / pair_div, a % pair_div), or (a, 0) when pair_div == 0).  Random numbers are a
 * counter-based function of (*d_seed, counter, env). */
int fjsp_policy_sample(const float *d_probs, int32_t n, int32_t n_actions, int32_t pair_div, const float *d_epsilon,
                       const uint64_t *d_seed, uint64_t counter, uint8_t *d_pair, float *d_action, float *d_log_prob,
                       void *stream);

/* The selection step of a beam search (policy_search.beam_search; csrc/fjsp_beam.hip) for n_src source envs in ONE
 * launch, one wavefront per source env.  d_cost f64[width_in][n_src][n_actions], beam-major like every branch batch
 * (beam b of source env i is branch env b * n_src + i): entry (b, i, a) is the cost of applying action a in beam b of
 * source env i, lower is better; a NaN or +inf entry is not a candidate.  d_done u8[width_in][n_src] (nullable:
 * nothing done): a done beam has exactly one candidate, (b, action -1) with cost d_cost[b][i][0]; its other entries
 * are ignored whatever they hold.  Outputs, all [width_out][n_src]: d_parent / d_action i32 and d_cost_out f64 = the parent beam, the
 * action and the cost (the input's bits) of source env i's k-th candidate in ascending cost, equal costs by lower
 * parent, then lower action; -0.0 and 0.0 are equal.  Ranks beyond the number of candidates: parent -1, action -1,
 * cost +inf.  The costs are compared and never computed with: the result is a function of the input bits.
 * Stream-ordered, no host synchronisation, capturable.  FJSP_E_ARG before any device call: a null d_cost or output,
 * n_src < 1, width_in or width_out outside 1..64, n_actions outside 1..128 (MO_DFJSP has 120 actions). */
int fjsp_beam_select(const double *d_cost, const uint8_t *d_done, int32_t n_src, int32_t width_in, int32_t n_actions,
                     int32_t width_out, int32_t *d_parent, int32_t *d_action, double *d_cost_out, void *stream);

/* The Pareto front of every source env's candidates (pareto.select; csrc/fjsp_pareto.hip; the reference's
 * filter_pareto_front, utilities/Utility_Class.py:132-146) for n_src source envs in ONE launch.  d_obj
 * f64[n_cand][n_src][n_obj], candidate-major like every branch batch (candidate c of source env i is branch env
 * c * n_src + i); lower is better in every objective.  d_valid u8[n_cand][n_src] (nullable: every candidate valid).  A
 * candidate with valid == 0 or with a NaN in any objective is not a candidate; the infinities are ordinary values under
 * IEEE comparison; -0.0 and 0.0 are equal.  Candidate c is on the front iff no candidate j has obj[j] <= obj[c] in
 * every objective and < in at least one, and no candidate j < c has the same objective vector (of equal points the
 * lowest index survives).  Outputs: d_index i32[n_src][cap] = the front members' candidate indices in ascending
 * lexicographic order of their objective vectors, objective 0 most significant (np.unique(axis=0)'s order), -1 past
 * the front; d_count i32[n_src] = the true front size, which may exceed cap (d_index then holds the first cap
 * members); d_mask u8[n_cand][n_src] (nullable) = 1 on the front.  The values are compared and never computed with;
 * no atomics: the result is a function of the input bits.  Stream-ordered, no host synchronisation, capturable.
 * FJSP_E_ARG before any device call: a null d_obj, d_index or d_count, n_src < 1, n_cand outside 1..1024, n_obj
 * outside 1..4, cap outside 1..n_cand. */
int fjsp_pareto_select(const double *d_obj, const uint8_t *d_valid, int32_t n_src, int32_t n_cand, int32_t n_obj,
                       int32_t cap, int32_t *d_index, int32_t *d_count, uint8_t *d_mask, void *stream);

/* Explicit schedules decoded on the device (schedule.decode, policy_search.improve; csrc/fjsp_decode.hip): an operation
 * sequence with a machine per operation -> its times and objectives, n_cand candidates per env in ONE decode launch.
 * Candidate (i, q), i < N, q < n_cand, is decoded on the instance of env i (instance i % n_inst, as resident on the
 * device: operation counts, processing times, order counts and arrivals, due dates); no env's episode state is read or
 * changed.  Stream-ordered, no host synchronisation (a handle's first call allocates its 8 (KP + 1) bytes per instance).
 *
 * d_plan i32[N][q_plans][cap][3]: rows (r, n, m) -- kind, job number within the kind counted over all orders
 * (class_FJSSP.py:212-216), machine -- in sequence order, the plan ends at its first row of three -1 (or at cap); q_plans
 * is 1 (the env's candidates share one parent plan) or n_cand.  The stage of a row is implied: the t-th row of job (r, n) is
 * its stage t.  d_moves (nullable) i32[N][n_cand][3] = (kind, u, m_new), applied while the plan is read: 0 nothing; 1 row
 * u runs on machine m_new; 2 rows u and u + 1 change places (nothing if they are rows of one job); 4, with the third
 * field dv | dw << 16, v = u + dv, w = u + dw, 1 <= dv <= 65535, 0 <= dw < dv, dw <= 32767 (the field is a non-negative
 * int32; a plan has at most 65535 rows, so dv always fits): rows u and v leave their places and stand, v first,
 * directly behind old row w -- old rows 0 .. u-1, u+1 .. w, v, u, w+1 .. v-1, v+1 .. (dw = 0 puts v in front of u,
 * dw = dv - 1 puts u behind v; no same-job exception).  3 is no kind.
 *
 * Decoding (SO_FJSSP.py:176-196 without the event clock): a job is ready at its order's arrival
 * (class_FJSSP.py:212-218 numbers the jobs of a kind across the orders), a machine is free at 0; row by row time_begin =
 * max(ready, free), time_end = time_begin + p[k][m], and both become time_end.  32-bit integers, exact.
 *
 * d_objective i64[N][n_cand][2] = (latest time_end, total tardiness of the last stages against the due dates the env
 * uses, class_FJSSP.py:214-218 / the order's delivery time for SO_DFJSP); d_status i32[N][n_cand]; d_table (nullable)
 * i32[N][n_cand][cap][6] in fjsp_env_schedule's format, -1 past d_len; d_len (nullable) i32[N][n_cand].
 * Status per candidate: 0 decoded; 1 a row names no job of the instance; 2 a job has more rows than stages, or the plan
 * ends with operations missing; 3 machine out of range or not eligible (p = 0); 4 bad move (unknown kind, or u -- for a
 * swap u + 1, for kind 4 v -- outside the plan, or a third field of kind 4 that is negative or has dv < 1 or dw >= dv).  4 outranks the others, else the first failing row in sequence order decides, a row's
 * checks in the order 1, 2, 3.  A failed candidate has objective -1, length 0 and a table of -1; every check is an
 * ordinary bounds-checked path and the other candidates are not affected.
 *
 * Limit: a candidate's state is 5 bytes per job of the batch's largest instance (jobs rounded up to 16) + 4 per machine
 * (of the largest), and 32 candidates must fit the 160 KB of a CU's LDS: at most 5120 bytes per candidate.  That admits the
 * reference's training distribution (12 kinds x 50 jobs, 20 machines: 3120 bytes) and every instance the environments take
 * up to about 1000 jobs.  fjsp_schedule_decode_group: the candidates one workgroup decodes (256, 128, 64 or 32), 0 where
 * the state does not fit or the batch is MO_DFJSP.
 * FJSP_E_ARG: a null e, d_plan, d_objective or d_status, n_cand < 1, q_plans neither 1 nor n_cand, N * n_cand >= 2^31.
 * FJSP_E_UNSUPPORTED: FJSP_VARIANT_MO_DFJSP (breakdown shifts and energy: fjsp_schedule_decode_dyn decodes those), a
 * state beyond the limit.
 * FJSP_E_STATE: a generated handle whose last regenerate failed. */
int fjsp_schedule_decode(fjsp_env *e, const int32_t *d_plan, int32_t q_plans, const int32_t *d_moves, int32_t n_cand,
                         int64_t *d_objective, int32_t *d_status, int32_t *d_table, int32_t *d_len, void *stream);
/* rows per plan = fjsp_env_schedule_capacity's cap (operations of the batch's largest instance), recording on or off */
int fjsp_schedule_decode_capacity(const fjsp_env *e);
int fjsp_schedule_decode_group(const fjsp_env *e);

/* Explicit schedules decoded ACTIVELY on the device (schedule.decode_active, policy_search.left_shift;
 * csrc/fjsp_decode.hip): fjsp_schedule_decode with insertion into machine gaps, the decoder the FJSP literature uses for
 * operation-sequence chromosomes.  Everything not said here is fjsp_schedule_decode's, unchanged: the plans, q_plans and
 * the moves (kinds 0, 1, 2, 4) applied while the plan is read; the status codes 0 to 4 and their precedence; a failed
 * candidate (objective -1, length 0, a table of -1, the others unaffected); d_objective i64[N][n_cand][2]; d_table rows
 * written AT THEIR PLAN POSITION t (not in begin order), -1 past d_len; the limit on a candidate's state and the group
 * size; FJSP_E_ARG and FJSP_E_STATE; stream order, no host synchronisation, no atomics.
 *
 * Decoding.  Jobs are ready at their order's arrival.  Every machine has an empty list of busy intervals, kept in
 * ascending begin order.  For plan row (r, n, m), with stage the job's next stage and k its operation type, d = p[k][m]
 * and s = ready[job]; machine m's intervals (b, e) are walked from the first:
 *     s + d <= b    the row takes [s, s + d) in front of that interval (touching is allowed) and the walk stops;
 *     else          s = max(s, e) and the walk goes on;
 * past the last interval the row takes [s, s + d).  Then ready[job] = s + d; makespan and tardiness as
 * fjsp_schedule_decode.  32-bit integers, exact.  Every row ends no later than in fjsp_schedule_decode's table of the same
 * plan (induction over the rows: appending behind the machine's latest interval is always available, and that interval
 * ends at or before the semi-active free[m]), so no clock exceeds its semi-active value and the bound of fjsp_env_create
 * that keeps those below 2^31 covers this entry.
 * The result is an active schedule.  Sorting the table's rows stably by begin (schedule.begin_order) gives a plan that
 * fjsp_schedule_decode decodes to the same table row for row, and that this entry decodes to it with nothing inserted.
 *
 * d_inserted (nullable) i32[N][n_cand]: the rows placed in front of at least one interval already on their machine; 0
 * for a failed candidate.  Where it is 0 the table is fjsp_schedule_decode's.
 *
 * One path for every plan size: a candidate's intervals live in a device workspace that the handle owns, 8 bytes per plan
 * row (begin, duration | predecessor on the machine), allocated by the handle's first call and never cleared -- a
 * candidate reads only entries it wrote itself.  The grid is bounded: groups = min(FJSP_DECODE_ACTIVE_MAX_GROUPS, max(1,
 * FJSP_DECODE_ACTIVE_WORKSPACE_BYTES / (8 cap G))) workgroups of G = fjsp_schedule_decode_group candidates loop over the
 * call's ceil(N n_cand / G) groups, so groups x G candidates are resident at once (fjsp_schedule_decode_active_resident)
 * and the workspace is 8 cap G groups bytes (cap = fjsp_schedule_decode_capacity) whatever N and n_cand are; entry i of
 * the candidates of a workgroup are G consecutive 8-byte words.  ORDERING: the calls on one handle share the workspace,
 * fjsp_schedule_evolve_active's among them, so they must be ordered on one stream (or by events); calls on different
 * handles are independent.
 * fjsp_schedule_decode_active_group: G, 0 where fjsp_schedule_decode_group is 0.
 * FJSP_E_UNSUPPORTED: FJSP_VARIANT_MO_DFJSP (an insertion under breakdown shifts is not defined by the reference), a
 * state beyond fjsp_schedule_decode's limit.  FJSP_E_HIP: the workspace could not be allocated. */
#define FJSP_DECODE_ACTIVE_WORKSPACE_BYTES (128 * 1024 * 1024)
#define FJSP_DECODE_ACTIVE_MAX_GROUPS 512
int fjsp_schedule_decode_active(fjsp_env *e, const int32_t *d_plan, int32_t q_plans, const int32_t *d_moves, int32_t n_cand,
                                int64_t *d_objective, int32_t *d_status, int32_t *d_table, int32_t *d_len, int32_t *d_inserted,
                                void *stream);
int fjsp_schedule_decode_active_group(const fjsp_env *e);
int fjsp_schedule_decode_active_resident(const fjsp_env *e);

/* Explicit schedules of MO_DFJSP decoded on the device (schedule.decode_dyn, policy_search.improve on such a batch;
 * csrc/fjsp_decode.hip): fjsp_schedule_decode with the machines' breakdown windows and the third objective, energy.
 * Arguments, plans, moves, the checks, the status codes 0 to 4, d_table, d_len and the handling of a failed candidate are
 * fjsp_schedule_decode's, unchanged; d_objective is i64[N][n_cand][3] = (latest time_end, total tardiness, energy), all
 * -1 on failure.  Plan capacity: fjsp_schedule_decode_capacity.
 *
 * Decoding (MO_DFJSP_breakdown.py:203-256 without the event clock).  Jobs are ready at their order's arrival, machines
 * are free at 0 and have no last task.  Then per plan row (r, n, m), with stage the job's next stage and k its operation
 * type:
 *   d = p[k][m], t = max(ready[job], free[m]); begin = t, end = machine_end = t + d.
 *   Machine m's windows (bs, be) are walked in file order from the first, t fixed, end as it stands at that window:
 *     bs <= t < be        begin += be - t, end += be - t, machine_end = end   (dispatched inside the window)
 *     else t < bs < end   end += be - bs, machine_end = end                   (the window interrupts the operation)
 *     else bs == end      machine_end += be - bs                              (the table's end does not move)
 *     else bs > end       the walk stops.
 *   energy += power[k][m] * d; if the machine had a task before, energy += (t - last_end[m]) * idle_power[m] -- the gap
 *   is measured to the dispatch time t, not to the shifted begin; then last_end[m] = end.
 *   ready[job] = free[m] = machine_end: the job's next stage waits for the machine's end too (the reference re-queues the
 *   job when machine.time_end is reached).
 *   makespan = max(makespan, end); at a job's last stage tardiness += max(0, end - due), due = the order's delivery time
 *   (class_MODFJSP.py:224).  The table row is (r, stage, n, m, begin, end).
 * This is the schedule the environment dispatches when every operation is dispatched at max(ready, free): it returns a
 * recorded single-order episode's table, its energy_consumption, completion time and tardiness.  With several orders it is
 * tighter than the environment where an order arrives between two events: the environment releases the order's jobs at
 * the first event time at or after the arrival, the decode at the arrival.
 *
 * 32-bit clocks, exact, for windows with 0 <= bs < be (what the reference's files hold).  No clock can overflow: a window
 * stretches a task on its machine at most once per candidate, because a window that moved anything leaves free[m] >= be,
 * every later t on that machine is then >= be > bs, and none of its three cases can hold again; so every time is at most
 * last arrival + sum of p + sum of the window lengths, which fjsp_env_create bounds below 2^31 (the sum over EVERY
 * operation at the largest p and EVERY window).  Energy is int64: at most 65535 terms power x d, each below 2^31 by
 * create's rule, and per machine idle power x (its gaps, which add up to at most the clock bound): below 2^63 on 32
 * machines for idle powers below 2^26 (the reference's are below 100).
 *
 * Limit: a candidate's state is 5 bytes per job (jobs of the largest instance rounded up to 16) + 8 per machine (free and
 * last_end), at most 5120 bytes, grouped by fjsp_schedule_decode's rule on that figure; fjsp_schedule_decode_dyn_group:
 * the candidates one workgroup decodes, 0 where the state does not fit or the batch is not MO_DFJSP.
 * FJSP_E_ARG, FJSP_E_STATE: as fjsp_schedule_decode.  FJSP_E_UNSUPPORTED: a handle that is not FJSP_VARIANT_MO_DFJSP
 * (fjsp_schedule_decode decodes those), a state beyond the limit.
 * No critical paths for MO_DFJSP: fjsp_schedule_critical refuses it, and so do the critical neighbourhoods of
 * fjsp_schedule_search with the whole of that entry -- the critical-path analysis is additive in durations and window
 * shifts are not.  The uniform neighbourhood needs a decode only: fjsp_schedule_search_dyn searches MO_DFJSP with it. */
int fjsp_schedule_decode_dyn(fjsp_env *e, const int32_t *d_plan, int32_t q_plans, const int32_t *d_moves, int32_t n_cand,
                             int64_t *d_objective, int32_t *d_status, int32_t *d_table, int32_t *d_len, void *stream);
int fjsp_schedule_decode_dyn_group(const fjsp_env *e);

/* Critical paths of decoded schedules (schedule.critical, policy_search.improve(neighbourhood=...); csrc/fjsp_decode.hip):
 * tails, critical flags, one critical path and that path's neighbourhood as moves fjsp_schedule_decode takes, n_cand
 * tables per env in ONE launch, one lane per table, grouped as fjsp_schedule_decode groups its candidates.  Table (i, q)
 * is read against the instance of env i; no env's episode state is read or changed.  Stream-ordered, no host
 * synchronisation, no atomics.
 *
 * d_table i32[N][n_cand][cap][6]: rows (r, stage, n, m, begin, end) as fjsp_schedule_decode writes them; a table ends at
 * its first row of six -1 (or at cap).  Only the table's own order defines the arcs: the job (machine) predecessor of
 * row t is the latest row in front of it with the same (r, n) (the same m), its successor the first such row behind it;
 * a row's duration is end - begin.  For a table that fjsp_schedule_decode wrote these are the arcs of the schedule.
 *
 * Per table: C = the largest end (d_makespan), e0 = the first row with end = C.
 *   d_tail i32[..][cap]: the larger of (tail + duration) of the job successor and of the machine successor, 0 without a
 *     successor: the work that must follow the row (32-bit, exact for every table a decode wrote); -1 past the table.
 *   d_flags u8[..][cap]: bit 1 end + tail = C (critical); bit 2 on the path; bit 4 joined to its path successor by a
 *     machine arc; 0 past the table.
 *   d_path i32[..][cap], d_path_len: row indices from e0 backwards, -1 past path_len.  From the path's current row the
 *     next is, of its job predecessor and its machine predecessor, a tight one (end = the current row's begin), the one
 *     later in the table if both are; a row that is both predecessors is a job arc; with no tight predecessor the
 *     path ends (begin 0, an order's arrival, idle time in a foreign table).
 *   d_moves i32[..][max_moves][3] (may be null with max_moves = 0), d_n_moves, d_skipped: first, per machine arc of the
 *     path in path order (a in row u -> b in row v), the move (4, u, (v - u) | (w - u) << 16) with w = the last row of
 *     b's job in (u, v), or u without one -- it exchanges a and b on their machine --, if w stands in front of the first
 *     row of a's job in (u, v) and w - u <= 32767 (the decoder's limit on dw); an arc that does not is counted in
 *     d_skipped instead (none in a table whose rows are in begin order).  Then, per path row in path order, (1, row, m)
 *     for every other machine m with p > 0 for the row's operation, ascending.  d_n_moves counts all of them; the first
 *     max_moves are written, the rest of the array is (0, 0, 0).
 * d_status i32[N][n_cand]: 0; 1 a row fails a range check (r, n, m, stage against the instance, 0 <= begin < end), checked
 * before the value addresses anything; 2 the table is empty.  With 1 or 2: tail, path and makespan -1, the rest 0.
 *
 * Limits and refusals are fjsp_schedule_decode's (the state here, 4 bytes per job word and per machine, fits in its).
 * FJSP_E_ARG: a null e, d_table or output pointer (d_moves only with max_moves > 0), n_cand < 1, max_moves < 0,
 * N * n_cand >= 2^31.  FJSP_E_UNSUPPORTED: FJSP_VARIANT_MO_DFJSP, a state beyond the limit.  FJSP_E_STATE: a generated
 * handle whose last regenerate failed. */
int fjsp_schedule_critical(fjsp_env *e, const int32_t *d_table, int32_t n_cand, int32_t *d_tail, uint8_t *d_flags, int32_t *d_path,
                           int32_t *d_path_len, int32_t *d_moves, int32_t max_moves, int32_t *d_n_moves, int32_t *d_skipped,
                           int32_t *d_status, int32_t *d_makespan, void *stream);

/* Hill climbing and tabu search on explicit schedules, every round of every env in ONE launch (policy_search.local_search;
 * csrc/fjsp_decode.hip, schedule_search_kernel): one 64-lane workgroup per env, lane q decodes candidate q of a round, the
 * round's selection is a reduction over the wave and the plan stays in LDS from the first round to the last.  The result
 * is a function of the arguments alone; tests/search_reference.py restates it in numpy, bit for bit.
 *
 * Draws: splitmix64 (csrc/fjsp_gen_stream.h, draw(seed, i)).  The env with global id g = first_env + e has the stream
 * s_g = draw(seed ^ FJSP_SEARCH_STREAM, (uint32_t)g); candidate q of round t owns draw(s_g, 3 (t n_cand + q) + c), c = 0, 1, 2
 * (c0, c1, c2).  pick(d, n) = ((d >> 32) * n) >> 32.  The stream depends on g alone: a shard [k, k + n) of a batch
 * reproduces those envs of the whole batch.  fjsp_search_draws (host only) returns draws first .. first + n - 1 of an env's
 * stream, the index wrapping at 2^32.
 *
 * A round t of an env whose current plan has L rows (the input plan at t = 0):
 *   neighbourhood 1, 2: the current plan is decoded and put into begin order (a stable sort of the rows by begin; the same
 *     schedule), and the round's move list is what fjsp_schedule_critical writes for that table with max_moves = 128.
 *     neighbourhood 0 never reorders the plan.
 *   candidate q < n_cand: from the list (neighbourhood 1; 2 for q < n_cand / 2) entry pick(c2, min(n_moves, 128)), masked
 *     when the list is empty; else, q even, (1, u, m) with u = pick(c0, L) and m the pick(c1, n_e)-th of the n_e eligible
 *     machines of row u's operation, ascending (it may be the row's machine); q odd, (2, u, 0) with u = pick(c0, max(L - 1,
 *     1)).  Every candidate is decoded as fjsp_schedule_decode decodes the move on the current plan.
 *   selection: of the unmasked candidates with status 0 the least objective, the lowest q among equals.
 *   accept 0 (strict): taken if below the current plan's objective; 1 (sideways): if not above it.
 *   accept 2 (tabu): every row carries its index in the input plan as identity, through moves and sorting; until[id] = 0
 *     at the start.  A candidate that changes nothing (a reassignment to the row's machine, a swap of two rows of one
 *     job) is masked; one that moves a row with until[id] > t (rows u; u, u + 1; u, v of kinds 1; 2; 4) is tabu and
 *     admissible only if its objective is below the best seen so far.  The winner of the admissible candidates is taken,
 *     better or worse, and its moved rows get until = t + 1 + tenure (saturating at 2^31 - 1).
 *   The move taken is applied to the current plan (as schedule.apply_moves applies it).
 *
 * d_plan i32[N][cap][3] as fjsp_schedule_decode takes it, one plan per env.  d_status i32[N]: the decode status of the
 * input plan; an env whose plan does not decode gets its plan copied through, history and objective -1, accepted 0 and
 * a trace of zeros, and the others are not affected.  d_plan_out i32[N][cap][3]: the best plan seen, replaced only on
 * strict improvement -- with accept 0 and 1 the current plan after the last round; with rounds = 0 the input plan as it
 * came --, -1 rows past its end; d_objective i64[N][2] its (makespan, total tardiness).  d_history i64[rounds + 1][N]: the
 * chosen objective of the input plan, then of the CURRENT plan after every round.  d_accepted i32[N]: moves taken.
 * d_trace (nullable) i32[rounds][N][3]: the move taken in round t, (0, 0, 0) for none; its indices refer to the plan the
 * round started from (in begin order with neighbourhood 1, 2).
 *
 * Stream-ordered, no host synchronisation, two launches for any number of rounds (the kind table, then the search).
 * Limit: 64 candidate states (fjsp_schedule_decode's, 5 bytes per job rounded up to 16 jobs + 4 per machine) and 61
 * bytes per row of the longest plan, 1552 bytes more, must fit the 160 KB of a CU's LDS; fjsp_schedule_search_lds is that
 * sum in bytes, 0 where it does not fit or the batch is MO_DFJSP.
 * FJSP_E_ARG: a null e, d_plan or output other than d_trace, n_cand outside 1..64, rounds < 0, tenure < 0, an objective
 * outside 0..1, a neighbourhood or accept outside 0..2, neighbourhood != 0 with objective != 0, 3 x rounds x n_cand > 2^32 - 1.
 * FJSP_E_UNSUPPORTED: FJSP_VARIANT_MO_DFJSP (fjsp_schedule_search_dyn searches those), a working set beyond the limit (the
 * message gives the bytes).  FJSP_E_STATE: a generated handle whose last regenerate failed. */
#define FJSP_SEARCH_STREAM 0x8CB92BA72F3D8DD7ULL
int fjsp_schedule_search(fjsp_env *e, const int32_t *d_plan, int32_t rounds, int32_t n_cand, int32_t objective, int32_t neighbourhood,
                         int32_t accept, int32_t tenure, uint64_t seed, int64_t first_env, int32_t *d_plan_out, int64_t *d_objective,
                         int64_t *d_history, int32_t *d_accepted, int32_t *d_status, int32_t *d_trace, void *stream);
int fjsp_schedule_search_lds(const fjsp_env *e);
int fjsp_search_draws(uint64_t seed, int64_t env, uint32_t first, int32_t n, uint64_t *h_out);

/* Hill climbing and tabu search on explicit schedules of MO_DFJSP, every round of every env in ONE launch (schedule.search_dyn,
 * policy_search.local_search on such a batch; csrc/fjsp_decode.hip, schedule_search_kernel<true>: that kernel's text
 * compiled with the MO_DFJSP decode).  The contract is fjsp_schedule_search's, restated where it differs;
 * tests/search_dyn_reference.py restates it in numpy, bit for bit.
 *
 * Arguments: fjsp_schedule_search's without `neighbourhood`.  Only the uniform neighbourhood exists here (the critical ones
 * need tails that add up along a path, and window shifts do not): the plan is never reordered and candidate q of a round
 * is drawn as neighbourhood 0 draws it.  objective is 0, 1 or 2: makespan, total tardiness, energy.
 * Decoding: every decode -- the input plan, each candidate's move applied while the plan is read -- is
 * fjsp_schedule_decode_dyn's rule, windows and energy included.
 * Draws: the same stream, s_g = draw(seed ^ FJSP_SEARCH_STREAM, (uint32_t)g), candidate q of round t owns draws
 * 3 (t n_cand + q) + c; fjsp_search_draws serves both entries, and a shard [k, k + n) with first_env = k reproduces those
 * envs of the whole batch.
 * Selection and accept modes: unchanged.  The winner is the least chosen objective among the unmasked candidates of
 * status 0, the lowest q among equals; accept 0 strict, 1 sideways, 2 tabu with until[identity], aspiration against the
 * best chosen objective seen, no-op moves masked, until = t + 1 + tenure saturating at 2^31 - 1; the best plan is replaced
 * only on strict improvement of the chosen objective.  The other two objectives travel with the plans and decide nothing.
 * Outputs: d_objective i64[N][3] = the returned plan's (makespan, total tardiness, energy), all -1 for an env whose input
 * plan does not decode; d_history i64[rounds + 1][N] of the chosen column; d_plan_out, d_accepted, d_status and d_trace
 * (nullable) as fjsp_schedule_search writes them; an env whose plan fails is copied through and the others are not
 * affected.
 *
 * Stream-ordered, no host synchronisation, no atomics, two launches for any number of rounds.
 * Limit: 64 candidate states of fjsp_schedule_decode_dyn (5 bytes per job rounded up to 16 jobs + 8 per machine) and 24
 * bytes per row of the longest plan (the row with its operation type and identity, 20, and until, 4) must fit the 160 KB
 * of a CU's LDS: 64 x (5 x jobs16 + 8 x MP) + 24 x rows; fjsp_schedule_search_dyn_lds is that sum in bytes, 0 where it
 * does not fit or the batch is not MO_DFJSP.
 * FJSP_E_ARG: a null e, d_plan or output other than d_trace, n_cand outside 1..64, rounds < 0, tenure < 0, an objective
 * or accept outside 0..2, 3 x rounds x n_cand > 2^32 - 1.  FJSP_E_UNSUPPORTED: a handle that is not FJSP_VARIANT_MO_DFJSP
 * (fjsp_schedule_search searches those), a working set beyond the limit (the message gives the bytes).  FJSP_E_STATE: a
 * generated handle whose last regenerate failed.  Every check runs before any device call. */
int fjsp_schedule_search_dyn(fjsp_env *e, const int32_t *d_plan, int32_t rounds, int32_t n_cand, int32_t objective, int32_t accept,
                             int32_t tenure, uint64_t seed, int64_t first_env, int32_t *d_plan_out, int64_t *d_objective,
                             int64_t *d_history, int32_t *d_accepted, int32_t *d_status, int32_t *d_trace, void *stream);
int fjsp_schedule_search_dyn_lds(const fjsp_env *e);

/* Search explicit schedules for Pareto fronts, every round of every env in ONE launch (schedule.search_front,
 * policy_search.front_search; csrc/fjsp_decode.hip, schedule_search_kernel<DYN, FrontArgs>: that kernel's text compiled
 * with a weighted key and an archive).  The search is fjsp_schedule_search_dyn's, steered by a weighted sum of the
 * objectives with one weight vector per env -- a batch sweeps the weight simplex over one instance --, and it keeps the
 * Pareto archive of every vector it decodes.  The result is a function of the arguments alone;
 * tests/search_front_reference.py restates it in numpy and Python integers, bit for bit.
 *
 * One entry serves both families.  On a FJSP_VARIANT_MO_DFJSP handle every decode is fjsp_schedule_decode_dyn's and NO = 3
 * (makespan, total tardiness, energy); on every other handle every decode is fjsp_schedule_decode's and NO = 2.  Only the
 * uniform neighbourhood exists here (the critical ones follow the makespan alone).
 *
 * Arguments: fjsp_schedule_search_dyn's with `objective` replaced by d_weights i64[N][NO], one weight vector per env, and
 * cap_front (1..64), the slots of an env's archive, and the archive outputs behind d_trace.
 * Key: key = sum over c of w[c] * obj[c] in int64; every product and every partial sum (left to right) saturates at
 * 2^63 - 2, so a key never reaches the "no candidate" sentinel 2^63 - 1.  The weights are checked per env on the device
 * before anything else: a negative weight or an all-zero vector gives status 5, which outranks the plan's decode status;
 * such an env is copied through exactly as one whose plan does not decode, and its archive is empty.
 * Search: fjsp_schedule_search_dyn's with "chosen objective" read as "key" -- the draw stream (s_g = draw(seed ^
 * FJSP_SEARCH_STREAM, (uint32_t)g), three draws per round and candidate, fjsp_search_draws, global env ids so a shard
 * reproduces its envs), candidate q even (1, u, m) / odd (2, u, 0), selection by the least key and the lowest q, accept 0
 * strict / 1 sideways / 2 tabu with until[identity], aspiration against the best key seen, masked no-ops, until = t + 1 +
 * tenure saturating at 2^31 - 1, the best plan replaced only on strict improvement of the key.
 * d_history i64[rounds + 1][N]: the key of the input plan, then of the current plan after every round.  d_objective
 * i64[N][NO]: the vector of the returned plan.  d_plan_out, d_accepted, d_status, d_trace (nullable): as the siblings.
 *
 * Archive, per env, defined on sets.  It starts as {the input plan's vector} in slot 0 with source (-1, 0).  In round t the
 * round's candidates are every q < n_cand whose decode has status 0, tabu and no-op candidates too.  A candidate is an
 * entrant if no archive member is <= it in every objective (equal included), no other candidate of the round dominates it
 * (<= in every objective and < in one) and no candidate of lower q in the round has the same vector.  Every member that an
 * entrant dominates leaves, whether or not that entrant finds a slot; the entrants then take the lowest free slots in
 * ascending q, and those that find none are counted in d_front_dropped and lost.  A member never moves to another slot.
 * The archive is updated before the round's accepted move is applied: an entrant's plan is the round's start plan with
 * its move applied, as schedule.apply_moves applies it.
 *   d_front_obj     i64[N][cap_front][NO]       member vectors, -1 in free slots
 *   d_front_src     i32[N][cap_front][2]        (round, q) that found the member, (-1, 0) the input plan, (-1, -1) free
 *   d_front_plan    i32[N][cap_front][cap][3]   nullable: member plans, -1 rows past a plan's end (slot 0 holds the input
 *                                               plan's rows up to its first -1 row), all -1 in free slots
 *   d_front_count   i32[N]                      members
 *   d_front_dropped i32[N]                      entrants that found no slot
 * An env with a status other than 0 has count 0, dropped 0 and every slot free.
 *
 * Stream-ordered, no host synchronisation, no atomics, two launches for any number of rounds; capturable.
 * Limit: the 64 candidate states of the family's decode (5 bytes per job rounded up to 16 jobs + 4 per machine, 8 per
 * machine on MO_DFJSP), 24 bytes per row of the longest plan, 8 NO + 8 per archive slot (vector, source) and 64 x (8 NO + 4)
 * (the round's candidate vectors, the free slots in order) must fit the 160 KB of a CU's LDS:
 *   64 x state + 24 x rows + cap_front x (8 NO + 8) + 64 x (8 NO + 4)
 * fjsp_schedule_search_front_lds(e, cap_front) is that sum in bytes, 0 where it does not fit or cap_front is outside 1..64.
 * FJSP_E_ARG: a null e, d_plan, d_weights or output other than d_trace and d_front_plan, n_cand or cap_front outside 1..64,
 * rounds < 0, tenure < 0, accept outside 0..2, 3 x rounds x n_cand > 2^32 - 1.  FJSP_E_UNSUPPORTED: a working set beyond the
 * limit (the message gives the bytes).  FJSP_E_STATE: a generated handle whose last regenerate failed.  Every check runs
 * before any device call. */
int fjsp_schedule_search_front(fjsp_env *e, const int32_t *d_plan, int32_t rounds, int32_t n_cand, const int64_t *d_weights,
                               int32_t accept, int32_t tenure, uint64_t seed, int64_t first_env, int32_t cap_front,
                               int32_t *d_plan_out, int64_t *d_objective, int64_t *d_history, int32_t *d_accepted, int32_t *d_status,
                               int32_t *d_trace, int64_t *d_front_obj, int32_t *d_front_src, int32_t *d_front_plan,
                               int32_t *d_front_count, int32_t *d_front_dropped, void *stream);
int fjsp_schedule_search_front_lds(const fjsp_env *e, int32_t cap_front);

/* Evolve populations of explicit schedules, every generation of every env in ONE launch (schedule.evolve,
 * policy_search.genetic_search; csrc/fjsp_decode.hip, schedule_evolve_kernel<DYN>): a genetic algorithm with tournament
 * selection, a precedence-preserving order crossover, a machine mutation and one elite, the non-learning baseline of the
 * FJSP literature, on the instances, objectives and decode rules of the entries above.  The result is a function of the
 * arguments alone; tests/evolve_reference.py restates it in numpy and Python integers, bit for bit.
 *
 * One entry serves both families.  On a FJSP_VARIANT_MO_DFJSP handle every decode is fjsp_schedule_decode_dyn's and NO = 3
 * (makespan, total tardiness, energy); on every other handle every decode is fjsp_schedule_decode's and NO = 2.
 *
 *   d_pop        i32[N][pop][cap][3]  the start population: pop (1..64) plans per env, as decode takes them
 *   d_weights    i64[N][NO]           the key, fjsp_schedule_search_front's: sum over c of w[c] * obj[c], every product and
 *                                     partial sum saturating at 2^63 - 2; a unit vector is a single objective
 *   mut_rate     0..65536             a child is mutated with probability mut_rate / 65536
 *   d_pop_out    i32[N][pop][cap][3]  the last generation, -1 rows past a plan's end
 *   d_work       i32[N][pop][cap][3]  the other population buffer; its content after the call is unspecified
 *   d_pop_obj    i64[N][pop][NO]      the vectors of d_pop_out's individuals
 *   d_best_plan  i32[N][cap][3], d_objective i64[N][NO]   the individual of d_pop_out with the least (key, index)
 *   d_history    i64[generations + 1][N]   the least key of every generation, the start population's first; it never
 *                                     increases, because of the elite
 *   d_status     i32[N]
 *   d_trace      nullable, i32[generations][N][pop][3]   per child (parent A, parent B, the mutated row or -1)
 * d_pop, d_pop_out and d_work must not overlap.  Generation t reads one of d_pop_out / d_work and writes the other
 * (generation 1 reads d_pop); the first buffer is picked by the parity of `generations`, so that the last lands in
 * d_pop_out.  With generations = 0 the outputs describe the start population (d_pop_out = its rows, -1 past each plan's end).
 *
 * Draws: splitmix64 as everywhere (draw(seed, i)), in a stream of its own: env g = first_env + e has s_g = draw(seed ^
 * FJSP_EVOLVE_STREAM, (uint32_t)g), child q of generation t (1-based) has c = draw(s_g, (uint32_t)((t - 1) * pop + q)), and its
 * draws are d_i = draw(c, i): i = 0..3 the tournaments, 4, 5, 6 the mutation, 8 + w word w of the job set.  pick(d, n) =
 * ((d >> 32) * n) >> 32, as in fjsp_schedule_search.  A shard with first_env = k reproduces its envs of the whole batch.
 *
 * Generation 0: every individual of d_pop is decoded.  Bad weights (a negative one, or all zero) give the env status 5;
 * otherwise, if an individual has a decode status other than 0, the env's status is that of the lowest such q.  An env
 * whose status is not 0 is copied through, and the other envs are not affected: d_pop_out = the input rows as they came,
 * d_best_plan = individual 0, d_pop_obj, d_objective and its d_history column -1, its trace zeros.
 *
 * Generation t >= 1, child q, from generation t - 1:
 *   parents    q = 0 is the elite: A = B = the individual with the least (key, index), every job in J1, no mutation.
 *              q > 0: A = whichever of pick(d0, pop), pick(d1, pop) has the lesser (key, index), B the same of d2, d3.
 *   job set    job j is in J1 iff bit (j & 63) of draw(c, 8 + (j >> 6)) is set; j numbers the jobs over the instance's
 *              kinds in order (the first job of kind r, + n), as the decoder's state does.
 *   crossover  precedence-preserving order crossover: position t' = 0 .. L - 1 of the child is row A[t'] if its job is in
 *              J1, else the next row of B whose job is not in J1, from a cursor that starts at 0 and only moves forward.
 *              Rows travel whole, (r, n, m).
 *   mutation   iff pick(d4, 65536) < mut_rate: child row u = pick(d5, L) runs on the pick(d6, n_e)-th of the n_e eligible
 *              machines of its operation, ascending (the kind-1 candidate of the searches; it may be the row's own).
 *   decode     by the family's rule; the child's vector and key are recorded.
 * The child always decodes: both parents decoded with status 0 on the same instance, so they hold the same operations --
 * the positions of A whose job is outside J1 are as many as the rows of B whose job is outside J1, so the cursor never runs
 * out --, the rows of one job come from one parent and keep that parent's order, so every job meets its stages in order,
 * and every row keeps a machine that was eligible for it, or is moved to one.  The kernel does not rely on it: the cursor is
 * bounded by cap and the child ends where it runs out, every check of the decode runs on every child, and a child that
 * failed would hold no rows and the key 2^63 - 1, which loses every comparison.  Nothing is left to fault.
 *
 * Stream-ordered, no host synchronisation, no atomics, two launches for any number of generations; capturable.
 * Limit: the 64 individuals' states of the family's decode (5 bytes per job rounded up to 16 jobs + 4 per machine, 8 per
 * machine on MO_DFJSP), per individual one bit per job in words of 4 bytes, and two rows of 64 keys must fit the 160 KB of
 * a CU's LDS:   64 x (state + 4 x ceil(jobs16 / 32)) + 1024
 * fjsp_schedule_evolve_lds(e) is that sum in bytes, 0 where it does not fit.
 * FJSP_E_ARG: a null e, d_pop, d_weights or output other than d_trace, pop outside 1..64, generations < 0, mut_rate outside
 * 0..65536, generations x pop > 2^32 - 1.  FJSP_E_UNSUPPORTED: a working set beyond the limit (the message gives the
 * bytes).  FJSP_E_STATE: a generated handle whose last regenerate failed.  Every check runs before any device call. */
#define FJSP_EVOLVE_STREAM 0xC2B2AE3D27D4EB4FULL
int fjsp_schedule_evolve(fjsp_env *e, const int32_t *d_pop, int32_t pop, int32_t generations, const int64_t *d_weights,
                         int32_t mut_rate, uint64_t seed, int64_t first_env,
                         int32_t *d_pop_out, int32_t *d_work, int64_t *d_pop_obj, int32_t *d_best_plan, int64_t *d_objective,
                         int64_t *d_history, int32_t *d_status, int32_t *d_trace, void *stream);
int fjsp_schedule_evolve_lds(const fjsp_env *e);

/* fjsp_schedule_evolve under the ACTIVE decoder (schedule.evolve_active, policy_search.genetic_search(decoder="active");
 * csrc/fjsp_decode.hip, schedule_evolve_active_kernel): the genetic algorithm the FJSP literature scores with insertion
 * into machine gaps.  fjsp_schedule_evolve's arguments in its order, plus d_pop_inserted in front of the stream, and
 * fjsp_schedule_evolve's contract word for word -- the draw stream (FJSP_EVOLVE_STREAM, global env id, generation, child),
 * the key, the parents, job set, crossover and mutation, the status codes 0 to 3 and 5 and the env copied through on one,
 * generations = 0, d_trace, first_env, pop <= 64, the limits on generations and mut_rate, FJSP_E_ARG and FJSP_E_STATE --
 * with ONE change: every decode is fjsp_schedule_decode_active's rule, generation 0 and every child, the mutated row put
 * on its machine before it is placed.  tests/evolve_active_reference.py restates it, bit for bit.
 *
 * Chromosomes are not rewritten (a Baldwinian GA): a child's rows in d_pop_out and d_best_plan are the merged rows in
 * merge order, as fjsp_schedule_evolve writes them; d_pop_obj, d_objective, d_history and the keys of the tournaments are
 * the ACTIVE objectives of those rows, so fjsp_schedule_decode_active of d_pop_out gives d_pop_obj and of d_best_plan
 * d_objective (fjsp_schedule_decode of them gives no less in either entry).
 *   d_pop_inserted   nullable, i32[N][pop]   per individual of d_pop_out, the rows its decode placed in front of an
 *                    interval (fjsp_schedule_decode_active's d_inserted); zeros for an env with a status.
 *
 * Intervals live in the handle's workspace of fjsp_schedule_decode_active: the same allocation, of the same size whichever
 * of the two entries makes it first, the same 8-byte entries, never cleared.  A one-wave workgroup owns an env and cap x 64
 * entries, entry i of individual q of workgroup w at ws[(w cap + i) 64 + q] -- the workgroup's index, not the env's --,
 * and the grid is bounded: min(N, fjsp_schedule_evolve_active_resident(e)) workgroups, workgroup w evolving the envs w,
 * w + grid, ... one after the other.  fjsp_schedule_evolve_active_resident = fjsp_schedule_decode_active_resident / 64:
 * the envs resident at once; 0 where that is 0 (MO_DFJSP included).  ORDERING: as fjsp_schedule_decode_active -- the calls
 * of both entries on one handle share the workspace, so they must be ordered on one stream (or by events).
 * Stream-ordered, no host synchronisation, no atomics, two launches for any number of generations; capturable.
 * Limit: fjsp_schedule_evolve's, unchanged (the LDS layout is the same; fjsp_schedule_evolve_lds).
 * FJSP_E_UNSUPPORTED: FJSP_VARIANT_MO_DFJSP (an insertion under breakdown shifts is not defined by the reference:
 * fjsp_schedule_evolve evolves such a handle), a working set beyond the limit.  FJSP_E_HIP: the workspace could not be
 * allocated.  Every check runs before any device call. */
int fjsp_schedule_evolve_active(fjsp_env *e, const int32_t *d_pop, int32_t pop, int32_t generations, const int64_t *d_weights,
                                int32_t mut_rate, uint64_t seed, int64_t first_env,
                                int32_t *d_pop_out, int32_t *d_work, int64_t *d_pop_obj, int32_t *d_best_plan, int64_t *d_objective,
                                int64_t *d_history, int32_t *d_status, int32_t *d_trace, int32_t *d_pop_inserted, void *stream);
int fjsp_schedule_evolve_active_resident(const fjsp_env *e);

/* ---- fused pieces of the clipped-PPO learning iteration (agents/MPPPO/MPPPO.py:314-370; csrc/fjsp_ppo.hip).
 * All pointers are device pointers, f32; *d_count is the (global) number of samples the losses average over.
 *
 * fjsp_ppo_actor_loss: logits f32[n][n_actions] of the new policy, d_actions f32[n] (flat action index),
 * d_old_log_prob / d_advantages f32[n] -> *d_loss = -sum(min(A r, A clip(r, 1 - eps, 1 + eps))) / count with
 * r = exp(log_softmax(logits)[action]) / (exp(old) + 1e-8) (:325-352), and d_dlogits = d loss / d logits with
 * autograd's conventions (minimum halves ties, clamp passes the gradient on the closed interval).
 * d_partial: f32 scratch of fjsp_ppo_partials(n) entries.
 * fjsp_ppo_critic_loss: *d_loss = sum((value - returns)^2) / count (F.mse_loss, :317-318), d_dvalue = its gradient.
 * fjsp_relu_bwd_bias: d_dh f32[n][width] <- d_dh * (d_h > 0) in place (d_h == NULL: no mask) and d_bias_grad
 * f32[width] = its column sums, through d_partial f32[n_partial_rows][width] (two-stage, deterministic).
 * fjsp_adam_clip_step: clip_grad_norm_(max_norm; <= 0: none) followed by one Adam step (torch.optim.Adam, no weight
 * decay) over flat buffers of n parameters; *d_step is the step count kept on the device (f32), d_scratch64 f32[64]. */
int fjsp_ppo_partials(int32_t n);
int fjsp_ppo_actor_loss(const float *d_logits, const float *d_actions, const float *d_old_log_prob, const float *d_advantages, int32_t n,
                        int32_t n_actions, float clip_epsilon, const float *d_count, float *d_dlogits, float *d_partial, float *d_loss,
                        void *stream);
int fjsp_ppo_critic_loss(const float *d_value, const float *d_returns, int32_t n, const float *d_count, float *d_dvalue, float *d_partial,
                         float *d_loss, void *stream);
int fjsp_relu_bwd_bias(float *d_dh, const float *d_h, int32_t n, int32_t width, float *d_partial, int32_t n_partial_rows, float *d_bias_grad,
                       void *stream);
int fjsp_adam_clip_step(float *d_params, const float *d_grads, float *d_exp_avg, float *d_exp_avg_sq, int32_t n, float max_norm, float lr,
                        float beta1, float beta2, float eps, float *d_step, float *d_scratch64, void *stream);

/* ---- one launch per network and learning iteration: forward + loss + backward on the f32 matrix cores
 * (csrc/fjsp_mlp_train.hip), for the reference's Linear-ReLU-Linear-ReLU-Linear networks with 128 hidden units
 * (agents/MPPPO/MPPPO.py:27-70 actor / critic; the iteration is :314-370).  d_params: the network's parameters in ONE
 * flat f32 buffer, order W1[128][S] b1[128] W2[128][128] b2[128] W3[n_out][128] b3[n_out] (16-byte aligned);
 * d_x f32[n][S].  mode 0 (actor): d_aux0 = actions (flat index as f32), d_aux1 = old log-probabilities, d_aux2 =
 * advantages; loss and gradient as fjsp_ppo_actor_loss.  mode 1 (critic, n_out == 1): d_aux0 = returns; loss as
 * fjsp_ppo_critic_loss.  Outputs: d_grad f32[numel] = d loss / d params (same order as d_params), *d_loss.
 * Scratch: d_partial f32[n_groups][numel], d_loss_partial f32[n_groups], n_groups = fjsp_mlp_train_groups(n).
 * FJSP_E_UNSUPPORTED unless state_size <= 31, hidden == 128, n_out <= 32.
 * fjsp_mlp_train_step: the pass followed by the optimiser step of fjsp_adam_clip_step on d_grad, in three launches
 * (pass, gradient finish + squared norm + step count, clip + Adam); d_sumsq_partial: f32 scratch of (numel + 63) / 64
 * entries.  Single-process form: with several GPUs call fjsp_mlp_train_pass, all-reduce d_grad, fjsp_adam_clip_step. */
int fjsp_mlp_train_groups(int32_t n);
int fjsp_mlp_train_step(int32_t mode, float *d_params, const float *d_x, int32_t n, int32_t state_size, int32_t hidden, int32_t n_out,
                        const float *d_aux0, const float *d_aux1, const float *d_aux2, const float *d_count, float clip_epsilon,
                        float *d_partial, int32_t n_groups, float *d_loss_partial, float *d_grad, float *d_loss, float *d_exp_avg,
                        float *d_exp_avg_sq, float max_norm, float lr, float beta1, float beta2, float eps, float *d_step,
                        float *d_sumsq_partial, void *stream);
int fjsp_mlp_train_pass(int32_t mode, const float *d_params, const float *d_x, int32_t n, int32_t state_size, int32_t hidden,
                        int32_t n_out, const float *d_aux0, const float *d_aux1, const float *d_aux2, const float *d_count,
                        float clip_epsilon, float *d_partial, int32_t n_groups, float *d_loss_partial, float *d_grad, float *d_loss,
                        void *stream);

/* fjsp_mlp_train_step for the critic (mode 1) that also hands out what its forward computed: d_values_out f32[n] = V(s) of
 * every sample under the parameters BEFORE this step's update -- the values the advantages of the round are built from
 * (MPPPO.py:263 returns - critic(states)), so the first critic iteration of a learning round replaces the separate
 * forward pass. */
int fjsp_mlp_train_step_values(int32_t mode, float *d_params, const float *d_x, int32_t n, int32_t state_size, int32_t hidden,
                               int32_t n_out, const float *d_aux0, const float *d_aux1, const float *d_aux2, const float *d_count,
                               float clip_epsilon, float *d_partial, int32_t n_groups, float *d_loss_partial, float *d_grad,
                               float *d_loss, float *d_exp_avg, float *d_exp_avg_sq, float max_norm, float lr, float beta1,
                               float beta2, float eps, float *d_step, float *d_sumsq_partial, float *d_values_out, void *stream);

/* ------------------------------------------------------------------------- *
 * Action sampling of the HMPSAC policy networks in one launch
 * (agents/HMPSAC/SAC_Discrete.py:277-284 pick_lower_action, :248-254 pick_action;
 *  A3C_v5.1.py:35-75 TaskPolicyNet / MachinePolicyNet)
 * ------------------------------------------------------------------------- */
/* a_task ~ Categorical(softmax(task(state.float()))), then -- if machine_layers > 0 --
 * a_machine ~ Categorical(softmax(machine(cat(state.float(), a_task)))) for `rows` states f64[rows][state_size].
 * A network is Linear-ReLU-...-Linear: n linear layers (1..6), dims[n + 1] widths (each <= 256, outputs <= 64,
 * dims[0] = state_size, resp. state_size + 1), weights[l] f32[dims[l]][dims[l+1]] row-major -- the TRANSPOSE of
 * torch.nn.Linear.weight, so that the threads of a wave read consecutive words -- and biases[l] f32[dims[l+1]], device pointers.  Randomness: a counter-based stream per row -- splitmix64(seed, row,
 * d_draws[row]) -- whose draw counters u32[rows] live in device memory and advance with every call, so the launch can be
 * replayed from a HIP graph.  d_p_task / d_p_machine (nullable): the f32 probabilities the actions were drawn from.
 * d_pair (nullable, needs the machine network): u8[rows][2] = (a_task, a_machine), the action pair as fjsp_env_step takes it,
 * written for the rows with d_select[row] == which (d_select NULL: every row) -- pick_lower_action's "env e follows lower
 * policy which[e]" without the gather / where launches around it.
 * Other shapes: FJSP_E_UNSUPPORTED (the caller keeps the library path). */
int fjsp_policy_pair_sample(int32_t task_layers, const int32_t *task_dims, const float *const *task_w, const float *const *task_b,
                            int32_t machine_layers, const int32_t *machine_dims, const float *const *machine_w,
                            const float *const *machine_b, const double *d_state, int32_t rows, int32_t state_size, uint64_t seed,
                            uint32_t *d_draws, int64_t *d_a_task, int64_t *d_a_machine, float *d_p_task, float *d_p_machine,
                            uint8_t *d_pair, const int64_t *d_select, int32_t which, void *stream);

#ifdef __cplusplus
}
#endif
#endif
