// Host-only check of the shared generator text (csrc/fjsp_gen_stream.h) as fjsp_instance.cpp instantiates it: its element
// functions are templates over the rows' element type (int vectors here, u8 / u16 rows in LDS on the device), so the host's
// instantiation is the one a sanitizer can see.  Generates the parameter sets of tests/golden/make_generator_golden.py, a
// few seeds each, and reads every array back.  Meant for the address and undefined-behaviour sanitizers:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_DEVICE_COMPILE__ \
//       -I include tools/gen_stream_check.cpp deep_reinforcement_learning_for_fjsp_amd/csrc/fjsp_instance.cpp \
//       deep_reinforcement_learning_for_fjsp_amd/csrc/fjsp_lp.cpp -o gen_stream_check -lpthread && ./gen_stream_check
//
// (-D__HIP_DEVICE_COMPILE__ as in tools/lp_pool_check.cpp: fjsp_lp.cpp's branch without target_clones.)
#include <cstdio>
#include <vector>

#include "../include/fjsp_amd.h"

static fjsp_gen_params params(int R_min, int R_max, int J_min, int J_max, int M, int p_min, int p_max, int N_min, int N_max, int S, double DDT,
                              double t_min = 100.0, double t_max = 200.0) {
    fjsp_gen_params g{};
    g.R_min = R_min; g.R_max = R_max; g.J_min = J_min; g.J_max = J_max; g.M = M; g.p_min = p_min; g.p_max = p_max;
    g.N_min = N_min; g.N_max = N_max; g.S = S; g.DDT = DDT; g.t_si_min = t_min; g.t_si_max = t_max;
    return g;
}
static fjsp_gen_params small(int M = 4) { return params(2, 3, 1, 3, M, 1, 9, 1, 2, 1, 1.0); }
static fjsp_gen_params reference(int N_min = 5, int N_max = 50, int M = 0) { return params(3, 12, 3, 5, M, 40, 400, N_min, N_max, 1, 1.0); }
static fjsp_gen_orders orders(fjsp_gen_params base, int M_min, int M_max, double d_min, double d_max, int S_min, int S_max) {
    fjsp_gen_orders o{};
    o.r.base = base; o.r.M_min = M_min; o.r.M_max = M_max; o.r.DDT_min = d_min; o.r.DDT_max = d_max; o.S_min = S_min; o.S_max = S_max;
    return o;
}
static fjsp_gen_dynamic dynamic(fjsp_gen_orders o, int W_max, int redraws, int gap_min = 1, int gap_max = 60, int len_min = 1, int len_max = 30) {
    fjsp_gen_dynamic d{};
    d.o = o; d.redraws = redraws;
    d.m.pw_min = 10; d.m.pw_max = 200; d.m.idle_min = 1; d.m.idle_max = 9; d.m.W_max = W_max;
    d.m.gap_min = gap_min; d.m.gap_max = gap_max; d.m.len_min = len_min; d.m.len_max = len_max;
    return d;
}

static int n_made = 0, n_refused = 0;
// reads instance 0 back in full: a row the generator left too short shows here
static int read_back(fjsp_instances *s, const char *name) {
    int32_t d[6], dd[2];
    if (fjsp_instances_dims(s, 0, d) != FJSP_OK || fjsp_instances_dynamic_dims(s, 0, dd) != FJSP_OK) { std::printf("%s: dims: %s\n", name, fjsp_last_error()); return 1; }
    const size_t R = d[0], M = d[1], K = d[2], S = d[3];
    std::vector<int32_t> Jr(R), p(K * M), en(K), el(K * M), cnt(S * R), arr(S), del(S), pw(K * M), ip(M), bn(M), bk(2 * (size_t)dd[1] + 2);
    std::vector<double> x(K * M);
    double ddt = 0.0;
    if (fjsp_instances_get(s, 0, Jr.data(), p.data(), en.data(), el.data(), cnt.data(), arr.data(), del.data(), &ddt, x.data()) != FJSP_OK) return 1;
    if (dd[0] && fjsp_instances_get_dynamic(s, 0, pw.data(), ip.data(), bn.data(), bk.data()) != FJSP_OK) return 1;
    for (size_t i = 1; i < S; ++i)
        if (del[i] < del[i - 1]) { std::printf("%s: delivery times not ascending\n", name); return 1; }
    ++n_made;
    return 0;
}

template <class Q, class Call>
static int run(const char *name, const Q &q, Call call, bool may_refuse = false) {
    fjsp_instances *s = nullptr;
    if (fjsp_instances_create(1, &s) != FJSP_OK) return 2;
    int bad = 0;
    for (uint64_t seed = 31000; seed < 31008 && !bad; ++seed) {
        const int rc = call(s, 0, seed, &q);
        if (rc == FJSP_E_UNSUPPORTED && may_refuse) { ++n_refused; continue; }
        if (rc != FJSP_OK) { std::printf("%s seed %llu: %s\n", name, (unsigned long long)seed, fjsp_last_error()); bad = 1; }
        else bad = read_back(s, name);
    }
    fjsp_instances_destroy(s);
    return bad;
}

int main() {
    int bad = 0;
    bad |= run("bench_10x5", params(10, 10, 3, 5, 5, 1, 20, 1, 1, 1, 1.0), fjsp_instances_generate);
    bad |= run("reference_m10", reference(5, 50, 10), fjsp_instances_generate);
    bad |= run("multi_job", params(3, 5, 2, 3, 6, 1, 20, 2, 4, 1, 1.5), fjsp_instances_generate);
    bad |= run("training_mpppo", orders(reference(), 10, 20, 0.5, 1.5, 1, 1).r, fjsp_instances_generate_drawn);
    bad |= run("training_ddqn", orders(reference(1, 2), 3, 8, 0.5, 1.5, 1, 1).r, fjsp_instances_generate_drawn);
    bad |= run("orders_da3c / orders_hmpsac", orders(reference(), 10, 20, 0.5, 1.5, 1, 5), fjsp_instances_generate_orders);
    bad |= run("dynamic_hmpsac", dynamic(orders(reference(), 10, 20, 0.5, 1.5, 1, 5), 0, 8, 50, 400, 5, 60), fjsp_instances_generate_dynamic);
    bad |= run("one_machine", small(1), fjsp_instances_generate);
    fjsp_gen_params wide = small(32); wide.J_min = 2;
    bad |= run("machines_32", wide, fjsp_instances_generate);
    bad |= run("types_beyond_64", params(14, 16, 4, 5, 4, 1, 9, 1, 2, 1, 1.0), fjsp_instances_generate);
    bad |= run("orders_16_tied", orders(params(2, 2, 1, 2, 4, 1, 9, 1, 2, 1, 1.0, 0.0, 0.0), 3, 5, 0.5, 1.5, 16, 16), fjsp_instances_generate_orders);
    bad |= run("ddt_signed", orders(small(), 3, 6, -1.0, 1.5, 1, 1).r, fjsp_instances_generate_drawn);
    bad |= run("one_job", orders(params(2, 3, 1, 3, 4, 1, 9, 1, 1, 1, 1.0), 3, 6, 0.5, 1.5, 1, 3), fjsp_instances_generate_orders);
    const fjsp_gen_orders shop = orders(params(3, 3, 2, 3, 4, 1, 9, 1, 2, 1, 1.0), 3, 6, 0.5, 1.5, 1, 3);
    bad |= run("dynamic_no_windows", dynamic(shop, 0, 8), fjsp_instances_generate_dynamic);
    bad |= run("dynamic_windows", dynamic(shop, 3, 8), fjsp_instances_generate_dynamic);
    const fjsp_gen_orders few = orders(params(1, 1, 2, 4, 4, 1, 9, 1, 2, 1, 1.0), 4, 4, 0.5, 1.5, 1, 2);
    bad |= run("dynamic_redraw", dynamic(few, 2, 16), fjsp_instances_generate_dynamic);
    bad |= run("dynamic_refused", dynamic(few, 2, 0), fjsp_instances_generate_dynamic, true);
    if (bad) return 1;
    std::printf("gen_stream_check OK: %d instances generated and read back, %d refused with redraws = 0\n", n_made, n_refused);
    return 0;
}
