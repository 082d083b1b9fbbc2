// Host-only check of the blocking LP pool (csrc/fjsp_lp_pool.h) through fjsp_instances_solve_fluid: the same few dozen
// generated instances solved on 1, 2 and 8 threads must give the same x, bit for bit; then one LpPool kept alive, as a handle
// keeps its own, with run() called over and over on varying counts (1 and 0 included, a failing index too).  Meant for a
// thread sanitizer:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=thread -D__HIP_DEVICE_COMPILE__ -I include tools/lp_pool_check.cpp \
//       deep_reinforcement_learning_for_fjsp_amd/csrc/fjsp_instance.cpp deep_reinforcement_learning_for_fjsp_amd/csrc/fjsp_lp.cpp \
//       -o lp_pool_check -lpthread && ./lp_pool_check
//
// (-D__HIP_DEVICE_COMPILE__ takes fjsp_lp.cpp's branch without target_clones: the resolvers of cloned functions run
// before the sanitizer's runtime is up and the program would die before main.)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../deep_reinforcement_learning_for_fjsp_amd/csrc/fjsp_lp_pool.h"

// One kept pool, many runs: every index visited exactly once per run, the first failure reported, nothing after it begun under skip_rest
static int kept_pool() {
    fjsp::LpPool pool(7);
    const uint32_t counts[] = {1, 40, 0, 1, 3, 500, 1, 8, 2, 1000};
    for (int rep = 0; rep < 30; ++rep) {
        const uint32_t n = counts[rep % 10];
        std::vector<int> hits(n, 0);
        const int fail_at = rep % 3 == 2 && n > 2 ? (int)n / 2 : -1;
        const bool skip = rep % 2 == 1;
        const fjsp::LpFailure bad = pool.run(n, [&](uint32_t q) { ++hits[q]; return (int)q != fail_at; }, skip);
        if ((bad.index >= 0) != (fail_at >= 0) || (fail_at >= 0 && bad.index != fail_at)) { std::printf("kept pool: run %d reported %d\n", rep, bad.index); return 1; }
        for (uint32_t q = 0; q < n; ++q)
            if (hits[q] > 1 || (hits[q] == 0 && !(skip && fail_at >= 0))) { std::printf("kept pool: run %d index %u visited %d times\n", rep, q, hits[q]); return 1; }
    }
    return 0;
}

int main() {
    const int n = 48, threads[3] = {1, 2, 8};
    fjsp_gen_params prm{};
    prm.R_min = 6; prm.R_max = 10; prm.J_min = 3; prm.J_max = 5; prm.M = 5; prm.p_min = 1; prm.p_max = 20;
    prm.N_min = 1; prm.N_max = 3; prm.S = 1; prm.DDT = 1.0; prm.t_si_min = 100.0; prm.t_si_max = 200.0;
    std::vector<std::vector<double>> xs[3];
    for (int t = 0; t < 3; ++t) {
        fjsp_instances *s = nullptr;
        if (fjsp_instances_create(n, &s) != FJSP_OK) return 2;
        for (int i = 0; i < n; ++i)
            if (fjsp_instances_generate(s, i, 5000u + (uint64_t)i, &prm) != FJSP_OK) { std::printf("generate: %s\n", fjsp_last_error()); return 2; }
        // twice on the same pool size: the second run meets solved instances, as a training loop's refill does
        for (int rep = 0; rep < 2; ++rep)
            if (fjsp_instances_solve_fluid(s, 0, n, threads[t]) != FJSP_OK) { std::printf("solve_fluid: %s\n", fjsp_last_error()); return 2; }
        for (int i = 0; i < n; ++i) {
            int32_t dims[6];
            fjsp_instances_dims(s, i, dims);
            std::vector<double> x((size_t)dims[2] * dims[1]);
            fjsp_instances_get(s, i, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, x.data());
            xs[t].push_back(x);
        }
        fjsp_instances_destroy(s);
    }
    for (int t = 1; t < 3; ++t)
        for (int i = 0; i < n; ++i)
            if (xs[t][i].size() != xs[0][i].size() || std::memcmp(xs[t][i].data(), xs[0][i].data(), xs[0][i].size() * 8) != 0) {
                std::printf("x of instance %d differs between 1 and %d threads\n", i, threads[t]);
                return 1;
            }
    if (kept_pool() != 0) return 1;
    std::printf("lp_pool_check OK: %d instances, x equal on 1, 2 and 8 threads; 30 runs on one kept pool\n", n);
    return 0;
}
