// One env of fjsp_schedule_evolve (schedule_evolve_kernel<DYN>: ACTIVE false) and of fjsp_schedule_evolve_active
// (schedule_evolve_active_kernel: ACTIVE true, in its loop over the workgroup's envs); fjsp_decode.hip includes it in both
// and says there why it is a text and not a function, what it reads and what FJSP_EVOLVE_DONE is.  ACTIVE: every decode
// places its rows through the lane's Gaps object (fjsp_schedule_decode_active's rule; the intervals in slot q of `ws`),
// and `ins` takes the count of the lane's last decode.
    static_assert(!(DYN && ACTIVE), "an insertion under breakdown shifts is not defined");
    constexpr int NO = DYN ? 3 : 2;
    constexpr long long kNone = 0x7fffffffffffffffLL;                    // the key of a lane without an individual, or of a child that failed
    const int q = (int)threadIdx.x, inst = env % b.n_inst;
    const int cap = a.cap, P = a.P, N = b.N, T = a.generations;
    const Shop sh = shop_of(b, a.kinds, inst, a.JW);
    const State st = state_at(decode_lds, q, 64, a.JW);
    DynShop dy{};
    if constexpr (DYN) dy = dyn_shop_of(b, sh, st, dyn_windows(b));
    const int SW = DYN ? dyn_state_words(a.JW, b.MP) : state_words(a.JW, b.MP), JS = evolve_set_words(a.JW);
    uint32_t *jset = decode_lds + (size_t)SW * 64 + q;                   // word w of this lane's set at jset[w * 64]
    long long *keys = reinterpret_cast<long long *>(decode_lds + (size_t)(SW + JS) * 64);     // [2][64]
    const size_t PW = (size_t)cap * 3, base = (size_t)env * P * PW;      // words of a plan; the env's first word in a population
    auto gaps_of = evolve_gaps<ACTIVE>(ws, q);                           // the lane's, handed to both decodes by pointer
    auto *gaps = evolve_gaps_ptr(gaps_of);

    const long long *w = reinterpret_cast<const long long *>(a.weights) + NO * (size_t)env;
    const long long w0 = w[0], w1 = w[1], w2 = DYN ? w[2] : 0;
    const bool bad_w = w0 < 0 || w1 < 0 || w2 < 0 || (w0 | w1 | w2) == 0;
    auto chosen = [&](long long mk, long long td, long long en) { return key_add(key_add(key_mul(w0, mk), key_mul(w1, td)), DYN ? key_mul(w2, en) : 0LL); };
    // the least (key, index) of the wave, the same in every lane
    auto least = [&](long long key, long long &bkey, int &bq) {
        bkey = key; bq = q;
        for (int off = 32; off > 0; off >>= 1) {
            const long long ok2 = __shfl_xor(bkey, off);
            const int oq = __shfl_xor(bq, off);
            if (ok2 < bkey || (ok2 == bkey && oq < bq)) { bkey = ok2; bq = oq; }
        }
    };

    // ---- generation 0: every individual of pop decoded by its lane
    int L = 0, st0 = 0;
    long long mk = 0, td = 0, en = 0, key = kNone;
    if (q < P && !bad_w) {
        const int32_t *pl = a.pop + base + (size_t)q * PW;
        st0 = decode_plan<DYN>(b, sh, st, [&](int idx) { return row_at(pl, idx); }, cap, no_move(), [](int, const Row &, const Step &) {}, L, mk, td, &dy, &en, NoFix{}, gaps);
        if (st0 == 0) key = chosen(mk, td, en);
    }
    const unsigned long long failed = __ballot(st0 != 0);
    const int status = bad_w ? 5 : (failed ? __shfl(st0, __ffsll(failed) - 1) : 0);
    if (status != 0) {                                                   // (the same in every lane) the env is copied through
        for (size_t i = q; i < (size_t)P * PW; i += 64) a.pop_out[base + i] = a.pop[base + i];
        for (size_t i = q; i < PW; i += 64) a.best_plan[(size_t)env * PW + i] = a.pop[base + i];
        if (q < P)
            for (int c = 0; c < NO; ++c) a.pop_obj[((size_t)env * P + q) * NO + c] = -1;
        if (q == 0) {
            a.status[env] = status;
            for (int c = 0; c < NO; ++c) a.objective[NO * (size_t)env + c] = -1;
        }
        for (int t = q; t <= T; t += 64) a.history[(size_t)t * N + env] = -1;
        if (a.trace)
            for (int t = 0; t < T; ++t)
                for (int i = q; i < P * 3; i += 64) a.trace[((size_t)t * N + env) * (size_t)P * 3 + i] = 0;
        if constexpr (ACTIVE)
            if (ins && q < P) ins[(size_t)env * P + q] = 0;
        FJSP_EVOLVE_DONE;
    }
    if (T == 0) {                                                        // the outputs describe the input population: the wave copies it
        for (int p = 0; p < P; ++p) {
            const int Lp = __shfl(L, p);
            const int32_t *pl = a.pop + base + (size_t)p * PW;
            int32_t *o = a.pop_out + base + (size_t)p * PW;
            for (int i = q; i < cap * 3; i += 64) o[i] = i < Lp * 3 ? pl[i] : -1;
        }
    }
    keys[q] = key;
    __syncthreads();

    const uint64_t sg = gen::draw(a.seed, (uint32_t)(a.first_env + env));
    const int32_t *src = a.pop + base;
    for (int t = 1; t <= T; ++t) {
        long long bkey;
        int bq;
        least(key, bkey, bq);
        if (q == 0) a.history[(size_t)(t - 1) * N + env] = bkey;
        int32_t *dst = (((T - t) & 1) ? a.work : a.pop_out) + base;      // the last generation lands in pop_out
        const long long *kprev = keys + ((t - 1) & 1) * 64;
        if (q < P) {
            const uint64_t c = gen::draw(sg, (uint32_t)(t - 1) * (uint32_t)P + (uint32_t)q);
            int pa = bq, pb = bq, mrow = -1;
            const bool elite = q == 0;                                   // both parents the best individual, every job from A, no mutation
            if (!elite) {
                auto tournament = [&](uint32_t i) {
                    const int x = (int)search_pick(gen::draw(c, i), (uint32_t)P), y = (int)search_pick(gen::draw(c, i + 1u), (uint32_t)P);
                    const long long kx = kprev[x], ky = kprev[y];
                    return (ky < kx || (ky == kx && y < x)) ? y : x;
                };
                pa = tournament(0u); pb = tournament(2u);
                for (int i = 0; i < JS; ++i) jset[(size_t)i * 64] = (uint32_t)(gen::draw(c, 8u + (uint32_t)(i >> 1)) >> (32 * (i & 1)));
                if ((int)search_pick(gen::draw(c, 4u), 65536u) < a.mut_rate && sh.ops > 0) mrow = (int)search_pick(gen::draw(c, 5u), (uint32_t)sh.ops);
            }
            const int32_t *A = src + (size_t)pa * PW, *B = src + (size_t)pb * PW;
            int32_t *ch = dst + (size_t)q * PW;
            // is the row's job in J1?  (a row whose kind or job number is out of range is in no set; the decode refuses it)
            auto in_set = [&](const Row &x) {
                if (elite) return true;
                if (x.r < 0 || x.r >= sh.R) return false;
                const uint32_t ka = sh.kinds[1 + x.r].x;
                const int j = (int)(ka & 0xFFFFu) + x.n;
                if (x.n < 0 || x.n >= (int)(ka >> 16) || j >= sh.JW) return false;
                return ((jset[(size_t)(j >> 5) * 64] >> (j & 31)) & 1u) != 0u;
            };
            // The child's rows: decode_plan asks for rows 0, 1, 2 ... in this order, each once, when the move is none (or of kind
            // 1), so B's cursor lives here and only moves forward.  It stays below cap; where it runs out the child ends.
            int cur = 0;
            auto row = [&](int idx) {
                const Row x = row_at(A, idx);
                if (is_end(x) || in_set(x)) return x;
                while (cur < cap) {
                    const Row y = row_at(B, cur++);
                    if (is_end(y)) break;
                    if (!in_set(y)) return y;
                }
                return Row{-1, -1, -1};
            };
            // the mutation: row mrow runs on the pick(d6, n_e)-th of the n_e eligible machines of its operation, ascending
            auto fix = [&](int i, Row &x, int k) {
                if (i != mrow) return;
                const uint16_t *pk = sh.p + (size_t)k * sh.MP;
                int n_e = 0;
                for (int m = 0; m < sh.M; ++m) n_e += pk[m] != 0 ? 1 : 0;
                if (n_e == 0) return;
                int left = (int)search_pick(gen::draw(c, 6u), (uint32_t)n_e);
                for (int m = 0; m < sh.M; ++m)
                    if (pk[m] != 0 && left-- == 0) { x.m = m; break; }
            };
            evolve_gaps_reset(gaps);                                     // (the count is a decode's, not the lane's)
            const int err = decode_plan<DYN>(b, sh, st, row, cap, no_move(), [&](int i, const Row &x, const Step &) {
                ch[3 * i] = x.r; ch[3 * i + 1] = x.n; ch[3 * i + 2] = x.m;
            }, L, mk, td, &dy, &en, fix, gaps);
            key = err ? kNone : chosen(mk, td, en);                      // a child that failed loses every comparison; its plan is empty
            for (int i = err ? 0 : L; i < cap; ++i) { ch[3 * i] = -1; ch[3 * i + 1] = -1; ch[3 * i + 2] = -1; }
            if (a.trace) {
                int32_t *o = a.trace + (((size_t)(t - 1) * N + env) * (size_t)P + q) * 3;
                o[0] = pa; o[1] = pb; o[2] = mrow;
            }
        }
        keys[(t & 1) * 64 + q] = key;
        __syncthreads();                                                 // the children and their keys are handed on
        src = dst;
    }

    long long bkey;
    int bq;
    least(key, bkey, bq);
    const long long b_mk = __shfl(mk, bq), b_td = __shfl(td, bq), b_en = __shfl(en, bq);
    if (q == 0) {
        a.history[(size_t)T * N + env] = bkey;
        a.status[env] = 0;
        a.objective[NO * (size_t)env] = b_mk; a.objective[NO * (size_t)env + 1] = b_td;
        if constexpr (DYN) a.objective[NO * (size_t)env + 2] = b_en;
    }
    if (q < P) {
        int64_t *o = a.pop_obj + ((size_t)env * P + q) * NO;
        o[0] = mk; o[1] = td;
        if constexpr (DYN) o[2] = en;
        if constexpr (ACTIVE)
            if (ins) ins[(size_t)env * P + q] = key == kNone ? 0 : evolve_gaps_count(gaps);      // (a failed child holds no rows)
    }
    __syncthreads();                                                     // (T = 0: the rows above)
    for (size_t i = q; i < PW; i += 64) a.best_plan[(size_t)env * PW + i] = a.pop_out[base + (size_t)bq * PW + i];
