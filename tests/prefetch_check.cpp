// Stand-alone program around the self-play driver with speculative leaf prefetch (cattus_sp_config::prefetch): the runner, the
// stand-in network, several worker and evaluation threads.  Built by tests/test_prefetch.py together with
// cattus_amd/csrc/host/cabi.cpp, once with -fsanitize=address,undefined and once with -fsanitize=thread, and run as a program.
// Every case plays the same games with prefetch off and on and compares the records byte for byte.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/cattus_selfplay.h"

struct Run {
    int rc = -1;
    cattus_sp_summary s{};
    uint64_t pf[4] = {0, 0, 0, 0};
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> meta;
};

static Run play(int game, uint32_t sims, uint32_t prefetch, uint32_t fill, uint32_t threads, uint32_t batch, uint32_t slots, uint32_t games,
                bool two_models, bool noisy, uint32_t eval_threads) {
    cattus_sp_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c, c.sim_num = sims, c.explore_factor = 1.41421f;
    c.temperature_count = 2, c.temperature_threshold[0] = noisy ? 4 : 0, c.temperature_value[0] = 1.0f;
    c.temperature_threshold[1] = 9999, c.temperature_value[1] = 0.0f;
    if (noisy) c.prior_noise_alpha = 0.3f, c.prior_noise_epsilon = 0.25f;
    c.cache_size = 20000, c.batch_size = batch, c.threads = threads, c.concurrent_games = slots, c.seed = 5, c.game_stride = 1;
    c.eval_threads = eval_threads, c.max_game_plies = game == CATTUS_GAME_CHESS ? 10 : 0;
    c.prefetch = prefetch, c.prefetch_fill = fill;
    uint32_t info[5];
    cattus_sp_game_info(game, info);
    uint32_t ctx[2] = {info[1], info[2] * info[3]};
    Run r;
    cattus_sp_result* res = nullptr;
    r.rc = cattus_sp_run(game, &c, cattus_sp_stub_net, ctx, two_models ? cattus_sp_stub_net : nullptr, two_models ? ctx : nullptr, games, nullptr,
                         nullptr, 1, &res);
    if (r.rc != 0) {
        fprintf(stderr, "run failed: %s\n", cattus_sp_last_error());
        return r;
    }
    cattus_sp_result_summary(res, &r.s);
    cattus_sp_result_prefetch(res, r.pf);
    r.bytes.resize((size_t)r.s.records * info[4]);
    r.meta.resize((size_t)r.s.records * 3);
    cattus_sp_result_records(res, r.bytes.data(), r.meta.data());
    cattus_sp_result_free(res);
    return r;
}

int main() {
    struct Case {
        int game;
        uint32_t sims, prefetch, fill, threads, batch, slots, games;
        bool two_models, noisy;
        uint32_t eval_threads;
    };
    const Case cases[] = {
        {CATTUS_GAME_TTT, 30, 4, 0, 4, 8, 6, 12, false, false, 2},   {CATTUS_GAME_HEX5, 30, 15, 0, 6, 16, 12, 12, false, true, 2},
        {CATTUS_GAME_HEX5, 30, 4, 3, 3, 4, 8, 8, true, true, 3},     {CATTUS_GAME_CHESS, 12, 4, 0, 6, 8, 6, 6, false, false, 2},
        {CATTUS_GAME_CHESS, 12, 15, 0, 4, 32, 4, 4, true, true, 1},  {CATTUS_GAME_HEX4, 24, 1, 0, 2, 1, 4, 8, false, false, 2},
    };
    int bad = 0;
    for (const Case& k : cases) {
        const Run off = play(k.game, k.sims, 0, 0, 1, 1, k.slots, k.games, k.two_models, k.noisy, 1);
        const Run on = play(k.game, k.sims, k.prefetch, k.fill, k.threads, k.batch, k.slots, k.games, k.two_models, k.noisy, k.eval_threads);
        const bool same = off.rc == 0 && on.rc == 0 && off.bytes == on.bytes && off.meta == on.meta && !off.bytes.empty();
        // batch_size 1: no batch ever has a free row, so everything nominated is dropped
        const bool counted = on.pf[0] == on.pf[1] + on.pf[3] && on.pf[0] > 0 && (k.batch > 1 ? on.pf[2] > 0 : on.pf[1] == 0) &&
                             off.pf[0] + off.pf[1] + off.pf[2] + off.pf[3] == 0;
        printf("game %d prefetch %u: records %s, %llu bytes; nominated %llu evaluated %llu hits %llu dropped %llu; evals %llu -> %llu, batches %llu -> %llu\n",
               k.game, k.prefetch, same ? "equal" : "DIFFER", (unsigned long long)on.bytes.size(), (unsigned long long)on.pf[0],
               (unsigned long long)on.pf[1], (unsigned long long)on.pf[2], (unsigned long long)on.pf[3], (unsigned long long)off.s.node_evals,
               (unsigned long long)on.s.node_evals, (unsigned long long)off.s.activation_count, (unsigned long long)on.s.activation_count);
        if (!same || !counted) bad++;
    }
    if (bad) {
        printf("%d cases failed\n", bad);
        return 1;
    }
    printf("prefetch ok\n");
    return 0;
}
