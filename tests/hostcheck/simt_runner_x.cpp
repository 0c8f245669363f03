// simt_runner_x.cpp -- TEST-ONLY: the P-player GameRunner (azx::runner_body_x of csrc/azul_rules_x.hpp, the body of azul_x_runner_kernel,
// UNMODIFIED) compiled by g++ and run lane by lane in lockstep (simt/simt.hpp) on host memory, so that it can be diffed against the model
// composed from the oracle (tests/mp_runner_model.py) before a GPU sees it.  Built by tests/test_hostcheck_runner_x.py with the flags of
// tests/hostcheck/Makefile.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
#include "azul_selfplay2.hpp"
#include "azul_rules_x.hpp"

using namespace az;

struct RJob {
    azx::XBatchDev b;
    azx::XRun run;
    u32 wave;
    u32 mt_lds[2][624];
    double2 tab_lds[51 * T_STRIDE];
};

template <u32 P, u32 D>
static void lane_run(void *arg)
{
    RJob *j = (RJob *)arg;
    azx::runner_body_x<P, D>(j->b, j->run, j->wave, j->mt_lds, j->tab_lds);
}

typedef void (*lane_fn)(void *);
static lane_fn pick_fn(int players, int displays)
{
#define AZ_CASE(PP, DD) if (players == PP && displays == DD) return lane_run<PP, DD>
    AZ_CASE(2, 5); AZ_CASE(3, 5); AZ_CASE(3, 7); AZ_CASE(4, 5); AZ_CASE(4, 9);
#undef AZ_CASE
    return nullptr;
}

static double *table_for(int displays)
{
    static double tabs[3][51 * T_STRIDE * 2];
    static bool built[3] = {false, false, false};
    const int i = displays == 5 ? 0 : displays == 7 ? 1 : 2;
    if (!built[i]) { if (!build_sample_pairs(5 * (displays + 1) + 1, tabs[i])) return nullptr; built[i] = true; }
    return tabs[i];
}

extern "C" {

// one runner call (azx::XRUN_*) on n_games games (wide records [N][256], MT19937 states [N][624] + positions [N], counters), two per wave.
// Returns the number of cross-lane operations executed, or a negative number on bad arguments.
long long shx_runner(int n_games, int players, int displays, uint8_t *state, u32 *mt, u32 *mtpos, u64 *episodes, u32 *stuck, double *stat_sum,
                     int first_player, int pool, int end_bonus, int short_deal, int op, const i32 *actions, const uint8_t *active, i32 *reward,
                     uint8_t *done, uint8_t *status, i32 *potential, int persp, float *obs, uint8_t *mask, uint8_t *player)
{
    lane_fn fn = pick_fn(players, displays);
    double *tab = table_for(displays);
    if (!fn || !tab || n_games <= 0) return -1;
    long long ops = 0;
    for (u32 w = 0; w < ((u32)n_games + 1u) / 2u; w++) {
        RJob *j = (RJob *)calloc(1, sizeof(RJob));
        j->b = {state, mt, mtpos, episodes, stuck, stat_sum, (u32)n_games, AZ_DRAW_MARGIN,
                {(u32)first_player, (u32)pool, (u32)end_bonus, (u32)short_deal}, (const double2 *)tab, nullptr};
        j->run.op = op; j->run.actions = actions; j->run.active = active; j->run.reward = reward; j->run.done = done; j->run.status = status;
        j->run.potential = potential; j->run.mask = mask; j->run.obs = obs; j->run.persp = persp; j->run.player = player;
        j->run.count = (u32)n_games;
        j->wave = w;
        ops += (long long)simt::run_wave(fn, j);
        free(j);
    }
    return ops;
}

}
