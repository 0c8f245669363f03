// simt_net_x.cpp -- TEST-ONLY: the P-player GameRunner with an external opponent (azx::net_body_x of csrc/azul_rules_x.hpp, the body of
// azul_x_net_kernel, UNMODIFIED) compiled by g++ and run lane by lane in lockstep (simt/simt.hpp) on host memory, so that it can be diffed
// against the model composed from the oracle (tests/mp_net_model.py) before a GPU sees it.  Built by tests/test_hostcheck_net_x.py with the
// flags of tests/hostcheck/Makefile.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
#include "azul_selfplay2.hpp"
#include "azul_rules_x.hpp"

using namespace az;

struct NJob {
    azx::XBatchDev b;
    azx::XNet net;
    u32 wave;
    u32 mt_lds[2][624];
};

template <u32 P, u32 D>
static void lane_run(void *arg)
{
    NJob *j = (NJob *)arg;
    azx::net_body_x<P, D>(j->b, j->net, j->wave, j->mt_lds);
}

typedef void (*lane_fn)(void *);
static lane_fn pick_fn(int players, int displays)
{
#define AZ_CASE(PP, DD) if (players == PP && displays == DD) return lane_run<PP, DD>
    AZ_CASE(2, 5); AZ_CASE(3, 5); AZ_CASE(3, 7); AZ_CASE(4, 5); AZ_CASE(4, 9);
#undef AZ_CASE
    return nullptr;
}

extern "C" {

// one cut of the protocol (azx::XNET_*) on n_games games (wide records [N][256], MT19937 states [N][624] + positions [N], counters), two per
// wave.  Returns the number of cross-lane operations executed, or a negative number on bad arguments.
long long shx_net(int n_games, int players, int displays, uint8_t *state, u32 *mt, u32 *mtpos, u64 *episodes, u32 *stuck, double *stat_sum,
                  int first_player, int pool, int end_bonus, int short_deal, int op, const i32 *actions, const uint8_t *active, uint8_t *pending,
                  uint8_t *replies, i32 *reward, uint8_t *done, uint8_t *status, float *obs, uint8_t *mask, u32 *owing)
{
    lane_fn fn = pick_fn(players, displays);
    if (!fn || n_games <= 0) return -1;
    long long ops = 0;
    for (u32 w = 0; w < ((u32)n_games + 1u) / 2u; w++) {
        NJob *j = (NJob *)calloc(1, sizeof(NJob));
        j->b = {state, mt, mtpos, episodes, stuck, stat_sum, (u32)n_games, AZ_DRAW_MARGIN,
                {(u32)first_player, (u32)pool, (u32)end_bonus, (u32)short_deal}, nullptr, nullptr};
        j->net.op = op; j->net.actions = actions; j->net.active = active; j->net.pending = pending; j->net.replies = replies;
        j->net.reward = reward; j->net.done = done; j->net.status = status; j->net.obs = obs; j->net.mask = mask; j->net.owing = owing;
        j->net.count = (u32)n_games;
        j->wave = w;
        ops += (long long)simt::run_wave(fn, j);
        free(j);
    }
    return ops;
}

}
