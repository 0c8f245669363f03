// simt_net_x.cpp -- TEST-ONLY: the P-player GameRunner kernel with an external opponent (azul_x_net_kernel of csrc/azul_x_kernels.hpp on
// azx::net_body_x of csrc/azul_rules_x.hpp, UNMODIFIED) compiled by g++ and run lane by lane in lockstep (simt/simt.hpp) on host memory, so
// that it can be diffed against the model composed from the oracle (tests/mp_net_model.py) before a GPU sees it.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_x_kernels.hpp"
#include "simt_x_common.hpp"

struct NJob { azx::XBatchDev b; azx::XNet net; };

template <u32 P, u32 D>
static void lane_run(void *arg)
{
    NJob *j = (NJob *)arg;
    azul_x_net_kernel<P, D>(j->b, j->net);
}

extern "C" {

// one cut of the protocol (azx::XNET_*) on n_games games (wide records [N][256], MT19937 states [N][624] + positions [N], counters), two per
// wave.  Returns the number of cross-lane operations executed, or a negative number on bad arguments.
long long shx_net(int n_games, int players, int displays, uint8_t *state, u32 *mt, u32 *mtpos, u64 *episodes, u32 *stuck, double *stat_sum,
                  int first_player, int pool, int end_bonus, int short_deal, int op, const i32 *actions, const uint8_t *active, uint8_t *pending,
                  uint8_t *replies, i32 *reward, uint8_t *done, uint8_t *status, float *obs, uint8_t *mask, u32 *owing)
{
    lane_fn fn = x_for_shape(players, displays, [](auto s) { return (lane_fn)lane_run<s.P, s.D>; });
    if (!fn || n_games <= 0) return -1;
    NJob j;
    memset(&j, 0, sizeof(j));
    j.b = x_batch(n_games, state, mt, mtpos, episodes, stuck, stat_sum, first_player, pool, end_bonus, short_deal, nullptr);
    j.net.op = op; j.net.actions = actions; j.net.active = active; j.net.pending = pending; j.net.replies = replies;
    j.net.reward = reward; j.net.done = done; j.net.status = status; j.net.obs = obs; j.net.mask = mask; j.net.owing = owing;
    j.net.count = (u32)n_games;
    return x_launch(fn, &j, ((unsigned)n_games + 1u) / 2u, 1u);
}

}
