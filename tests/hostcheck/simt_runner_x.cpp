// simt_runner_x.cpp -- TEST-ONLY: the P-player GameRunner kernel (azul_x_runner_kernel of csrc/azul_x_kernels.hpp on azx::runner_body_x of
// csrc/azul_rules_x.hpp, UNMODIFIED) compiled by g++ and run lane by lane in lockstep (simt/simt.hpp) on host memory, so that it can be
// diffed against the model composed from the oracle (tests/mp_runner_model.py) before a GPU sees it.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_x_kernels.hpp"
#include "simt_x_common.hpp"

struct RJob { azx::XBatchDev b; azx::XRun run; };

template <u32 P, u32 D>
static void lane_run(void *arg)
{
    RJob *j = (RJob *)arg;
    azul_x_runner_kernel<P, D>(j->b, j->run);
}

extern "C" {

// one runner call (azx::XRUN_*) on n_games games (wide records [N][256], MT19937 states [N][624] + positions [N], counters), two per wave.
// Returns the number of cross-lane operations executed, or a negative number on bad arguments.
long long shx_runner(int n_games, int players, int displays, uint8_t *state, u32 *mt, u32 *mtpos, u64 *episodes, u32 *stuck, double *stat_sum,
                     int first_player, int pool, int end_bonus, int short_deal, int op, const i32 *actions, const uint8_t *active, i32 *reward,
                     uint8_t *done, uint8_t *status, i32 *potential, int persp, float *obs, uint8_t *mask, uint8_t *player)
{
    lane_fn fn = x_for_shape(players, displays, [](auto s) { return (lane_fn)lane_run<s.P, s.D>; });
    const double2 *tab = table_for(displays);
    if (!fn || !tab || n_games <= 0) return -1;
    RJob j;
    memset(&j, 0, sizeof(j));
    j.b = x_batch(n_games, state, mt, mtpos, episodes, stuck, stat_sum, first_player, pool, end_bonus, short_deal, tab);
    j.run.op = op; j.run.actions = actions; j.run.active = active; j.run.reward = reward; j.run.done = done; j.run.status = status;
    j.run.potential = potential; j.run.mask = mask; j.run.obs = obs; j.run.persp = persp; j.run.player = player;
    j.run.count = (u32)n_games;
    return x_launch(fn, &j, ((unsigned)n_games + 1u) / 2u, 1u);
}

}
