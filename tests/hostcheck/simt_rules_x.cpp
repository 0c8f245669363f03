// simt_rules_x.cpp -- TEST-ONLY: the rule kernel and the flat self-play kernel of WIDE batches (azul_x_op_kernel and azul_x_selfplay_kernel
// of csrc/azul_x_kernels.hpp on csrc/azul_rules_x.hpp, all UNMODIFIED) compiled by g++ and run lane by lane in lockstep (simt/simt.hpp),
// one emulated workgroup per pair of games with the kernels' own LDS and blockIdx -> game placement, so that they can be diffed against
// the oracle -- and run under UBSan / ASan -- in the build container, before a GPU sees them.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_x_kernels.hpp"
#include "simt_x_common.hpp"

struct XJob { azx::XBatchDev b; azx::XOp op; azx::XTraj t; int variant; };

template <u32 P, u32 D>
static void lane_op(void *arg)
{
    XJob *j = (XJob *)arg;
    azul_x_op_kernel<P, D>(j->b, j->op);
}

template <u32 P, u32 D>
static void lane_play(void *arg)
{
    XJob *j = (XJob *)arg;
    switch (j->variant) {
    case 0: azul_x_selfplay_kernel<P, D, 1, true, true>(j->b, j->t); break;
    case 1: azul_x_selfplay_kernel<P, D, 1, true, false>(j->b, j->t); break;
    case 3: azul_x_selfplay_kernel<P, D, 2, false, false>(j->b, j->t); break;
    default: azul_x_selfplay_kernel<P, D, 0, false, false>(j->b, j->t); break;
    }
}

extern "C" {

// n_games games (wide records [N][256], MT19937 states [N][624] + positions [N], counters) advance by n_steps moves, two per wave, on
// the launch's own grid of ceil(n_games / 2) blocks.  variant: 0 = OUT 1 / PAD / BITS, 1 = OUT 1 / PAD, 3 = OUT 2 (run-time subset),
// 4 = OUT 0.  Returns the number of cross-lane operations executed, or a negative number on bad arguments.
long long shx_selfplay(int n_games, int players, int displays, uint8_t *state, u32 *mt, u32 *mtpos, u64 *episodes, u32 *stuck, double *stat_sum,
                       int first_player, int pool, int end_bonus, int short_deal, unsigned long long margin, int n_steps, int variant,
                       uint8_t *mask, int pitch, u64 *maskbits, i32 *action, i32 *reward, uint8_t *done, u32 *packed, uint8_t *rec)
{
    lane_fn fn = x_for_shape(players, displays, [](auto s) { return (lane_fn)lane_play<s.P, s.D>; });
    const double2 *tab = table_for(displays);
    if (!fn || !tab || n_games <= 0 || n_steps < 0) return -1;
    XJob j;
    memset(&j, 0, sizeof(j));
    j.b = x_batch(n_games, state, mt, mtpos, episodes, stuck, stat_sum, first_player, pool, end_bonus, short_deal, tab, margin);
    j.t = {n_steps, mask, maskbits, action, reward, done, rec, packed, (u32)pitch};
    j.variant = variant;
    return x_launch(fn, &j, ((unsigned)n_games + 1u) / 2u, 1u);
}

// one rule call on ONE game (the wave's other half stays idle): record [256], stream (624 words + index), results on request
int shx_op(uint8_t *rec, int players, int displays, int first_player, int pool, int end_bonus, int short_deal, unsigned long long margin, int op,
           int action, u32 *mt, u32 *pos, const uint8_t *mask_in, uint8_t *mask_out, float *obs, int persp, int *flags, double *stats10,
           int *action_out, int *player, int *rng_dirty, int *next_action /* NULL: not asked for */, unsigned pos_set /* 0, or 1 + index */)
{
    lane_fn fn = x_for_shape(players, displays, [](auto s) { return (lane_fn)lane_op<s.P, s.D>; });
    const double2 *tab = table_for(displays);
    if (!fn || !tab) return -1;
    u64 episodes = 0; u32 stuck = 0; double stat_sum[10] = {0};
    XJob j;
    memset(&j, 0, sizeof(j));
    j.b = x_batch(1, rec, mt, pos, &episodes, &stuck, stat_sum, first_player, pool, end_bonus, short_deal, tab, margin);
    i32 act_in = action, act_out = 0, nxt = -2;
    uint8_t status = 0, fl = 0, pl = 0, rd = 0;
    j.op.op = op; j.op.actions = &act_in; j.op.mask_in = mask_in; j.op.actions_out = &act_out; j.op.status = &status;
    j.op.mask = mask_out; j.op.obs = obs; j.op.persp = persp; j.op.flags = &fl; j.op.stats = stats10; j.op.player = &pl;
    j.op.rng_dirty = &rd; j.op.first = 0; j.op.count = 1;
    j.op.next_action = next_action ? &nxt : nullptr; j.op.pos_set = pos_set;
    x_launch(fn, &j, 1u, 1u);
    if (flags) *flags = fl;
    if (action_out) *action_out = act_out;
    if (player) *player = pl;
    if (rng_dirty) *rng_dirty = rd;
    if (next_action) *next_action = nxt;
    return status;
}

}
