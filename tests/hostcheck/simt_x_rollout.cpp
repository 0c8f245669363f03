// simt_x_rollout.cpp -- TEST-ONLY: the window kernel of wide batches (x_policy_rollout_body of csrc/azul_rollout2.hpp, the body of
// azul_x_policy_rollout_kernel: env phases on azul_rules_x.hpp's P-seat GameRunner, matrix phases on v_mfma_f32_16x16x4_f32, the head of
// azul_policy_head_n_kernel), UNMODIFIED, as a workgroup of eight emulated wavefronts (simt/simt.hpp: run_workgroup).  The workgroup's LDS is
// declared here as azul_kernels.hip's wrapper declares it.  Built by tests/test_hostcheck_x_rollout.py with the flags of tests/hostcheck/Makefile.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_ops2.hpp"
#include "azul_policy.hpp"
#include "azul_rollout2.hpp"

struct XJob { azx::XBatchDev b; PolicyWeights W; RolloutArgs a; u32 id_base; };

template <u32 P, u32 D, int OPP>
static void lane_run(void *arg)
{
    __shared__ PXShared<P, D> S;
    XJob *j = (XJob *)arg;
    x_policy_rollout_body<P, D, OPP>(j->b, j->W, j->a, j->id_base, S);
}

typedef void (*lane_fn)(void *);
static lane_fn pick_fn(int players, int displays, int opp)
{
#define AZ_CASE(PP, DD) if (players == PP && displays == DD) return opp ? lane_run<PP, DD, 1> : lane_run<PP, DD, 0>
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

unsigned long long sxr_buffer_oob() { return simt::g_buffer_oob; }

// one launch over n_games wide records (a multiple of 16 or not: the last workgroup is ragged) for n_steps moves; `w` = the six weight
// arrays in the layouts of azul_policy_forward (w1t [obs_size][360], b1, w2c, b2c, w2a_t [180][NA], b2a).  Returns the number of
// cross-lane operations executed, or a negative number on bad arguments.
long long sxr_rollout(int n_games, int players, int displays, int opp, uint8_t *state, u32 *mt, u32 *mtpos, u64 *episodes, u32 *stuck,
                      double *stat_sum, int first_player, int pool, int end_bonus, int short_deal, unsigned id_base, const float *const *w, int n_steps,
                      float *obs, uint8_t *mask, uint8_t *player, i32 *action, i32 *reward, uint8_t *done, float *value, float *logp, float *entropy,
                      uint8_t *status, unsigned long long seed, unsigned long long counter)
{
    lane_fn fn = pick_fn(players, displays, opp);
    double *tab = table_for(displays);
    if (!fn || !tab || n_games <= 0) return -1;
    XJob j;
    memset(&j, 0, sizeof(j));
    j.b = {state, mt, mtpos, episodes, stuck, stat_sum, (u32)n_games, AZ_DRAW_MARGIN,
           {(u32)first_player, (u32)pool, (u32)end_bonus, (u32)short_deal}, (const double2 *)tab, nullptr};
    j.W = {w[0], w[1], w[2], w[3], w[4], w[5]};
    j.a.n_steps = n_steps; j.a.obs = obs; j.a.mask = mask; j.a.player = player; j.a.action = action; j.a.reward = reward; j.a.done = done;
    j.a.value = value; j.a.logp = logp; j.a.entropy = entropy; j.a.status = status; j.a.seed = seed; j.a.counter = counter;
    j.id_base = id_base;
    const unsigned blocks = ((unsigned)n_games + PF_GAMES - 1u) / PF_GAMES;
    simt::g_grid_dim = {blocks, 1, 1};
    long long ops = 0;
    for (unsigned blk = 0; blk < blocks; blk++) {
        simt::g_block_idx = {blk, 0, 0};
        ops += (long long)simt::run_workgroup(fn, &j, (int)PR2_WAVES);
    }
    return ops;
}

}
