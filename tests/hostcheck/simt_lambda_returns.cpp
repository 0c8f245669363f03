// simt_lambda_returns.cpp -- TEST-ONLY: the TD(lambda) returns scan over a trajectory ring (csrc/azul_selfplay_kernels.hpp:
// azul_lambda_returns_ring_kernel), UNMODIFIED, as one-wave workgroups of the lockstep lane emulation (simt/simt.hpp), launched as
// azul_lambda_returns_ring launches it -- a CPU check of its float32 arithmetic against the host model of the header's contract
// (tests/lambda_returns_cases.py) and of every index it forms.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_selfplay_kernels.hpp"

struct LamJob { const i32 *reward; const uint8_t *done; const float *value, *tail; float *out; float gamma, lambda; int ring_steps, s_end, span; u32 n; };
static void lam_lane(void *arg)
{
    LamJob *j = (LamJob *)arg;
    azul_lambda_returns_ring_kernel(j->reward, j->done, j->value, j->tail, j->out, j->gamma, j->lambda, j->ring_steps, j->s_end, j->span, j->n);
}

extern "C" {

unsigned long long slr_buffer_oob() { return simt::g_buffer_oob; }

// the entry's launch: the host reduces the step clock to the slot behind the newest step, 64 games per one-wave workgroup
long long slr_lambda_returns_ring(const i32 *reward, const uint8_t *done, const float *value, const float *tail, float *out, float gamma,
                                  float lambda, int ring_steps, long long steps_played, int span, int n)
{
    LamJob j = {reward, done, value, tail, out, gamma, lambda, ring_steps,
                (int)(steps_played % ring_steps == 0 ? ring_steps : steps_played % ring_steps), span, (u32)n};
    const unsigned blocks = ((unsigned)n + 63u) / 64u;
    simt::g_grid_dim = {blocks, 1, 1};
    long long ops = 1;
    for (unsigned blk = 0; blk < blocks; blk++) {
        simt::g_block_idx = {blk, 0, 0};
        ops += (long long)simt::run_workgroup(lam_lane, &j, 1);
    }
    return ops;
}

}
