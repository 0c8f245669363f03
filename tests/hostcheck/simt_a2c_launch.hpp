// simt_a2c_launch.hpp -- TEST-ONLY: the launches simt_learner.cpp and simt_learner_n.cpp share, as the host entries perform them
// (csrc/azul_kernels.hip): the reduce behind a gradient kernel, and azul_a2c_apply_adam_n's step counter + Adam step -- the reference
// shape through azul_a2c_reduce_kernel / azul_a2c_apply_kernel, every other shape through the _n entries.  Included after
// csrc/azul_learner.hpp.
#pragma once

static bool a2c_is_reference(const A2CShapeN &S) { return S.in == (u32)PF_IN && S.act == (u32)PF_ACT; }

struct RedJob { A2CShapeN S; const float *partial; u32 parts; float *grad; };
static void red_lane(void *arg)
{
    RedJob *j = (RedJob *)arg;
    if (a2c_is_reference(j->S)) azul_a2c_reduce_kernel(j->partial, j->parts, j->grad);
    else azul_a2c_reduce_n_kernel(j->partial, j->parts, j->S.params + 4u, j->grad);
}
static long long run_reduce(A2CShapeN S, const float *partial, int parts, float *grad)
{
    RedJob j = {S, partial, (u32)parts, grad};
    const unsigned blocks = (S.params + 4u + 255u) / 256u;
    simt::g_grid_dim = {blocks, 1, 1};
    long long ops = 1;
    for (unsigned blk = 0; blk < blocks; blk++) { simt::g_block_idx = {blk, 0, 0}; ops += (long long)simt::run_workgroup(red_lane, &j, 4, 128u << 10); }
    return ops;
}

// step: the device step counter (advanced first, like azul_a2c_apply_adam_n does), or NULL with the host's bias corrections bc1 / bc2s
struct AdamJob { A2CShapeN S; const float *grad; float *flat, *m, *v; float lr, b1, b2, eps, bc1, bc2s; ModuleParams P; i32 *step; const float *n_total; float *stats; int phase; };
static void adam_lane(void *arg)
{
    AdamJob *j = (AdamJob *)arg;
    if (j->phase == 0) azul_a2c_step_kernel(j->step, j->n_total);
    else if (a2c_is_reference(j->S))
        azul_a2c_apply_kernel(j->grad, j->flat, j->m, j->v, j->lr, j->b1, j->b2, j->eps, j->bc1, j->bc2s, j->P, j->step, j->n_total, 0.f, j->stats);
    else
        azul_a2c_apply_n_kernel(j->S, j->grad, j->flat, j->m, j->v, j->lr, j->b1, j->b2, j->eps, j->bc1, j->bc2s, j->P, j->step, j->n_total, 0.f, j->stats);
}
static long long run_adam(AdamJob &j)
{
    long long ops = 1;
    if (j.step) {
        j.phase = 0;
        simt::g_grid_dim = {1, 1, 1};
        simt::g_block_idx = {0, 0, 0};
        ops += (long long)simt::run_workgroup(adam_lane, &j, 1);
    }
    j.phase = 1;
    const unsigned blocks = (j.S.params + 255u) / 256u;
    simt::g_grid_dim = {blocks, 1, 1};
    for (unsigned blk = 0; blk < blocks; blk++) {
        simt::g_block_idx = {blk, 0, 0};
        ops += (long long)simt::run_workgroup(adam_lane, &j, 4, 128u << 10);
    }
    return ops;
}
