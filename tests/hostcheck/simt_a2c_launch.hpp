// simt_a2c_launch.hpp -- TEST-ONLY: the launches simt_learner.cpp, simt_learner_n.cpp and simt_ppo.cpp share: a shape's gradient kernel on
// its grid, the reduce behind it, and azul_a2c_apply_adam_n's step counter + Adam step.  Which kernel serves a shape, on which grid and
// arguments, is the library's own choice (csrc/azul_learner.hpp: a2c_grad, a2c_reduce_launch, a2c_apply_launch; a2c_gradients and
// a2c_apply_adam of csrc/azul_kernels.hip launch through the same).  Included after csrc/azul_learner.hpp.
#pragma once

static const auto a2c_call = [](auto kernel, auto... args) { kernel(args...); };      // "launch": this lane calls the kernel

// the gradient kernel of (in, act) for objective obj on `parts` parts; 0 where the shape has none
struct GradJob { A2CGrad g; PolicyWeights W; LearnerArgs a; };
static void grad_lane(void *arg) { GradJob *j = (GradJob *)arg; j->g.kernel(j->W, j->a); }
static long long run_gradients(int in, int act, int obj, const PolicyWeights &W, const LearnerArgs &a, int parts)
{
    GradJob j = {a2c_grad(in, act, obj), W, a};
    if (!j.g.kernel) return 0;
    simt::g_grid_dim = {(unsigned)parts, j.g.roles, 1};
    long long ops = 0;
    for (unsigned role = 0; role < j.g.roles; role++)
        for (int blk = 0; blk < parts; blk++) {
            simt::g_block_idx = {(unsigned)blk, role, 0};
            ops += (long long)simt::run_workgroup(grad_lane, &j, (int)j.g.waves, 512u << 10);
        }
    return ops;
}

struct RedJob { A2CShapeN S; const float *partial; u32 parts; float *grad; };
static void red_lane(void *arg)
{
    RedJob *j = (RedJob *)arg;
    a2c_reduce_launch(j->S, a2c_call, j->partial, j->parts, j->grad);
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
    else a2c_apply_launch(j->S, a2c_call, j->grad, j->flat, j->m, j->v, j->lr, j->b1, j->b2, j->eps, j->bc1, j->bc2s, j->P, j->step, j->n_total, 0.f, j->stats);
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
