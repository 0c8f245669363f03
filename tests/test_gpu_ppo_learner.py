"""GPU: PPOLearner and BatchedTrainer(algorithm="ppo").  The fused path's flat gradient (azul_ppo_gradients, read from the learner's
workspace BEFORE the Adam step) against autograd's of loss_terms_ppo on the same window, under the bound of
tests/test_hostcheck_learner.py (3e-4 of each block's largest element); parameters after Adam steps are NOT compared between the two
paths (Adam's first steps are about lr * sign(g): an element whose gradient is rounding noise may legitimately move the other way).
Then the fused learner's epochs x minibatches schedule: step count, bit-identical twins, the statistics' meaning, a resumed learner;
and the trainer on two-player batches, wide batches on the PyTorch learner and wide batches fused, with a resume that replays the
next batch bit for bit."""
import copy
import os

import numpy as np
import pytest
import torch

from azul_deep_reinforcement_learning_amd import BatchedActorCritic
from azul_deep_reinforcement_learning_amd.learner import PPOLearner
from azul_deep_reinforcement_learning_amd.training import AGENT_STAT_KEYS, BatchedTrainer

pytestmark = pytest.mark.gpu

T, N = 8, 18
LOG_RATIOS = (0.5, -0.5, 0.05, -0.05)                         # far from both bounds of clip_eps = 0.2: no sample can change sides in f32


def _window(pol, seed, perturb):
    """18 games x 8 steps of synthetic records; value and log_prob are the policy's own (so the first step's ratio is 1), log_prob then
    shifted by LOG_RATIOS when `perturb`."""
    IN, A = pol.critic_linear1.in_features, pol.actor_linear2.out_features
    g = torch.Generator().manual_seed(seed)
    obs = torch.randint(0, 6, (T + 1, N, IN), generator=g).float()
    mask = (torch.rand(T + 1, N, A, generator=g) < 0.2).to(torch.uint8)
    action = torch.randint(0, A, (T, N), generator=g).to(torch.int32)
    mask[:T].scatter_(2, action.long().unsqueeze(2), 1)
    action[3, 5] = -1                                          # a record without an agent step
    mask[2, 7] = 0                                             # a stuck game: no legal action, no sample
    done = torch.zeros(T, N, dtype=torch.uint8)
    done[T - 1, :] = 1
    done[4, 2] = 1
    tr = {"obs": obs.cuda(), "mask": mask.cuda(), "action": action.cuda(), "done": done.cuda(), "returns": (3 * torch.randn(T, N, generator=g)).cuda()}
    with torch.no_grad():
        x, legal = tr["obs"][:T].reshape(T * N, IN), tr["mask"][:T].reshape(T * N, A).bool()
        legal = legal | ~legal.any(1, keepdim=True)
        h = torch.relu(torch.nn.functional.linear(x, torch.cat([pol.critic_linear1.weight, pol.actor_linear1.weight]),
                                                  torch.cat([pol.critic_linear1.bias, pol.actor_linear1.bias])))
        H = pol.critic_linear1.out_features
        tr["value"] = pol.critic_linear2(h[:, :H]).reshape(T, N, 1).contiguous()
        logp = torch.log_softmax(pol.actor_linear2(h[:, H:]).masked_fill(~legal, float("-inf")), dim=1)
        lp = logp.gather(1, tr["action"].reshape(-1).long().clamp(min=0).unsqueeze(1)).reshape(T, N)
        if perturb:
            lp = lp - torch.tensor(LOG_RATIOS, device="cuda").repeat(T * N // 4 + 1)[:T * N].reshape(T, N)
        tr["log_prob"] = lp.contiguous()
    return [tr]


def _policy(shape, seed):
    torch.manual_seed(seed)
    return BatchedActorCritic(shape[0], shape[1], 180).cuda()


def _flat_from_module_grads(lrn):
    pol, lay = lrn.policy, lrn.layout
    out = torch.zeros(lay["size"], device="cuda")
    v = lrn._views(out)
    v["w1t"].copy_(torch.cat([pol.critic_linear1.weight.grad, pol.actor_linear1.weight.grad], dim=0).t())
    v["b1"].copy_(torch.cat([pol.critic_linear1.bias.grad, pol.actor_linear1.bias.grad]))
    v["w2c"].copy_(pol.critic_linear2.weight.grad.reshape(-1))
    v["b2c"].copy_(pol.critic_linear2.bias.grad)
    v["w2a_t"].copy_(pol.actor_linear2.weight.grad.t())
    v["b2a"].copy_(pol.actor_linear2.bias.grad)
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", [(136, 180), (188, 180)], ids=["ref", "p3_d5"])
def test_fused_gradient_matches_autograd_before_the_adam_step(shape):
    pol = _policy(shape, 1)
    tr = _window(pol, 2, perturb=True)
    kw = dict(epochs=1, minibatches=1, shuffle_seed=3)
    fused, plain = PPOLearner(pol, fused=True, **kw), PPOLearner(copy.deepcopy(pol), fused=False, **kw)
    grabbed = []
    finish = fused._finish_fused
    fused._finish_fused = lambda *a: (grabbed.append(fused._ws["grad"].clone()), finish(*a))[1]
    out_f = fused.update_from_windows(tr)
    out_p = plain.update_from_windows(tr)
    torch.cuda.synchronize()
    assert len(grabbed) == 1 and fused.updates == plain.updates == 1 and int(fused._ws["step"]) == 1
    got, want = grabbed[0].cpu().numpy(), _flat_from_module_grads(plain)
    size = fused.layout["size"]
    n = int((tr[0]["action"] >= 0).sum())
    assert float(out_f["samples"]) == float(out_p["samples"]) == n == T * N - 1 and got[size + 3] == n - 1           # (the stuck game's row carries none)
    for k, (o, ln) in ((k, on) for k, on in fused.layout.items() if k != "size"):
        scale = max(1e-3, float(np.abs(want[o:o + ln]).max()))
        err = float(np.abs(got[o:o + ln] - want[o:o + ln]).max())
        print("BLOCK %s %s err %.3g scale %.3g" % (shape, k, err, scale))
        assert err < 3e-4 * scale, (k, err, scale)
    for k in ("actor_loss", "critic_loss", "entropy_loss", "ac_loss", "clip_fraction", "approx_kl"):
        a, b = float(out_f[k]), float(out_p[k])
        assert abs(a - b) <= 2e-5 * max(1.0, abs(b)) + 1e-6, (k, a, b)
    assert 0.4 < float(out_f["clip_fraction"]) < 0.6           # the +-0.5 half of LOG_RATIOS lies outside 1 +- 0.2
    assert abs(float(out_f["ac_loss"]) - (float(out_f["actor_loss"]) + 0.5 * float(out_f["critic_loss"]) - 0.01 * float(out_f["entropy_loss"]))) <= 1e-5


def _state(lrn):
    ws = lrn._ws
    return [p.detach().clone() for p in lrn.policy.parameters()] + [ws["flat"].clone(), ws["m"].clone(), ws["v"].clone(), ws["step"].clone()]


def _stats(lrn):
    return {k: [float(v) for v in d] for k, d in lrn.statistics.items()}


def test_fused_epochs_and_minibatches_twins_statistics_and_resume():
    shape = (136, 180)
    kw = dict(epochs=2, minibatches=3, shuffle_seed=7, fused=True)
    a, b = PPOLearner(_policy(shape, 5), **kw), PPOLearner(_policy(shape, 5), **kw)
    tr = _window(a.policy, 6, perturb=False)
    a.update_from_windows(tr)
    b.update_from_windows(tr)
    torch.cuda.synchronize()
    assert int(a._ws["step"]) == 6 and a.updates == 6 and a.u == 1
    assert all(torch.equal(x, y) for x, y in zip(_state(a), _state(b)))
    sa, sb = _stats(a), _stats(b)
    assert sa == sb and all(len(v) == 6 and np.isfinite(v).all() for v in sa.values())
    n = T * N - 1
    assert sa["samples"] == [float(len(c)) for c in np.array_split(np.arange(n), 3)] * 2
    # the window's log_prob is the policy's own: before the first step the ratio is 1 up to the f32 rounding of two evaluations
    assert sa["clip_fraction"][0] == 0.0 and abs(sa["approx_kl"][0]) <= 1e-5
    assert all(abs(k) < 0.1 for k in sa["approx_kl"]) and any(abs(k) > 1e-7 for k in sa["approx_kl"][1:])
    for i in range(6):
        assert abs(sa["ac_loss"][i] - (sa["actor_loss"][i] + 0.5 * sa["critic_loss"][i] - 0.01 * sa["entropy_loss"][i])) <= 1e-5 * max(1.0, abs(sa["ac_loss"][i]))
        assert sa["entropy_loss"][i] > 0.0 and sa["critic_loss"][i] > 0.0
    # the module and the flat master copy agree after the steps
    assert torch.equal(a._views(a._ws["flat"])["w2a_t"], a.policy.actor_linear2.weight.t())
    # a learner restored through optimizer_state() performs a bit-identical second call
    r = PPOLearner(_policy(shape, 99), **kw)
    r.policy.load_state_dict(copy.deepcopy(a.policy.state_dict()))
    r.load_optimizer_state(copy.deepcopy(a.optimizer_state()))
    tr2 = _window(a.policy, 8, perturb=True)
    a.update_from_windows(tr2)
    r.update_from_windows(tr2)
    torch.cuda.synchronize()
    assert r.u == 2 and int(r._ws["step"]) == 12 and all(torch.equal(x, y) for x, y in zip(_state(a), _state(r)))
    # an empty selection: no step, one entry of zeros
    before = _state(a)
    tr2[0]["done"].zero_()
    out = a.update_from_windows(tr2)
    assert all(torch.equal(x, y) for x, y in zip(before, _state(a))) and all(float(v) == 0.0 for v in out.values()) and a.updates == 13


TRAINERS = {
    "two-player": (lambda: BatchedActorCritic(136, 180, 180), dict(fused=True)),
    "two-player-greedy": (lambda: BatchedActorCritic(136, 180, 180), dict(opponent="greedy", fused=True)),
    "wide-pytorch": (lambda: BatchedActorCritic(188, 180, 180), dict(players=3, fused=False)),
    "wide-fused": (lambda: BatchedActorCritic(188, 180, 180), dict(players=3, fused_wide=True, fused_learner=True, fused=True)),
}


@pytest.mark.parametrize("name", list(TRAINERS))
def test_trainer_ppo_trains_and_resumes_bit_for_bit(name, tmp_path):
    net, kw = TRAINERS[name]
    kw = dict(kw)
    fused = kw.pop("fused")
    kw.update(n_games=33, window=8, ring=1, algorithm="ppo", epochs=2, minibatches=2, bootstrap_tail=True, gae_lambda=0.95,
              results_dir=str(tmp_path))
    torch.manual_seed(4)
    tr = BatchedTrainer(net(), seed_base=21, **kw)
    assert isinstance(tr.learner, PPOLearner) and tr.learner._use_fused(tr.rollout.traj[0]["obs"]) == fused

    def batch(t):
        row = t.run_batch()
        t.rollout.synchronize()
        torch.cuda.synchronize()
        assert all(np.isfinite(row[k]) for k in AGENT_STAT_KEYS[1:]), row
        n = int((t.rollout.traj[0]["action"] >= 0).sum())      # bootstrap_tail: every recorded step with an action is a sample
        assert n > 0 and sum(float(s) for s in list(t.learner.statistics["samples"])[-2:]) == n
        return row

    batch(tr)
    batch(tr)
    assert tr.learner.updates == 8 and tr.learner.u == 2
    if fused:
        assert int(tr.learner._ws["step"]) == 8
    ck = os.path.join(str(tmp_path), "ppo.pt")
    tr.save_checkpoint(ck)
    row_a = batch(tr)
    torch.manual_seed(99)
    tr2 = BatchedTrainer(net(), seed_base=9000, **kw)
    tr2.load_checkpoint(ck)
    assert tr2.learner.u == 2
    row_b = batch(tr2)
    for (k, x), y in zip(tr.rollout.policy.state_dict().items(), tr2.rollout.policy.state_dict().values()):
        assert torch.equal(x, y), k
    for k in AGENT_STAT_KEYS[1:]:
        assert row_a[k] == row_b[k], k
    assert list(tr.history)[:6] == ["batch"] + list(AGENT_STAT_KEYS)                         # the columns and their order


def test_trainer_a2c_default_is_untouched():
    tr = BatchedTrainer(BatchedActorCritic(136, 180, 180), n_games=8, window=8)
    assert tr.algorithm == "a2c" and type(tr.learner).__name__ == "A2CLearner" and tr.rollout.ring == 3
