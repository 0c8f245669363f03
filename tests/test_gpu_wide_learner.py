"""GPU: the fused learner of wide batches -- azul_a2c_gradients on the four wide shapes ActorCritic(obs_size, num_actions, hidden 180)
against PyTorch autograd, azul_a2c_apply_adam_n against torch.optim.Adam, the trajectory ring of the wide window kernel
(PolicyRollout(fused_wide=True, wide_ring=k): every step of every finished episode trained exactly once, as NNRunner.train does,
nn_runner.py:59-76) and BatchedTrainer(fused_learner=True) with an exact resume."""
import ctypes as C

import numpy as np
import pytest
import torch

from azul_deep_reinforcement_learning_amd import _lib as L
from azul_deep_reinforcement_learning_amd.learner import A2CLearner
from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
from azul_deep_reinforcement_learning_amd.rollout import PolicyRollout

pytestmark = pytest.mark.gpu

# (players, rules) -> ActorCritic(obs_size, num_actions, 180)
WIDE = {
    "p3_d5": (3, {"first_player": "Random", "tile_pool": "Lid"}, 188, 180),
    "p4_d5": (4, {"first_player": "Random", "tile_pool": "Lid"}, 240, 180),
    "p3_d7": (3, {"first_player": "Random", "tile_pool": "Lid", "displays": "2P+1"}, 198, 240),
    "p4_d9": (4, {"first_player": "Random", "tile_pool": "Random", "displays": "2P+1", "short_deal": True}, 260, 300),
}


def _net(name, seed=0):
    _, _, n_obs, n_act = WIDE[name]
    torch.manual_seed(seed)
    return BatchedActorCritic(n_obs, n_act, 180).cuda()


def _random_samples(n, n_obs, n_act, seed):
    rs = np.random.RandomState(seed)
    obs = torch.from_numpy(rs.randint(0, 6, size=(n, n_obs)).astype(np.float32)).cuda()
    m = rs.rand(n, n_act) < 0.2
    m[np.arange(n), rs.randint(0, n_act, n)] = True
    act = np.array([rs.choice(np.flatnonzero(m[i])) for i in range(n)]) if n <= 5000 else \
        np.argmax(m * rs.rand(n, n_act), axis=1)                  # (a legal action of every row, vectorised)
    if n > 100:
        m[5] = False                                         # rows without a legal action carry no sample
        m[n - 1] = False
    q = rs.randn(n).astype(np.float32) * 5
    return obs, torch.from_numpy(m).cuda(), torch.from_numpy(act).cuda(), torch.from_numpy(q).cuda()


def _grads(learner, obs, mask, act, q):
    """The fused path's flat gradient (+ the four sums) for the given samples, parameters untouched."""
    n = obs.shape[0]
    learner._fused_gradients(obs, mask, act, q, n_total=n)
    return learner._ws["grad"].clone()


@pytest.mark.parametrize("name", list(WIDE))
@pytest.mark.parametrize("n", [48, 5000, 131072])
def test_wide_gradients_match_autograd(name, n):
    _, _, n_obs, n_act = WIDE[name]
    obs, mask, act, q = _random_samples(n, n_obs, n_act, n + n_obs)
    ref, net = _net(name), _net(name)
    # samples with a hidden pre-activation within 1e-4 of the ReLU kink are left out: there the f32 forward and the f64 reference may
    # take different sides of relu' and the sample's whole contribution to that unit's gradient row differs (not an error of either)
    with torch.no_grad():
        w1 = torch.cat([ref.critic_linear1.weight, ref.actor_linear1.weight], 0).double()
        b1 = torch.cat([ref.critic_linear1.bias, ref.actor_linear1.bias]).double()
        pre = obs.double() @ w1.t() + b1
        clear = (pre.abs() >= 1e-4).all(dim=1)
    obs, mask, act, q = obs[clear], mask[clear], act[clear], q[clear]
    n = obs.shape[0]
    keep = mask.bool().any(dim=1)
    scale_ref = float(keep.sum()) / n
    # the reference in float64 (fp32 autograd itself drifts by more than the tolerance on 10^5 samples of cancelling terms)
    ref = ref.double()
    lr = A2CLearner(ref, distributed=False, fused=False)
    a, c, e, loss = lr.loss_terms(obs[keep].double(), mask[keep], act[keep], q[keep].double())
    loss.backward()
    fl = A2CLearner(net, distributed=False, fused=True)
    g = _grads(fl, obs, mask, act, q)
    v = fl._views(g)
    H = 180
    got = {"critic_linear1.weight": v["w1t"][:, :H].t(), "actor_linear1.weight": v["w1t"][:, H:].t(), "critic_linear1.bias": v["b1"][:H],
           "actor_linear1.bias": v["b1"][H:], "critic_linear2.weight": v["w2c"].view(1, H), "critic_linear2.bias": v["b2c"],
           "actor_linear2.weight": v["w2a_t"].t(), "actor_linear2.bias": v["b2a"]}
    for name_, pr in ref.named_parameters():
        rg = pr.grad * scale_ref
        scale = float(rg.abs().max()) + 1e-12
        err = float((rg - got[name_].double()).abs().max())
        assert err <= 2e-5 * scale + 1e-7, (name_, err, scale)
    sums = g[fl.layout["size"]:].cpu()
    assert int(sums[3]) == int(keep.sum())
    for k, (want, got_) in enumerate(zip((a, c, e), sums[:3])):
        assert np.isclose(float(want.detach()) * scale_ref, float(got_) / n, rtol=2e-5, atol=1e-6), k
    # the same call twice: bit-identical
    assert torch.equal(g, _grads(fl, obs, mask, act, q))
    if n < 6000 and n > 100:
        # through index_dev / n_samples_dev / inv_n_total_dev: the selected rows of a larger array
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(7)).cuda()
        big = [torch.cat([t, t.flip(0)]) for t in (obs, mask, act, q)]
        index = perm.to(torch.int32).contiguous()
        count = torch.tensor([n], dtype=torch.int32, device="cuda")
        countf = torch.tensor([float(n), 1.0 / n], device="cuda")
        fl._fused_gradients(*big, index=index, count=count, countf=countf)
        gi = fl._ws["grad"]
        assert float((gi[:fl.layout["size"]] - g[:fl.layout["size"]]).abs().max()) <= 2e-5 * float(g.abs().max()) + 1e-7


@pytest.mark.parametrize("name", ["p3_d5", "p4_d9"])
def test_wide_adam_matches_torch_adam(name):
    _, _, n_obs, n_act = WIDE[name]
    ref, net = _net(name, 3), _net(name, 3)
    fl = A2CLearner(net, distributed=False, fused=True)
    opt = torch.optim.Adam(ref.parameters(), lr=3e-4)
    for step in range(4):
        obs, mask, act, q = _random_samples(300, n_obs, n_act, 50 + step)
        fl.update(obs, mask, act, q)
        # torch.optim.Adam on the kernel's own gradient of this step (the gradient is left in the workspace)
        v = fl._views(fl._ws["grad"])
        H = 180
        gd = {"critic_linear1.weight": v["w1t"][:, :H].t(), "actor_linear1.weight": v["w1t"][:, H:].t(), "critic_linear1.bias": v["b1"][:H],
              "actor_linear1.bias": v["b1"][H:], "critic_linear2.weight": v["w2c"].view(1, H), "critic_linear2.bias": v["b2c"],
              "actor_linear2.weight": v["w2a_t"].t(), "actor_linear2.bias": v["b2a"]}
        for k, p_ in ref.named_parameters():
            p_.grad = gd[k].clone().contiguous()
        opt.step()
        torch.cuda.synchronize()
        for (k, pr), (_, pg) in zip(ref.named_parameters(), net.named_parameters()):
            assert torch.allclose(pr, pg, rtol=0, atol=2e-6), (step, k, float((pr - pg).abs().max()))
    # module, flat copy and moments agree
    kw = fl.kweights()
    assert torch.equal(kw["w1t"], torch.cat([net.critic_linear1.weight, net.actor_linear1.weight], dim=0).t())
    assert torch.equal(kw["w2a_t"], net.actor_linear2.weight.t()) and torch.equal(kw["b2a"], net.actor_linear2.bias)
    mv = fl._views(fl._ws["m"])
    st = opt.state[ref.actor_linear2.weight]
    assert torch.allclose(mv["w2a_t"].t(), st["exp_avg"], rtol=0, atol=1e-7)
    assert int(fl._ws["step"].item()) == 4
    # an update with zero samples is a no-op: parameters, moments and step untouched
    before = {k: v_.detach().clone() for k, v_ in net.state_dict().items()}
    m0, s0 = fl._ws["m"].clone(), int(fl._ws["step"].item())
    obs, mask, act, q = _random_samples(32, n_obs, n_act, 99)
    idx = torch.zeros(32, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    countf = torch.tensor([0.0, 1.0], device="cuda")
    fl._finish_fused(*fl._fused_gradients(obs, mask, act, q, index=idx, count=count, countf=countf))
    torch.cuda.synchronize()
    for k, v_ in net.state_dict().items():
        assert torch.equal(v_, before[k]), k
    assert torch.equal(fl._ws["m"], m0) and int(fl._ws["step"].item()) == s0


def _ring_rollout(name, n, T, D, fused_opponent, learner=None, seed=321):
    players, rules, _, _ = WIDE[name]
    net = _net(name, 1)
    kw = dict(n_games=n, seed_base=seed, window=T, rules=rules, players=players, fused_wide=True, wide_ring=D)
    if fused_opponent:
        kw.update(opponent=_net(name, 2), fused_opponent=True)
    else:
        kw.update(opponent="random")
    if learner is not None:
        kw.update(kweights=learner.kweights())
    return net, PolicyRollout(net, **kw)


@pytest.mark.parametrize("name", ["p3_d5", "p4_d9"])
@pytest.mark.parametrize("fused_opponent", [False, True], ids=["random", "net_opponent"])
def test_wide_ring_trains_every_step_exactly_once(name, fused_opponent):
    """The wide version of test_learner.py's ring test: every (game, step) of every finished episode reaches the learner's selection
    exactly once, with the Monte-Carlo return of its whole episode history; opening steps are trained in a later window than the one
    that recorded them; nothing falls out of the ring."""
    n, T, D, windows, gamma = 128, 16, 12, 30, 0.99
    net, ro = _ring_rollout(name, n, T, D, fused_opponent)
    assert ro.ring == D
    fl = A2CLearner(net, distributed=False, fused=True)
    fl.optimizer = torch.optim.SGD(net.parameters(), lr=0.0)     # keep the parameters: only the selection is checked
    R = D * T
    hist = {k: [] for k in ("action", "reward", "done")}
    seen, later = {}, 0
    for w in range(windows):
        tr = ro.run_window(gamma)
        ro.synchronize()
        for k in hist:
            hist[k].append(tr[0][k].cpu().numpy().copy())
        fl.update_from_rollout(ro)
        torch.cuda.synchronize()
        st = fl._ring
        cnt = int(st["count"][0])
        idx = st["index"][:cnt].cpu().numpy().astype(np.int64)
        rets = ro.rings[0]["returns"].reshape(-1)[st["index"][:cnt].long()].cpu().numpy()
        slot, game = idx // n, idx % n
        end = (w + 1) * T - 1
        absstep = end - ((end % R - slot) % R)
        assert np.all(np.diff(game) >= 0)
        for gm, s_, rv in zip(game, absstep, rets):
            assert (int(gm), int(s_)) not in seen, "step trained twice"
            seen[(int(gm), int(s_))] = float(rv)
            later += int(s_ < w * T)                         # recorded in an earlier window than this update's
    assert int(fl.dropped_steps[1]) == 0
    assert later > 0
    action, reward, done = (np.concatenate(hist[k]) for k in ("action", "reward", "done"))
    total = 0
    for gm in range(n):
        ends = np.flatnonzero(done[:, gm] != 0)
        if len(ends) == 0:
            assert not any(g2 == gm for (g2, _) in seen)
            continue
        last = ends[-1]
        qv = 0.0
        for s_ in range(last, -1, -1):
            if done[s_, gm] != 0:
                qv = 0.0
            qv = reward[s_, gm] + gamma * qv
            if action[s_, gm] >= 0:
                assert (gm, s_) in seen, "step of a finished episode never trained: game %d step %d" % (gm, s_)
                assert abs(seen[(gm, s_)] - qv) <= 1e-3 + 1e-4 * abs(qv)
                total += 1
        assert all(s_ <= last for (g2, s_) in seen if g2 == gm)
    assert total == len(seen) and total > n * 20


@pytest.mark.parametrize("name", ["p3_d5", "p4_d9"])
def test_fused_wide_update_equals_pytorch_update(name):
    """One fused update on the ring selection lands on the parameters of a PyTorch A2CLearner.update over the same samples."""
    n, T, D, gamma = 256, 16, 3, 0.99
    net, ro = _ring_rollout(name, n, T, D, False)
    fl = A2CLearner(net, distributed=False, fused=True)
    for _ in range(5):
        ro.run_window(gamma)
        fl.update_from_rollout(ro)
    ref = _net(name, 0).double()                             # the PyTorch update in float64: the yardstick, not another f32 rounding
    ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    fl.sync_from_module()
    ro.run_window(gamma)
    ro.synchronize()
    pl = A2CLearner(ref, distributed=False, fused=False)
    fl2 = A2CLearner(net, distributed=False, fused=True)     # a fresh Adam on both sides: first step from equal parameters
    fl2._ring = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in fl._ring.items()}
    fl2.update_from_rollout(ro)
    torch.cuda.synchronize()
    st = fl2._ring
    cnt = int(st["count"][0])
    assert cnt > 0
    idx = st["index"][:cnt].long()
    rg = ro.rings[0]
    R = D * T
    obs = rg["obs"][:R].reshape(R * n, -1)[idx].double()
    mask = rg["mask"][:R].reshape(R * n, -1)[idx]
    act = rg["action"].reshape(-1)[idx]
    ret = rg["returns"].reshape(-1)[idx].double()
    # hidden units that some selected sample drives to within 1e-4 of the ReLU kink: there f32 and f64 may take different sides of
    # relu' (a whole sample's contribution to that unit's rows of the first layer) -- those rows are not compared
    with torch.no_grad():
        w1 = torch.cat([ref.critic_linear1.weight, ref.actor_linear1.weight], 0)
        b1 = torch.cat([ref.critic_linear1.bias, ref.actor_linear1.bias])
        kink = ((obs @ w1.t() + b1).abs() < 1e-4).any(dim=0)
    H = 180
    rows = {"critic_linear1.weight": ~kink[:H], "critic_linear1.bias": ~kink[:H], "actor_linear1.weight": ~kink[H:], "actor_linear1.bias": ~kink[H:]}
    before = {k: v.detach().clone() for k, v in ref.named_parameters()}
    pl.update(obs, mask, act, ret)
    torch.cuda.synchronize()
    v = fl2._views(fl2._ws["grad"])
    got = {"critic_linear1.weight": v["w1t"][:, :H].t(), "actor_linear1.weight": v["w1t"][:, H:].t(), "critic_linear1.bias": v["b1"][:H],
           "actor_linear1.bias": v["b1"][H:], "critic_linear2.weight": v["w2c"].view(1, H), "critic_linear2.bias": v["b2c"],
           "actor_linear2.weight": v["w2a_t"].t(), "actor_linear2.bias": v["b2a"]}
    for (k, pr), (_, pg) in zip(ref.named_parameters(), net.named_parameters()):
        keep = rows.get(k)
        sel = (lambda t: t[keep]) if keep is not None else (lambda t: t)
        gr, gg = sel(pr.grad), sel(got[k].double())
        scale = float(gr.abs().max()) + 1e-12
        assert float((gr - gg).abs().max()) <= 2e-5 * scale + 1e-7, k
        # Adam's first step is lr * g / (|g| + eps): wherever the gradient is not tiny both sides take the same step
        big = gr.abs() > 1e-4 * scale
        assert float(((sel(pr) - sel(pg).double()).detach().abs() * big).max()) <= 1e-6, k
        assert float((sel(pr) - sel(before[k])).detach().abs()[big].min()) > 0.0           # ... and every such parameter moved
    assert int((~kink).sum()) > 90                          # (most units are still compared)


def _trainer(tmp_path, seed):
    from azul_deep_reinforcement_learning_amd.training import BatchedTrainer
    players, rules, n_obs, n_act = WIDE["p3_d5"]
    torch.manual_seed(seed)
    return BatchedTrainer(BatchedActorCritic(n_obs, n_act, 180), n_games=256, window=16, players=players, rules=rules, device="cuda:0",
                          fused_wide=True, fused_learner=True, results_dir=str(tmp_path))


def test_fused_learner_trainer_trains_and_resumes_exactly(tmp_path):
    tr = _trainer(tmp_path, 0)
    assert tr.rollout.ring == 3 and tr.learner.fused is True
    assert tr.rollout.w1t.data_ptr() == tr.learner.kweights()["w1t"].data_ptr()        # one weight copy for both sides
    rows = [tr.run_batch() for _ in range(4)]
    for r in rows:
        for k in ("actor_loss", "critic_loss", "entropy_loss", "ac_loss"):
            assert np.isfinite(r[k]), (k, r)
    assert int(tr.learner.dropped_steps[1]) == 0
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    rows_a = [tr.run_batch() for _ in range(2)]
    tr.rollout.synchronize()
    want = ({k: v.detach().cpu() for k, v in tr.rollout.policy.state_dict().items()}, tr.rollout.envs[0].get_records().view(np.uint8).copy(),
            tr.rollout.envs[0].get_rng_range(), tr.rollout.work[0]["counter"].cpu())
    tr2 = _trainer(tmp_path, 1)
    tr2.load_checkpoint(path)
    rows_b = [tr2.run_batch() for _ in range(2)]
    tr2.rollout.synchronize()
    got = ({k: v.detach().cpu() for k, v in tr2.rollout.policy.state_dict().items()}, tr2.rollout.envs[0].get_records().view(np.uint8).copy(),
           tr2.rollout.envs[0].get_rng_range(), tr2.rollout.work[0]["counter"].cpu())
    for k in want[0]:
        assert torch.equal(want[0][k], got[0][k]), k
    assert np.array_equal(want[1], got[1])
    assert np.array_equal(want[2][0], got[2][0]) and np.array_equal(want[2][1], got[2][1])
    assert torch.equal(want[3], got[3])
    for ra, rb in zip(rows_a, rows_b):
        for k in ("actor_loss", "critic_loss", "entropy_loss", "ac_loss"):
            assert ra[k] == rb[k], k
