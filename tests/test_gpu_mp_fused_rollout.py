"""GPU: the one-launch window kernel of wide batches (PolicyRollout(players=P, fused_wide=True), azul_batch_mp_policy_rollout) against the
per-move path (fused_wide=False: PyTorch GEMMs + azul_policy_head_n + azul_batch_mp_agent_step / _policy_step).

Dyadic weights make the comparison bit for bit.  The observations are integers (checked), every layer-1 weight and bias is a multiple of 2^-6,
every layer-2 and critic weight and bias a multiple of 2^-6.  So every product and partial sum of layer 1 is a multiple of 2^-6, the hidden
units are too, and every product and partial sum of layer 2 and of the critic is a multiple of 2^-12.  `_assert_exact` bounds every partial
sum, in any order, by the float64 sum of the absolute terms: below 2^17 for layer 1 (17 + 6 = 23 bits) and below 2^11 for layer 2 and the
critic (11 + 12 = 23 bits), both within the 24-bit f32 significand.  Every sum is then exact in any order, and the two paths must agree in
every bit.  The runs are long enough that episodes end (and the slots restart) inside them in both paths."""
import ctypes as C

import numpy as np
import pytest
import torch

from azul_deep_reinforcement_learning_amd import _lib as L
from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
from azul_deep_reinforcement_learning_amd.rollout import PolicyRollout
from azul_deep_reinforcement_learning_amd.multiplayer import MultiplayerAzul

pytestmark = pytest.mark.gpu

# (players, rules) of the five instantiations: (2, 5) extended, (3, 5), (3, 7), (4, 5), (4, 9)
SHAPES = [
    (2, {"first_player": "Random", "tile_pool": "Lid", "bonuses": "end"}),
    (3, {"first_player": "Random", "tile_pool": "Lid"}),
    (3, {"first_player": "Random", "tile_pool": "Lid", "displays": "2P+1"}),
    (4, {"first_player": "Random", "tile_pool": "Lid"}),
    (4, {"first_player": "Random", "tile_pool": "Random", "displays": "2P+1", "short_deal": True}),
]
SHAPE_IDS = ["p2_d5x", "p3_d5", "p3_d7", "p4_d5", "p4_d9"]


def _dims(players, rules):
    d = 2 * players + 1 if rules.get("displays", 5) == "2P+1" else 5
    return 5 * d + 6 + 52 * players + 1, (d + 1) * 30


def _dyadic_policy(players, rules, seed):
    n_obs, n_act = _dims(players, rules)
    g = torch.Generator().manual_seed(seed)
    net = BatchedActorCritic(n_obs, n_act, 180)

    def dy(shape, step, keep=0.5):
        v = torch.randint(-16, 17, shape, generator=g).float() * step          # |v| <= 16 step
        return torch.where(torch.rand(shape, generator=g) < keep, v, torch.zeros_like(v))

    with torch.no_grad():
        net.critic_linear1.weight.copy_(dy((180, n_obs), 2.0 ** -6, 0.3))         # layer 1: multiples of 2^-6, |w| <= 1/4
        net.actor_linear1.weight.copy_(dy((180, n_obs), 2.0 ** -6, 0.3))
        net.critic_linear1.bias.copy_(dy((180,), 2.0 ** -6, 1.0))
        net.actor_linear1.bias.copy_(dy((180,), 2.0 ** -6, 1.0))
        net.critic_linear2.weight.copy_(dy((1, 180), 2.0 ** -6 / 4, 1.0))          # layer 2 / critic: multiples of 2^-6 (here 2^-8 steps)
        net.critic_linear2.bias.copy_(dy((1,), 2.0 ** -6, 1.0))
        net.actor_linear2.weight.copy_(dy((n_act, 180), 2.0 ** -6 / 4, 0.5))
        net.actor_linear2.bias.copy_(dy((n_act,), 2.0 ** -6, 1.0))
    return net


def _assert_exact(net, obs):
    """The premises of the module docstring on the recorded observations: integers; the weights on their grids; every partial sum of
    layer 1 below 2^17 and of layer 2 / the critic below 2^11 in magnitude (float64 sums of the absolute terms, biases included)."""
    sd = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    o = obs.reshape(-1, obs.shape[-1]).double().cpu()
    assert torch.equal(o, o.round())
    for k, v in sd.items():
        step = 2.0 ** -8 if k in ("critic_linear2.weight", "actor_linear2.weight") else 2.0 ** -6
        assert torch.equal(v / step, (v / step).round()), k
    w1 = torch.cat([sd["critic_linear1.weight"], sd["actor_linear1.weight"]]).abs()
    b1 = torch.cat([sd["critic_linear1.bias"], sd["actor_linear1.bias"]]).abs()
    h = o.abs() @ w1.t() + b1
    assert float(h.max()) < 2.0 ** 17
    hc, ha = h[:, :180], h[:, 180:]
    assert float((hc @ sd["critic_linear2.weight"].abs().t()).max() + sd["critic_linear2.bias"].abs().max()) < 2.0 ** 11
    assert float((ha @ sd["actor_linear2.weight"].abs().t() + sd["actor_linear2.bias"].abs()).max()) < 2.0 ** 11


def _state(ro):
    out = {"episodes": [], "stuck": [], "stat": [], "rec": [], "mt": [], "pos": []}
    for e in ro.envs:
        c = e.counters()
        out["episodes"].append(np.asarray(c["episodes"]).copy())
        out["stuck"].append(np.asarray(c["stuck"]).copy())
        out["stat"].append(np.asarray(c["stat_sums"]).copy())
        out["rec"].append(np.asarray(e.get_records()).copy())
        mt, pos = e.get_rng_range()
        out["mt"].append(np.asarray(mt).copy())
        out["pos"].append(np.asarray(pos).copy())
    return out


def _traj(ro):
    return [{k: v.detach().cpu().clone() for k, v in tr.items()} for tr in ro.traj]


def _run(players, rules, policy, fused, n_games, windows, opponent, selection, parts=1, window=8):
    ro = PolicyRollout(policy, n_games=n_games, parts=parts, rules=rules, seed_base=11, window=window, opponent=opponent, players=players,
                       action_selection=selection, fused_wide=fused, sample_seed=0x1234, use_graph=False)   # (a graph's warm-up plays a window)
    trajs = []
    for _ in range(windows):
        ro.run_window(gamma=0.99)
        ro.synchronize()
        trajs.append(_traj(ro))
    torch.cuda.synchronize()
    counter = [int(w["counter"][0]) for w in ro.work]
    return ro, trajs, _state(ro), counter


def _eq(a, b, what):
    if torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        if a.is_floating_point():
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what
        else:
            assert torch.equal(a, b), what
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), what


@pytest.mark.parametrize("selection", ["Distribution", "Max"])
@pytest.mark.parametrize("opponent", [None, "random"])
@pytest.mark.parametrize("shape", range(5), ids=SHAPE_IDS)
def test_fused_wide_equals_gemm_path_bit_for_bit(shape, opponent, selection):
    players, rules = SHAPES[shape]
    policy = _dyadic_policy(players, rules, 100 + shape).cuda()
    n, W, T = (37 if shape % 2 else 100), 4, 32                          # ragged last workgroups; 128 moves / agent steps per game
    ro_a, ta, sa, ca = _run(players, rules, policy, False, n, W, opponent, selection, window=T)
    ro_b, tb, sb, cb = _run(players, rules, policy, True, n, W, opponent, selection, window=T)
    for w in range(W):
        _assert_exact(policy, ta[w][0]["obs"])
        for k in ta[w][0]:
            _eq(ta[w][0][k], tb[w][0][k], "window %d: %s" % (w, k))
    for k in sa:
        for x, y in zip(sa[k], sb[k]):
            _eq(x, y, k)
    assert ca == cb == [W * T]
    _eq(ro_a.work[0]["status"].cpu(), ro_b.work[0]["status"].cpu(), "status")
    # episodes ended inside the runs, in both paths: the done flags, restarts, statistics and counters compared above are not all zeros
    for tr, st in ((ta, sa), (tb, sb)):
        assert sum(int((t[0]["done"] == 1).sum()) for t in tr) > 0
        assert int(st["episodes"][0].sum()) > 0 and float(np.abs(st["stat"][0]).sum()) > 0


def test_fused_wide_general_weights_sharding_forward_draws_and_model_replay():
    """Random weights: parts = 2 equal parts = 1 bit for bit; value within 1e-4 of a torch f32 forward on the recorded observations;
    action, log-prob and entropy against tests/policy_draw_ref.py on the torch logits (rows near a CDF boundary excused); every recorded
    step replayed through tests/mp_runner_model.py (the oracle's P-seat GameRunner) gives the recorded observations, masks, players,
    rewards and done flags, then the same records, MT19937 streams and counters."""
    from oracle import oracle as oz
    from tests import policy_draw_ref as pdr
    from tests.mp_runner_model import MPRunner
    players, rules = 3, SHAPES[2][1]
    torch.manual_seed(5)
    n_obs, n_act = _dims(players, rules)
    n, W, T = 64, 2, 32
    policy = BatchedActorCritic(n_obs, n_act, 180).cuda()
    ro1, t1, s1, _ = _run(players, rules, policy, True, n, W, "random", "Distribution", parts=1, window=T)
    ro2, t2, s2, _ = _run(players, rules, policy, True, n, W, "random", "Distribution", parts=2, window=T)
    for w in range(W):
        for k in t1[w][0]:
            both = torch.cat([t2[w][0][k], t2[w][1][k]], dim=1)
            _eq(t1[w][0][k], both, "sharding: %s" % k)
    for k in ("rec", "mt", "pos", "episodes", "stuck", "stat"):
        _eq(np.concatenate(s1[k]), np.concatenate(s2[k]), "sharding: %s" % k)
    models = [MPRunner(players, oz.FIRST_RANDOM, oz.POOL_LID, oz.EXT_DISPLAYS_2P1, seed=11 + g) for g in range(n)]
    for m in models:                                   # GameRunner() + reset(), as PolicyRollout opens the RandomAgent setup
        m.runner_init()
        m.reset()
    dones = 0
    for w in range(W):
        tr = t1[w][0]
        with torch.no_grad():
            obs = tr["obs"][:T].cuda().reshape(-1, n_obs)
            value = policy.forward_critic(obs).reshape(T, n)
            logits = policy.actor_linear2(torch.relu(policy.actor_linear1(obs))).reshape(T, n, n_act).cpu().numpy()
        assert torch.allclose(tr["value"].cuda().reshape(T, n), value, atol=1e-4, rtol=1e-5)
        for t in range(T):
            ref = pdr.head(logits[t], tr["mask"][t].numpy(), 0x1234, w * T + t, id_base=11)
            pdr.compare(ref, tr["action"][t].numpy(), tr["log_prob"][t].numpy(), tr["entropy"][t].numpy(), extra_lp=1e-4, extra_draw=1e-4,
                        extra_ent=1e-4)
        for g, m in enumerate(models):
            for t in range(T):
                assert np.array_equal(tr["obs"][t, g].numpy(), m.obs(0).astype(np.float32)), (w, t, g)
                assert np.array_equal(tr["mask"][t, g].numpy(), m.mask()) and int(tr["player"][t, g]) == m.g.current_player, (w, t, g)
                st, rew, dn = m.agent_step(int(tr["action"][t, g]))
                assert (int(tr["reward"][t, g]), int(tr["done"][t, g])) == (rew, dn), (w, t, g)
                dones += int(dn == 1)
    assert dones > 0
    recs = s1["rec"][0].view(np.uint8).reshape(n, -1)
    for g, m in enumerate(models):
        assert np.array_equal(recs[g], m.record()), g
        mt, pos = m.rng_state()
        assert int(s1["pos"][0][g]) == pos and np.array_equal(s1["mt"][0][g], mt), g
        assert (int(s1["episodes"][0][g]), int(s1["stuck"][0][g])) == (m.episodes, m.stuck), g
        assert np.array_equal(s1["stat"][0][g], m.stat_sum), g


def test_fused_wide_refusals():
    players, rules = 3, SHAPES[1][1]
    n_obs, n_act = _dims(players, rules)
    pol = BatchedActorCritic(n_obs, n_act, 180).cuda()
    with pytest.raises(ValueError):
        PolicyRollout(pol, n_games=16, rules=rules, players=players, opponent=BatchedActorCritic(n_obs, n_act, 180).cuda(), fused_wide=True)
    with pytest.raises(ValueError):
        PolicyRollout(BatchedActorCritic(n_obs, n_act, 64).cuda(), n_games=16, rules=rules, players=players, fused_wide=True)
    with pytest.raises(ValueError):
        PolicyRollout(BatchedActorCritic().cuda(), n_games=16, players=2, fused_wide=True)
    with pytest.raises(ValueError):
        PolicyRollout(pol, n_games=16, rules=rules, players=players, fused_head=False, fused_wide=True)
    # the C entry: mismatched sizes, hidden size, and a two-player reference batch
    env = MultiplayerAzul(16, rules=rules, players=players)
    T, d = 2, torch.device("cuda")
    bufs = {"obs": torch.zeros(T + 1, 16, n_obs, device=d), "mask": torch.zeros(T + 1, 16, n_act, dtype=torch.uint8, device=d),
            "player": torch.zeros(T + 1, 16, dtype=torch.uint8, device=d), "action": torch.zeros(T, 16, dtype=torch.int32, device=d),
            "reward": torch.zeros(T, 16, dtype=torch.int32, device=d), "done": torch.zeros(T, 16, dtype=torch.uint8, device=d),
            "value": torch.zeros(T, 16, device=d), "logp": torch.zeros(T, 16, device=d), "entropy": torch.zeros(T, 16, device=d)}
    p = lambda x: C.c_void_p(x.data_ptr())
    w1t = torch.zeros(n_obs, 360, device=d)
    z = torch.zeros(360 * 400, device=d)
    wa = L.NetWeights(p(w1t), p(z), p(z), p(z), p(z), p(z))
    out = L.RolloutBuffers(*[p(bufs[k]) for k in ("obs", "mask", "player", "action", "reward", "done", "value", "logp", "entropy")],
                           None, None, None, None, None, 0)
    call = lambda h, ni, hid, na: L.lib.azul_batch_mp_policy_rollout(h, T, 0, C.byref(wa), ni, hid, na, 1, 0, None, C.byref(out), C.c_float(0.9), None)
    assert call(env._h, n_obs + 1, 180, n_act) == L.ERR_INVALID
    assert call(env._h, n_obs, 180, n_act + 60) == L.ERR_INVALID
    assert call(env._h, n_obs, 128, n_act) == L.ERR_INVALID
    from azul_deep_reinforcement_learning_amd.batch import BatchedAzul
    two = BatchedAzul(16)
    assert call(two._h, 136, 180, 180) == L.ERR_INVALID
    assert call(env._h, n_obs, 180, n_act) == 0
    torch.cuda.synchronize()


def _trainer(tmp_path, seed):
    from azul_deep_reinforcement_learning_amd.training import BatchedTrainer
    players, rules = 3, SHAPES[1][1]
    n_obs, n_act = _dims(players, rules)
    torch.manual_seed(seed)
    return BatchedTrainer(BatchedActorCritic(n_obs, n_act, 180), n_games=256, window=16, players=players, rules=rules, device="cuda:0",
                          fused_wide=True, results_dir=str(tmp_path))


def test_fused_wide_trainer_trains_and_resumes_exactly(tmp_path):
    tr = _trainer(tmp_path, 0)
    assert tr.rollout.fused_wide and tr.rollout.ring == 1
    rows = [tr.run_batch() for _ in range(4)]
    for r in rows:
        for k in ("actor_loss", "critic_loss", "entropy_loss", "ac_loss"):
            assert np.isfinite(r[k]), (k, r)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    for _ in range(2):
        tr.run_batch()
    tr.rollout.synchronize()
    want = ({k: v.detach().cpu() for k, v in tr.rollout.policy.state_dict().items()}, tr.rollout.envs[0].get_records().view(np.uint8).copy(),
            tr.rollout.envs[0].get_rng_range())
    tr2 = _trainer(tmp_path, 1)
    tr2.load_checkpoint(path)
    for _ in range(2):
        tr2.run_batch()
    tr2.rollout.synchronize()
    got = ({k: v.detach().cpu() for k, v in tr2.rollout.policy.state_dict().items()}, tr2.rollout.envs[0].get_records().view(np.uint8).copy(),
           tr2.rollout.envs[0].get_rng_range())
    for k in want[0]:
        assert torch.equal(want[0][k], got[0][k]), k
    assert np.array_equal(want[1], got[1])
    assert np.array_equal(want[2][0], got[2][0]) and np.array_equal(want[2][1], got[2][1])
