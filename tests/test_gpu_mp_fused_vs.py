"""GPU: the wide window kernel with a NETWORK opponent (PolicyRollout(players=P, opponent=<net>, fused_wide=True, fused_opponent=True),
azul_batch_mp_policy_rollout_vs) against the per-cut path (fused_opponent=False: azul_batch_mp_net_* cuts, PyTorch GEMMs +
azul_policy_head_n per reply round).

Dyadic weights for the agent AND the opponent make the comparison bit for bit (tests/test_gpu_mp_fused_rollout.py's argument: every product
and partial sum of both layers is exact in any order).  The runs are long enough that episodes end inside agent steps, so that the next
episode's openings are played inside reply rounds.  The opponent trace of the per-cut path also holds answers for games that did not owe in
a round (its forward runs over the whole batch); the kernel writes only the rounds a game owed, so the trace is compared there."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from azul_deep_reinforcement_learning_amd import _lib as L
from azul_deep_reinforcement_learning_amd.multiplayer import MultiplayerAzul
from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
from azul_deep_reinforcement_learning_amd.rollout import PolicyRollout
from tests.test_gpu_mp_fused_rollout import SHAPE_IDS, SHAPES, _assert_exact, _dims, _dyadic_policy, _eq, _state, _traj

pytestmark = pytest.mark.gpu

ST_BAD_ACTION = 4
R = 6                          # opponent trace slots


def _run(players, rules, policy, opponent, fused, n_games, windows, selection, parts=1, window=16):
    ro = PolicyRollout(policy, n_games=n_games, parts=parts, rules=rules, seed_base=11, window=window, opponent=opponent, players=players,
                       action_selection=selection, opponent_selection=selection, opponent_trace=R, fused_wide=fused, fused_opponent=fused,
                       sample_seed=0x1234, use_graph=False)
    trajs = []
    for _ in range(windows):
        ro.run_window(gamma=0.99)
        ro.synchronize()
        trajs.append(_traj(ro))
    torch.cuda.synchronize()
    counter = [int(w["counter"][0]) for w in ro.work]
    return ro, trajs, _state(ro), counter


def _owed(tr):
    """[T][R][N] bool: round j of step t was played for game g (legal answers: one opponent move per round)."""
    j = torch.arange(R).view(1, R, 1)
    return j < tr["opp_replies"].long().unsqueeze(1)


@pytest.mark.parametrize("selection", ["Distribution", "Max"])
@pytest.mark.parametrize("shape", range(5), ids=SHAPE_IDS)
def test_fused_opponent_equals_per_cut_path_bit_for_bit(shape, selection):
    players, rules = SHAPES[shape]
    policy = _dyadic_policy(players, rules, 200 + shape).cuda()
    opponent = _dyadic_policy(players, rules, 300 + shape).cuda()
    n, W, T = (37 if shape % 2 else 100), 4, 16                          # ragged last workgroups; 64 agent steps per game
    ro_a, ta, sa, ca = _run(players, rules, policy, opponent, False, n, W, selection, window=T)
    ro_b, tb, sb, cb = _run(players, rules, policy, opponent, True, n, W, selection, window=T)
    assert ro_b.fused_opponent and not ro_a.fused_opponent
    traced = 0
    for w in range(W):
        _assert_exact(policy, ta[w][0]["obs"])
        _assert_exact(opponent, ta[w][0]["obs"])
        for k in ta[w][0]:
            if k in ("opp_action", "opp_logp"):
                continue
            _eq(ta[w][0][k], tb[w][0][k], "window %d: %s" % (w, k))
        owed = _owed(ta[w][0])
        traced += int(owed.sum())
        for k in ("opp_action", "opp_logp"):
            _eq(ta[w][0][k][owed], tb[w][0][k][owed], "window %d: %s" % (w, k))
    assert traced > n * W * T                          # most steps had replies
    for k in sa:
        for x, y in zip(sa[k], sb[k]):
            _eq(x, y, k)
    assert ca == cb == [W * T]
    _eq(ro_a.work[0]["status"].cpu(), ro_b.work[0]["status"].cpu(), "status")
    for tr, st in ((ta, sa), (tb, sb)):
        assert sum(int((t[0]["done"] == 1).sum()) for t in tr) > 0
        assert int(st["episodes"][0].sum()) > 0 and float(np.abs(st["stat"][0]).sum()) > 0
    # episodes ended inside steps that had reply rounds
    assert any(bool(((t[0]["done"] == 1) & (t[0]["opp_replies"] > 0)).any()) for t in tb)


def test_fused_opponent_general_weights_and_sharding():
    """Random weights: parts = 2 equals parts = 1 bit for bit per global game id; against the per-cut path, the agent's value / log-prob
    agree to f32 summation order and the actions, answers and states agree except in games where a draw near a CDF boundary went the
    other way (at most a few games); the agent's draws against tests/policy_draw_ref.py on torch logits of the recorded observations."""
    from tests import policy_draw_ref as pdr
    players, rules = 4, SHAPES[3][1]
    torch.manual_seed(7)
    n_obs, n_act = _dims(players, rules)
    n, W, T = 64, 2, 16
    policy = BatchedActorCritic(n_obs, n_act, 180).cuda()
    opponent = BatchedActorCritic(n_obs, n_act, 180).cuda()
    ro1, t1, s1, c1 = _run(players, rules, policy, opponent, True, n, W, "Distribution", parts=1, window=T)
    ro2, t2, s2, c2 = _run(players, rules, policy, opponent, True, n, W, "Distribution", parts=2, window=T)
    for w in range(W):
        for k in t1[w][0]:
            both = torch.cat([t2[w][0][k], t2[w][1][k]], dim=-1 if k in ("opp_action", "opp_logp") else 1)
            _eq(t1[w][0][k], both, "sharding: %s" % k)
    for k in ("rec", "mt", "pos", "episodes", "stuck", "stat"):
        _eq(np.concatenate(s1[k]), np.concatenate(s2[k]), "sharding: %s" % k)
    assert c1 == [W * T] and c2 == [W * T, W * T]
    ro3, t3, _, _ = _run(players, rules, policy, opponent, False, n, W, "Distribution", parts=1, window=T)
    same = np.ones(n, bool)                            # games whose trajectories have not diverged yet
    for w in range(W):
        a, b = t1[w][0], t3[w][0]
        with torch.no_grad():
            obs = a["obs"][:T].cuda().reshape(-1, n_obs)
            value = policy.forward_critic(obs).reshape(T, n)
            logits = policy.actor_linear2(torch.relu(policy.actor_linear1(obs))).reshape(T, n, n_act).cpu().numpy()
        assert torch.allclose(a["value"].cuda().reshape(T, n), value, atol=1e-4, rtol=1e-5)
        for t in range(T):
            ref = pdr.head(logits[t], a["mask"][t].numpy(), 0x1234, w * T + t, id_base=11)
            pdr.compare(ref, a["action"][t].numpy(), a["log_prob"][t].numpy(), a["entropy"][t].numpy(), extra_lp=1e-4, extra_draw=1e-4,
                        extra_ent=1e-4)
            owed = (torch.arange(R).view(R, 1) < b["opp_replies"][t].long().view(1, n)).numpy()
            for g in np.flatnonzero(same):
                eq = (torch.equal(a["obs"][t, g], b["obs"][t, g]) and int(a["action"][t, g]) == int(b["action"][t, g]) and
                      int(a["opp_replies"][t, g]) == int(b["opp_replies"][t, g]) and
                      np.array_equal(a["opp_action"][t, :, g].numpy()[owed[:, g]], b["opp_action"][t, :, g].numpy()[owed[:, g]]))
                if not eq:
                    same[g] = False
                    continue
                assert abs(float(a["value"][t, g]) - float(b["value"][t, g])) < 1e-4, (w, t, g)
                assert abs(float(a["log_prob"][t, g]) - float(b["log_prob"][t, g])) < 1e-4, (w, t, g)
                lp = np.abs(a["opp_logp"][t, :, g].numpy() - b["opp_logp"][t, :, g].numpy())[owed[:, g]]
                assert (lp < 1e-4).all(), (w, t, g)
    assert int((~same).sum()) <= 2, np.flatnonzero(~same)


def test_fused_opponent_reply_cap_marks_games_and_the_next_window_runs():
    """An opponent whose forward is NaN answers -1, which the env refuses (AZUL_BAD_ACTION): every reply round of a step fails, and after
    MAX_REPLY_ROUNDS rounds the step ends (pending cleared, status = the step's first status, legal mask of the state).  The window ends,
    the next one runs, and with a finite opponent installed again the games play on."""
    players, rules = 3, SHAPES[1][1]
    policy = _dyadic_policy(players, rules, 400).cuda()
    opponent = _dyadic_policy(players, rules, 401).cuda()
    n, T, cap = 40, 8, 3
    ro = PolicyRollout(policy, n_games=n, rules=rules, seed_base=5, window=T, opponent=opponent, players=players, opponent_trace=cap + 2,
                       fused_wide=True, fused_opponent=True, use_graph=False)
    ro.MAX_REPLY_ROUNDS = cap
    bad = copy.deepcopy(opponent)
    with torch.no_grad():
        bad.actor_linear2.bias.fill_(float("nan"))
    ro.set_opponent(bad)
    for _ in range(2):
        tr = ro.traj[0]
        tr["opp_action"].fill_(-99)
        ro.run_window()
        ro.synchronize()
        oa, rep = tr["opp_action"].cpu(), tr["opp_replies"].cpu()
        played = oa != -99                                  # [T][slots][N]: the rounds that ran
        assert bool(played.any())
        assert bool((oa[played] == -1).all())               # a forward that is not finite answers -1
        rounds = played.sum(dim=1)                          # [T][N]
        assert bool(((rounds == 0) | (rounds == cap)).all())     # every round failed: a step with replies ran up to the cap ...
        assert bool((oa[:, cap:] == -99).all())             # ... and no further
        assert bool((rep[rounds == cap] == 0).all())
        st = ro.work[0]["status"].cpu()
        assert bool((st == ST_BAD_ACTION).any())
    ro.set_opponent(opponent)                               # the weights are read at the next launch
    ro.run_window()
    ro.synchronize()
    assert int(ro.traj[0]["opp_replies"].sum()) > 0


def test_fused_opponent_refusals():
    players, rules = 3, SHAPES[1][1]
    n_obs, n_act = _dims(players, rules)
    pol = BatchedActorCritic(n_obs, n_act, 180).cuda()
    opp = BatchedActorCritic(n_obs, n_act, 180).cuda()
    with pytest.raises(ValueError, match="per-cut"):
        PolicyRollout(pol, n_games=16, rules=rules, players=players, opponent=BatchedActorCritic(n_obs, n_act, 64).cuda(), fused_wide=True,
                      fused_opponent=True)
    with pytest.raises(ValueError):
        PolicyRollout(pol, n_games=16, rules=rules, players=players, opponent=opp, fused_opponent=True)
    for o in (None, "random"):
        with pytest.raises(ValueError):
            PolicyRollout(pol, n_games=16, rules=rules, players=players, opponent=o, fused_wide=True, fused_opponent=True)
    ro = PolicyRollout(pol, n_games=16, rules=rules, players=players, opponent=BatchedActorCritic(n_obs, n_act, 64).cuda(), window=2)
    ro.run_window()                                         # the per-cut path keeps any hidden size
    ro.synchronize()
    # the C entry
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

    def call(h, ni, hid, na, wo=C.byref(wa), reps=8):
        return L.lib.azul_batch_mp_policy_rollout_vs(h, T, C.byref(wa), wo, ni, hid, na, 1, 2, 0, None, reps, C.byref(out), C.c_float(0.9), None)

    assert call(env._h, n_obs + 1, 180, n_act) == L.ERR_INVALID
    assert call(env._h, n_obs, 180, n_act + 60) == L.ERR_INVALID
    assert call(env._h, n_obs, 128, n_act) == L.ERR_INVALID
    assert call(env._h, n_obs, 180, n_act, wo=None) == L.ERR_INVALID
    assert call(env._h, n_obs, 180, n_act, reps=0) == L.ERR_INVALID
    from azul_deep_reinforcement_learning_amd.batch import BatchedAzul
    two = BatchedAzul(16)
    assert call(two._h, 136, 180, 180) == L.ERR_INVALID
    env.runner_init()
    assert call(env._h, n_obs, 180, n_act) == 0
    torch.cuda.synchronize()


def _trainer(tmp_path, seed):
    from azul_deep_reinforcement_learning_amd.training import BatchedTrainer
    players, rules = 3, SHAPES[1][1]
    n_obs, n_act = _dims(players, rules)
    torch.manual_seed(seed)
    # (window 24: every update sees episodes that ended inside its window, from the first one on)
    return BatchedTrainer(BatchedActorCritic(n_obs, n_act, 180), n_games=256, window=24, players=players, rules=rules, device="cuda:0",
                          fused_wide=True, fused_opponent=True, opponent="self", opponent_refresh=2, results_dir=str(tmp_path))


def test_fused_opponent_trainer_trains_and_resumes_exactly(tmp_path):
    tr = _trainer(tmp_path, 0)
    assert tr.rollout.fused_wide and tr.rollout.fused_opponent and tr.rollout.opponent == "net"
    rows = [tr.run_batch() for _ in range(4)]
    for r in rows:
        for k in ("actor_loss", "critic_loss", "entropy_loss", "ac_loss"):
            assert np.isfinite(r[k]), (k, r)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    for _ in range(3):                                      # (an opponent refresh inside)
        tr.run_batch()
    tr.rollout.synchronize()
    want = ({k: v.detach().cpu() for k, v in tr.rollout.policy.state_dict().items()}, tr.rollout.envs[0].get_records().view(np.uint8).copy(),
            tr.rollout.envs[0].get_rng_range(), tr.rollout.ow1t.detach().cpu())
    tr2 = _trainer(tmp_path, 1)
    tr2.load_checkpoint(path)
    for _ in range(3):
        tr2.run_batch()
    tr2.rollout.synchronize()
    got = ({k: v.detach().cpu() for k, v in tr2.rollout.policy.state_dict().items()}, tr2.rollout.envs[0].get_records().view(np.uint8).copy(),
           tr2.rollout.envs[0].get_rng_range(), tr2.rollout.ow1t.detach().cpu())
    for k in want[0]:
        assert torch.equal(want[0][k], got[0][k]), k
    assert np.array_equal(want[1], got[1])
    assert np.array_equal(want[2][0], got[2][0]) and np.array_equal(want[2][1], got[2][1])
    assert torch.equal(want[3], got[3])
