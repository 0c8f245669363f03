"""PolicyRollout(players=P, opponent="greedy_margin", fused_wide=True, fused_seats=True) on the GPU: the greedy_margin seats of wide batches
answer inside the window kernel (azul_batch_mp_policy_rollout_greedy, azul_x_policy_rollout_kernel<P, D, 3>).  The reference is the per-cut
path of the same rollout (one azul_batch_mp_score_moves launch per reply round), bit for bit: the agent's weights are dyadic
(test_gpu_mp_fused_rollout._dyadic_policy), so the kernel's matrix sums and the per-cut path's GEMMs are the same bits.  And the host model
(tests/mp_net_model.MPNetRunner answered by tests/mp_score_moves_model.greedy_of_game) for two shapes, from the seeds."""
import ctypes as C

import numpy as np
import pytest
import torch

from azul_deep_reinforcement_learning_amd import _lib as L
from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
from azul_deep_reinforcement_learning_amd.rollout import PolicyRollout
from tests import mp_score_moves_model as mm
from tests import training_ring_cases as rc
from tests.test_gpu_mp_fused_rollout import SHAPES, SHAPE_IDS, _assert_exact, _dims, _dyadic_policy, _eq, _state
from tests.test_gpu_mp_score_moves import rules_of

pytestmark = pytest.mark.gpu

TRACE = 6
PLAIN = ("obs", "mask", "player", "action", "reward", "done", "value", "log_prob", "entropy", "returns", "opp_replies")


def _rollout(players, rules, policy, fused, n, T, selection="Distribution", parts=1, trace=TRACE, wide_ring=1, seed_base=11):
    return PolicyRollout(policy, n_games=n, parts=parts, rules=rules, seed_base=seed_base, window=T, opponent="greedy_margin", players=players,
                         action_selection=selection, fused_wide=fused, fused_seats=fused, sample_seed=0x1234, use_graph=False,
                         opponent_trace=trace, wide_ring=wide_ring)


def _play(ro, windows, gamma=0.99):
    wins = []
    for _ in range(windows):
        ro.run_window(gamma)
        ro.synchronize()
        wins.append([{k: v.detach().cpu().clone() for k, v in tr.items()} for tr in ro.traj])
    torch.cuda.synchronize()
    return wins, _state(ro), [int(w["counter"][0]) for w in ro.work], [w["status"].cpu().clone() for w in ro.work]


def _same_window(a, b, what, trace=TRACE):
    for k in PLAIN:
        _eq(a[k], b[k], "%s: %s" % (what, k))
    # the traced answers of the rounds a game owed: reply j of a step that had more than j replies (the per-cut path copies every game's
    # answer buffer into the slot, the kernel writes the games that owed)
    owed = torch.arange(trace).view(1, trace, 1) < a["opp_replies"].long().unsqueeze(1)
    assert torch.equal(a["opp_action"][owed], b["opp_action"][owed]), "%s: opp_action" % what
    assert bool((b["opp_action"][owed] >= 0).all()), what
    assert bool((a["opp_logp"] == 0).all()) and bool((b["opp_logp"] == 0).all()), what


def _same_run(ra, rb, what):
    (wa, sa, ca, sta), (wb, sb, cb, stb) = ra, rb
    assert len(wa) == len(wb)
    for w, (x, y) in enumerate(zip(wa, wb)):
        for p, (xp, yp) in enumerate(zip(x, y)):
            _same_window(xp, yp, "%s window %d part %d" % (what, w, p))
    for k in sa:
        for x, y in zip(sa[k], sb[k]):
            _eq(x, y, "%s: %s" % (what, k))
    assert ca == cb, what
    for x, y in zip(sta, stb):
        _eq(x, y, "%s: status" % what)


@pytest.mark.parametrize("shape,selection", [(i, "Distribution") for i in range(5)] + [(4, "Max")], ids=SHAPE_IDS + ["p4_d9_max"])
def test_fused_seats_equal_the_per_cut_path_bit_for_bit(shape, selection):
    players, rules = SHAPES[shape]
    policy = _dyadic_policy(players, rules, 300 + shape).cuda()
    n, W, T = (37 if shape % 2 else 100), 4, 16
    cut = _play(_rollout(players, rules, policy, False, n, T, selection), W)
    ro = _rollout(players, rules, policy, True, n, T, selection)
    assert ro.fused_seats and ro.fused_wide and not ro.use_graph and ro.cut and ro.scripted and not hasattr(ro, "ow1t")
    fused = _play(ro, W)
    for w in range(W):
        _assert_exact(policy, cut[0][w][0]["obs"])
    _same_run(cut, fused, SHAPE_IDS[shape])
    assert cut[2] == [W * T]
    for run in (cut, fused):
        ended = sum(int(((win[0]["done"] == 1) & (win[0]["opp_replies"] > 0)).sum()) for win in run[0])
        assert ended > 0                                    # episodes ended inside steps that had replies
        assert int(run[1]["episodes"][0].sum()) > 0 and float(np.abs(run[1]["stat"][0]).sum()) > 0
        assert sum(int(win[0]["opp_replies"].sum()) for win in run[0]) >= W * T * n


@pytest.mark.parametrize("n", [1, 17])
def test_small_batches(n):
    """n = 1: one live half in the only wave; n = 17: a second workgroup with one game."""
    players, rules = SHAPES[2]
    policy = _dyadic_policy(players, rules, 77).cuda()
    cut = _play(_rollout(players, rules, policy, False, n, 4), 3)
    fused = _play(_rollout(players, rules, policy, True, n, 4), 3)
    _same_run(cut, fused, "n=%d" % n)
    assert sum(int(win[0]["opp_replies"].sum()) for win in fused[0]) > 0


@pytest.mark.parametrize("i", [2, 4], ids=[mm.shape_id(mm.SHAPES[2]), mm.shape_id(mm.SHAPES[4])])
def test_fused_seats_rollout_replays_through_the_model(i):
    """test_gpu_mp_score_moves.test_greedy_margin_rollout_replays_through_the_model with fused_seats=True: every game of two windows
    replayed through MPNetRunner.reset_with / step_with from its seed, answered by the model's greedy choice on the runner's own game."""
    from azul_deep_reinforcement_learning_amd.batch import batch_shape
    from tests.mp_net_model import MPNetRunner
    shape = mm.SHAPES[i]
    P, ext, pool, first = shape
    rules = rules_of(shape)
    n_obs, n_act = batch_shape(P, rules)
    torch.manual_seed(3 + i)
    T, n, R = 8, 6, 48
    ro = PolicyRollout(BatchedActorCritic(n_obs, n_act, 180), players=P, n_games=n, window=T, opponent="greedy_margin", opponent_trace=R,
                       rules=rules, seed_base=900, fused_wide=True, fused_seats=True)
    assert ro.opponent == "greedy_margin" and ro.cut and ro.fused_wide and ro.fused_seats and not ro.use_graph and ro.ring == 1
    assert not hasattr(ro, "ow1t")                                          # no opponent weights are staged
    env = ro.envs[0]
    start = env.get_records().view(np.uint8).reshape(n, 256)
    mt0, pos0 = env.get_rng_range()
    wins = []
    for _ in range(2):
        tr = ro.run_window()
        ro.synchronize()
        wins.append({k: v.cpu().numpy().copy() for k, v in tr[0].items()})
    finals, (fmt, fpos) = env.get_records().view(np.uint8).reshape(n, 256), env.get_rng_range()
    assert (np.concatenate([w["opp_logp"] for w in wins]) == 0).all()
    replies = 0
    for g in range(n):
        m = MPNetRunner(P, first, pool, ext, seed=900 + g)
        trace = {"want": None, "j": 0}

        def answer(obs, mask, player, m=m, trace=trace):
            a = mm.greedy_of_game(m.g, P)
            assert a >= 0 and mask[a], ("greedy answer not legal", g, a)
            if trace["want"] is not None:
                assert trace["j"] < R and a == int(trace["want"][trace["j"]]), ("traced opp_action", g, trace["j"], a)
            trace["j"] += 1
            return a

        assert m.runner_init() == 0 and m.reset_with(answer) == 0
        assert np.array_equal(m.record(), start[g]), g
        assert np.array_equal(m.rng_state()[0], mt0[g]) and m.rng_state()[1] == int(pos0[g]), g
        for w, win in enumerate(wins):
            for t in range(T):
                assert np.array_equal(win["obs"][t, g], m.obs(0).astype(np.float32)), (g, w, t)
                assert np.array_equal(win["mask"][t, g].astype(bool), m.mask()), (g, w, t)
                assert int(win["player"][t, g]) == int(m.g.current_player), (g, w, t)
                trace["want"], trace["j"] = win["opp_action"][t, :, g], 0
                st, rew, dn, rep = m.step_with(int(win["action"][t, g]), answer)
                assert (st, rew, dn, rep) == (0, int(win["reward"][t, g]), int(win["done"][t, g]), int(win["opp_replies"][t, g])), (g, w, t)
                replies += trace["j"]
            assert np.array_equal(win["obs"][T, g], m.obs(0).astype(np.float32)) and np.array_equal(win["mask"][T, g].astype(bool), m.mask())
        assert np.array_equal(m.record(), finals[g]), g
        assert np.array_equal(m.rng_state()[0], fmt[g]) and m.rng_state()[1] == int(fpos[g]), g
    assert replies >= 2 * T * n                              # the opponents really moved: at least one reply per agent step on average


def test_sharding():
    players, rules = SHAPES[1]
    policy = _dyadic_policy(players, rules, 5).cuda()
    runs = []
    for parts in (1, 2):
        ro = _rollout(players, rules, policy, True, 18, 8, parts=parts, seed_base=500)
        wins = []
        for _ in range(3):
            tr = ro.run_window()
            ro.synchronize()
            wins.append({k: np.concatenate([p[k].cpu().numpy() for p in tr], axis=2 if k in ("opp_action", "opp_logp") else 1) for k in tr[0]})
        runs.append((wins, ro.counters()))
    for wa, wb in zip(*[r[0] for r in runs]):
        for key in PLAIN + ("opp_action", "opp_logp"):
            assert wa[key].tobytes() == wb[key].tobytes(), key
    assert runs[0][1] == runs[1][1] and runs[0][1]["episodes"] >= 0


def test_ring_returns_chain_through_the_windows():
    players, rules = SHAPES[3]
    policy = _dyadic_policy(players, rules, 9).cuda()
    T, n, gamma = 8, 17, 0.99
    ro = _rollout(players, rules, policy, True, n, T, wide_ring=2, seed_base=900)
    assert ro.fused_seats and ro.ring == 2
    one = _rollout(players, rules, policy, True, n, T, seed_base=900)
    R = 2 * T
    want = np.zeros((R, n), np.float32)
    reward, done = [], []
    for w in range(5):                                      # the ring wraps twice
        ro.run_window(gamma)
        tr1 = one.run_window(gamma)
        ro.synchronize()
        one.synchronize()
        rg = ro.rings[0]
        rr, dd = rg["reward"].cpu().numpy(), rg["done"].cpu().numpy()
        played = (w + 1) * T
        want = rc.returns_ring(rr, dd, want, gamma, R, played, min(R, played))
        rc.compare_returns("window %d" % w, rg["returns"].cpu().numpy(), want)
        lo = (w % 2) * T                                    # the ring holds the windows the plain rollout plays
        for k in ("reward", "done", "action", "opp_replies", "value", "log_prob"):
            assert np.array_equal(rg[k].cpu().numpy()[lo:lo + T], tr1[0][k].cpu().numpy()), (w, k)
        reward.append(rr[lo:lo + T].copy())
        done.append(dd[lo:lo + T].copy())
        if w >= 1:                                          # q = r + gamma * q over the two newest windows, concatenated, within episodes
            two, _ = rc.returns_window(np.concatenate(reward[-2:]), np.concatenate(done[-2:]), gamma, None)
            got = np.concatenate([rg["returns"].cpu().numpy()[((w - 1) % 2) * T:][:T], rg["returns"].cpu().numpy()[lo:lo + T]])
            rc.compare_returns("two windows %d" % w, got, two)
    assert (np.concatenate(done) != 0).any()
    _eq(ro.envs[0].get_records(), one.envs[0].get_records(), "records")


def test_reply_cap_ends_the_step_stuck_and_the_window_goes_on():
    """Two fused rollouts from the same seeds, windows of one step: the first plays uncapped throughout and finds the first step in which
    some games had at most one reply and some had more; the second plays the same steps and meets that one with MAX_REPLY_ROUNDS = 1."""
    players, rules = SHAPES[2]
    policy = _dyadic_policy(players, rules, 21).cuda()
    n, R = 100, 8

    def snapshot(ro):
        tr = {k: v.cpu().numpy().copy() for k, v in ro.traj[0].items()}
        return (ro, tr, ro.work[0]["status"].cpu().numpy().copy(), ro.envs[0].get_records().view(np.uint8).reshape(n, 256).copy(),
                ro.envs[0].get_rng_range(), ro.envs[0].counters())

    roa = _rollout(players, rules, policy, True, n, 1, trace=R, seed_base=77)
    assert roa.MAX_REPLY_ROUNDS == 512
    for step in range(200):
        roa.traj[0]["opp_action"].fill_(-1)                 # (ring 1: every window writes the same trace buffer)
        roa.run_window()
        roa.synchronize()
        rep = roa.traj[0]["opp_replies"][0].cpu().numpy()
        if step >= 3 and (rep <= 1).any() and (rep > 1).any():
            break
    else:
        raise AssertionError("no step with both kinds of games")
    runs = [snapshot(roa)]
    rob = _rollout(players, rules, policy, True, n, 1, trace=R, seed_base=77)
    for _ in range(step):
        rob.run_window()
    rob.synchronize()
    rob.traj[0]["opp_action"].fill_(-1)
    rob.MAX_REPLY_ROUNDS = 1
    rob.run_window()
    rob.synchronize()
    runs.append(snapshot(rob))
    (_, ta, sa, ra, (mta, pa), ca), (rob, tb, sb, rb, (mtb, pb), cb) = runs
    few = ta["opp_replies"][0] <= 1
    assert few.any() and (~few).any()
    for k in ta:                                            # at most one reply: the cap changes nothing
        axis = 2 if k in ("opp_action", "opp_logp") else 1
        assert np.array_equal(np.compress(few, ta[k], axis=axis), np.compress(few, tb[k], axis=axis)), k
    assert np.array_equal(sa[few], sb[few]) and np.array_equal(ra[few], rb[few])
    assert np.array_equal(np.asarray(mta)[few], np.asarray(mtb)[few]) and np.array_equal(np.asarray(pa)[few], np.asarray(pb)[few])
    for k in ("episodes", "stuck", "stat_sums"):
        assert np.array_equal(np.asarray(ca[k])[few], np.asarray(cb[k])[few]), k
    # every other game gave up after its first reply
    more = ~few
    assert (sb[more] == L.STUCK).all()
    assert (tb["opp_replies"][0][more] == 1).all()
    assert np.array_equal(tb["opp_action"][0, 0][more], ta["opp_action"][0, 0][more]) and (tb["opp_action"][0, 1:][:, more] == -1).all()
    env = rob.envs[0]
    obs = torch.zeros(n, env.obs_size, device="cuda")
    mask = torch.zeros(n, env.num_actions, dtype=torch.uint8, device="cuda")
    player = torch.zeros(n, dtype=torch.uint8, device="cuda")
    env.observe_all(0, obs, mask, player)
    torch.cuda.synchronize()
    assert np.array_equal(tb["mask"][1], mask.cpu().numpy()) and np.array_equal(tb["obs"][1], obs.cpu().numpy())     # the state left behind
    assert np.array_equal(tb["player"][1], player.cpu().numpy())
    rob.run_window()                                        # a further window runs
    rob.synchronize()
    torch.cuda.synchronize()
    assert np.isfinite(rob.traj[0]["value"].cpu().numpy()).all() and (rob.traj[0]["action"].cpu().numpy() >= 0).all()


def test_c_entry_refusals_before_any_launch():
    from azul_deep_reinforcement_learning_amd import BatchedAzul
    players, rules = SHAPES[1]
    n_obs, n_act = _dims(players, rules)
    n, T, dev = 4, 2, "cuda"
    ro = _rollout(players, rules, BatchedActorCritic(n_obs, n_act, 180).cuda(), True, n, T, trace=0)
    env = ro.envs[0]
    CANARY = 0x5EED5EED
    wt = [torch.zeros(s, device=dev) for s in ((n_obs, 360), (360,), (180,), (1,), (180, n_act), (n_act,))]
    w = L.NetWeights(*[t.data_ptr() for t in wt])
    i32 = lambda *s: torch.full(s, CANARY, dtype=torch.int32, device=dev)
    u8 = lambda *s: torch.full(s, 0xA5, dtype=torch.uint8, device=dev)
    f32 = lambda *s: torch.full(s, 1234.5, device=dev)
    bufs = [f32(T + 1, n, n_obs + 1), u8(T + 1, n, n_act + 4), u8(T + 1, n), i32(T, n), i32(T, n), u8(T, n), f32(T, n), f32(T, n), f32(T, n), u8(n),
            f32(T, n), i32(T, 2, n), f32(T, 2, n), u8(T, n)]
    ptrs = [t.data_ptr() for t in bufs]
    out = L.RolloutBuffers(*ptrs, 2)
    ctr = torch.zeros(2, dtype=torch.int64, device=dev)
    two = BatchedAzul(n, device=dev, seed=1)
    two.runner_init()
    before = (env.get_records().tobytes(), two.get_records().tobytes())
    fn = L.lib.azul_batch_mp_policy_rollout_greedy

    def call(h=env._h, agent=C.byref(w), ni=n_obs, hid=180, na=n_act, cap=8, o=out):
        return fn(h, T, agent, ni, hid, na, 1, 0, C.c_void_p(ctr.data_ptr()), cap, None if o is None else C.byref(o), C.c_float(0.9), None)

    def refused(text, **kw):
        assert call(**kw) == L.ERR_INVALID
        msg = L.lib.azul_last_error_string().decode()
        assert msg.startswith("azul_batch_mp_policy_rollout_greedy:") and text in msg, msg

    refused("bad arguments", agent=None)
    refused("bad arguments", o=None)
    refused("two-player batch of 128-byte records: use azul_batch_policy_rollout_greedy", h=two._h, ni=136, na=180)
    refused("hidden size 180", hid=64)
    refused("azul_batch_obs_size", ni=n_obs + 1)
    refused("azul_batch_num_actions", na=n_act + 30)
    refused("max_replies must be at least 1", cap=0)
    refused("opp_slots must be positive", o=L.RolloutBuffers(*ptrs, 0))
    refused("4-byte aligned", o=L.RolloutBuffers(ptrs[0] + 2, *ptrs[1:], 2))
    refused("4-byte aligned", o=L.RolloutBuffers(ptrs[0], ptrs[1] + 1, *ptrs[2:], 2))
    refused("NULL pointer", o=L.RolloutBuffers(ptrs[0], ptrs[1], ptrs[2], None, *ptrs[4:], 2))
    # (the move-limit clause cannot be reached: azul_batch_set_move_limit refuses a wide batch)
    # the two-player entry keeps refusing a wide batch under its own name
    assert L.lib.azul_batch_policy_rollout_greedy(env._h, T, C.byref(w), 136, 180, 180, 1, 0, None, C.byref(out), C.c_float(0.9), None) == L.ERR_INVALID
    assert b"wide batch" in L.lib.azul_last_error_string() and b"azul_batch_policy_rollout_greedy" in L.lib.azul_last_error_string()
    torch.cuda.synchronize()
    for t, v in zip(bufs, (1234.5, 0xA5, 0xA5, CANARY, CANARY, 0xA5, 1234.5, 1234.5, 1234.5, 0xA5, 1234.5, CANARY, 1234.5, 0xA5)):
        assert bool((t == v).all())
    assert ctr.tolist() == [0, 0] and (env.get_records().tobytes(), two.get_records().tobytes()) == before
    # and the call these refuse goes through
    assert call() == L.SUCCESS
    torch.cuda.synchronize()
    assert ctr.tolist() == [T, 0] and not bool((bufs[3] == CANARY).any()) and not bool((bufs[13] == 0xA5).all())
    assert bool((bufs[12] == 1234.5).all())                 # opp_logp is never written
    assert bool(torch.isfinite(bufs[10]).all()) and not bool((bufs[10] == 1234.5).all())       # the returns scan ran behind the launch


def _trainer(tmp_path, seed, seed_base, **kw):
    from azul_deep_reinforcement_learning_amd.training import BatchedTrainer
    players, rules = SHAPES[1]
    n_obs, n_act = _dims(players, rules)
    torch.manual_seed(seed)
    return BatchedTrainer(BatchedActorCritic(n_obs, n_act, 180), players=players, rules=rules, opponent="greedy_margin", fused_wide=True,
                          fused_seats=True, seed_base=seed_base, results_dir=str(tmp_path), **kw)


def test_trainer_with_the_fused_learner_trains_and_resumes_exactly(tmp_path):
    from azul_deep_reinforcement_learning_amd.training import AGENT_STAT_KEYS
    kw = dict(fused_learner=True, n_games=256, window=24)
    tr = _trainer(tmp_path, 4, 11, **kw)
    ro = tr.rollout
    assert ro.opponent == "greedy_margin" and ro.fused_seats and ro.fused_wide and ro.ring == 3 and not ro.use_graph
    rows = [tr.run_batch() for _ in range(4)]
    torch.cuda.synchronize()
    assert tr.learner.updates == 4
    for r in rows:
        assert all(np.isfinite(r[k]) for k in AGENT_STAT_KEYS[1:]), r
    ck = str(tmp_path / "greedy_margin.pt")
    tr.save_checkpoint(ck)
    saved = torch.load(ck, map_location="cpu", weights_only=False)
    assert saved["ring"] == 3 and "ring_buffers" in saved and "opponent" not in saved
    state = lambda t: ({k: v.detach().cpu().clone() for k, v in t.rollout.policy.state_dict().items()}, t.rollout.envs[0].get_records().tobytes(),
                       t.rollout.envs[0].get_rng_range(), t.rollout.work[0]["counter"].tolist(),
                       {k: v.cpu().clone() for k, v in t.rollout.traj[0].items()})
    row_a = tr.run_batch()                                  # the fifth batch of the uninterrupted run
    tr.rollout.synchronize()
    want = state(tr)
    tr2 = _trainer(tmp_path, 99, 9000, **kw)
    tr2.load_checkpoint(ck)
    row_b = tr2.run_batch()
    tr2.rollout.synchronize()
    got = state(tr2)
    assert tr2.batch == 5
    for k in want[0]:
        assert torch.equal(want[0][k], got[0][k]), k
    assert want[1] == got[1] and np.array_equal(want[2][0], got[2][0]) and np.array_equal(want[2][1], got[2][1]) and want[3] == got[3]
    for k in want[4]:
        _eq(want[4][k], got[4][k], k)
    for k in AGENT_STAT_KEYS[1:]:
        assert row_a[k] == row_b[k], k


def test_trainer_on_the_pytorch_wide_learner(tmp_path):
    from azul_deep_reinforcement_learning_amd.training import AGENT_STAT_KEYS
    tr = _trainer(tmp_path, 4, 11, n_games=8, window=8)
    assert tr.rollout.opponent == "greedy_margin" and tr.rollout.fused_seats and tr.rollout.ring == 1
    rows = [tr.run_batch() for _ in range(2)]
    torch.cuda.synchronize()
    assert tr.learner.updates == 2
    for r in rows:
        assert all(np.isfinite(r[k]) for k in AGENT_STAT_KEYS[1:]), r
