"""GPU: GameRunner(opponent=<network>) for 3- and 4-player games -- the azul_batch_mp_net_* entries (azul_x_net_kernel) and
PolicyRollout(players=P, opponent=<module>) / BatchedTrainer(players=P, opponent="self").

  1. The three C entries, fed the fixture's agent actions and the reference net's recorded answers (tests/golden/runner_players_net.npz),
     hand the opponent what the reference handed it, call by call, and reproduce every step; the model (tests/mp_net_model.py) runs in
     lockstep and the records, tails and MT19937 streams equal its own.
  2. PolicyRollout with a network opponent, "Max": every step replays through the model with the traced answers, and every traced answer is
     the argmax of the torch forward on the model's mover-perspective observation.
  3. "Distribution" with parts=1 and parts=2 gives identical trajectories (sampling keys follow the global game id).
  4. BatchedTrainer(players=3, opponent="self", opponent_refresh=2) trains, and a checkpointed run resumed equals the uninterrupted one.
  5. An opponent that keeps answering illegally raises RuntimeError; a net of the wrong shape raises ValueError; two-player batches are
     refused by the mp_net entries."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "runner_players_net.npz")


def _stems():
    return sorted({str(k).rsplit("_", 1)[0] for k in np.load(GOLDEN)["keys"]})


@pytest.mark.parametrize("stem", _stems())
def test_entries_replay_the_reference_call_by_call(stem):
    from azul_deep_reinforcement_learning_amd import MultiplayerAzul
    from oracle import oracle as oz
    from tests.mp_net_model import READY, MPNetRunner
    from tests.test_mp_runner_model import parse_key
    z = np.load(GOLDEN)
    keys = [k for k in (str(x) for x in z["keys"]) if k.rsplit("_", 1)[0] == stem]
    P, first, pool = parse_key(keys[0])
    n = len(keys)
    fp = "Random" if first == oz.FIRST_RANDOM else first
    env = MultiplayerAzul(n, rules={"first_player": fp, "tile_pool": "Lid" if pool == oz.POOL_LID else "Random"}, players=P, device="cuda:0")
    env.set_rng_range(np.stack([z[k + "__mt0"] for k in keys]), np.array([int(z[k + "__pos0"]) for k in keys]))
    models = []
    for k in keys:
        r = oz.Rng()
        oz.lib().oz_rng_set(C.byref(r), np.ascontiguousarray(z[k + "__mt0"], np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), int(z[k + "__pos0"]))
        models.append(MPNetRunner(P, first, pool, rng=r))
        assert models[-1].runner_init() == 0
    assert (env.runner_init().cpu().numpy() == 0).all()
    net = env.net_state()
    d = "cuda:0"
    reward, done, status = (torch.zeros(n, dtype=torch.int32, device=d), torch.zeros(n, dtype=torch.uint8, device=d),
                            torch.zeros(n, dtype=torch.uint8, device=d))
    nxt = [0] * n

    def replies():
        rounds = 0
        while int(net["owing"].item()) > 0:
            pend = net["pending"].cpu().numpy()
            obs, mask = net["obs"].cpu().numpy(), net["mask"].cpu().numpy()
            ans = np.full(n, -3, np.int32)
            for g, k in enumerate(keys):
                assert (pend[g] != 0) == (models[g].pending != READY), (g, rounds)
                if pend[g]:
                    i = nxt[g]
                    assert np.array_equal(obs[g], z[k + "__call_state"][i].astype(np.float32)), (k, i)        # get_state(mover), :38
                    assert np.array_equal(mask[g], z[k + "__call_mask"][i]), (k, i)
                    assert models[g].g.current_player == int(z[k + "__call_player"][i]) and models[g].moves == int(z[k + "__call_moves"][i])
                    ans[g] = int(z[k + "__call_answer"][i])
                    nxt[g] += 1
                    models[g].net_reply(ans[g])
            net["action"].copy_(torch.from_numpy(ans))
            env.net_step_reply(net["action"], net, reward, done, status)
            rounds += 1
            assert rounds < 200

    env.net_reset_begin(net, status)
    for m in models:
        m.net_reset()
    replies()
    phi_prev = [0] * n
    for t in range(len(z[keys[0] + "__action"])):
        acts = [int(z[k + "__action"][t]) for k in keys]
        for g, m in enumerate(models):
            m.net_begin(acts[g])
        env.net_step_begin(torch.tensor(acts, dtype=torch.int32, device=d), net, reward, done, status)
        replies()
        rw, dn, st = reward.cpu().numpy(), done.cpu().numpy(), status.cpu().numpy()
        obs0, mask0, _ = env.observe_all(0)
        obs0, mask0 = obs0.cpu().numpy(), mask0.cpu().numpy()
        for g, k in enumerate(keys):
            s = z[k + "__whatif"][t][:P]
            phi = int(s[0] - max(s[1:]))
            assert (st[g], rw[g], dn[g]) == (0, phi - phi_prev[g], int(z[k + "__done"][t])), (k, t)
            phi_prev[g] = 0 if dn[g] else phi
            assert (rw[g], dn[g]) == (models[g].rew, models[g].dn)
            assert np.array_equal(obs0[g], z[k + "__obs"][t].astype(np.float32)) and np.array_equal(mask0[g], z[k + "__mask"][t]), (k, t)
            assert nxt[g] == int((z[k + "__call_step"] <= t).sum()), (k, t)
        mt, pos = env.get_rng_range()
        for g, k in enumerate(keys):
            assert int(pos[g]) == int(z[k + "__pos"][t]) and np.array_equal(mt[g], z[k + "__mt"][t]), (k, t)
    recs = env.get_records().view(np.uint8).reshape(n, 256)
    for g, m in enumerate(models):
        assert np.array_equal(recs[g], m.record()), g
    assert [int(x) for x in env.counters()["episodes"]] == [int(z[k + "__done"].sum()) for k in keys]


def _nets(players, rules, hidden_agent=64, hidden_opp=48, seed=0):
    from azul_deep_reinforcement_learning_amd import BatchedActorCritic, MultiplayerAzul
    probe = MultiplayerAzul(2, rules=rules, players=players, device="cuda:0")
    torch.manual_seed(seed)
    return (BatchedActorCritic(probe.obs_size, probe.num_actions, hidden_agent).cuda(),
            BatchedActorCritic(probe.obs_size, probe.num_actions, hidden_opp).cuda())


def _opp_logits(ro, obs):
    """The opponent's forward exactly as the rollout computes it (same shapes, same GEMMs)."""
    Ho = ro.ob1.numel() // 2
    hid = torch.relu(torch.addmm(ro.ob1[Ho:], obs, ro.ow1t[:, Ho:]))
    return torch.addmm(ro.ob2a, hid, ro.ow2a_t)


@pytest.mark.parametrize("players,rules", [
    (3, {"first_player": "Random", "tile_pool": "Lid"}),
    (4, {"first_player": 1, "tile_pool": "Random"}),
    (3, {"first_player": "Random", "tile_pool": "Lid", "displays": "2P+1", "bonuses": "end"}),
])
def test_rollout_with_a_network_opponent_replays_through_the_model(players, rules):
    from azul_deep_reinforcement_learning_amd import PolicyRollout
    from azul_deep_reinforcement_learning_amd.batch import parse_ext_rules, parse_rules
    from tests.mp_net_model import READY, MPNetRunner
    pol, opp = _nets(players, rules, seed=players)
    N, T, R = 64, 8, 40
    ro = PolicyRollout(pol, n_games=N, rules=rules, seed_base=700, device="cuda:0", window=T, opponent=opp, players=players,
                       action_selection="Max", opponent_selection="Max", opponent_trace=R)
    assert ro.opponent == "net" and not ro.use_graph
    first, pool = parse_rules(rules, players)
    models = [MPNetRunner(players, first, pool, parse_ext_rules(rules, players), seed=700 + g) for g in range(N)]
    dev = ro.device

    def rounds(traced=None):
        """Reply rounds of all models in lockstep; every answer is the argmax of the rollout's own forward on the model's view."""
        j = 0
        while any(m.pending != READY for m in models):
            obs = torch.zeros(N, ro.obs_size, device=dev)
            mask = torch.zeros(N, ro.num_actions, dtype=torch.bool, device=dev)
            for g, m in enumerate(models):
                if m.pending != READY:
                    o, k, _ = m.opp_view()
                    obs[g], mask[g] = torch.from_numpy(o), torch.from_numpy(k.astype(bool))
            with torch.no_grad():
                ans = _opp_logits(ro, obs).masked_fill(~mask, float("-inf")).argmax(dim=1).cpu().numpy()
            for g, m in enumerate(models):
                if m.pending != READY:
                    if traced is not None:
                        assert int(traced[j][g]) == int(ans[g]), (j, g)
                    m.net_reply(int(ans[g]))
            j += 1
            assert j < R
        return j

    for m in models:
        assert m.runner_init() == 0
        m.net_reset()
    rounds()
    for w in range(2):
        tr = ro.run_window()[0]
        torch.cuda.synchronize()
        tr = {k: v.cpu() for k, v in tr.items()}
        for t in range(T):
            for g, m in enumerate(models):
                assert np.array_equal(tr["obs"][t][g].numpy(), m.obs(0).astype(np.float32)), (w, t, g)
                m.net_begin(int(tr["action"][t][g]))
            rounds(tr["opp_action"][t])
            for g, m in enumerate(models):
                assert (int(tr["reward"][t][g]), int(tr["done"][t][g]), int(tr["opp_replies"][t][g])) == (m.rew, m.dn, m.replies), (w, t, g)
    recs = ro.envs[0].get_records().view(np.uint8).reshape(N, 256)
    for g, m in enumerate(models):
        assert np.array_equal(recs[g], m.record()), g
    assert ro.counters()["episodes"] == sum(m.episodes for m in models)


def test_distribution_sampling_does_not_depend_on_parts():
    from azul_deep_reinforcement_learning_amd import PolicyRollout
    rules = {"first_player": "Random", "tile_pool": "Lid"}
    pol, opp = _nets(4, rules, seed=9)
    outs = []
    for parts in (1, 2):
        ro = PolicyRollout(pol, n_games=128, parts=parts, rules=rules, seed_base=40, device="cuda:0", window=6, opponent=opp, players=4,
                           opponent_trace=8)
        got = []
        for _ in range(2):
            tr = ro.run_window()
            torch.cuda.synchronize()
            got.append({k: torch.cat([part[k] for part in tr], dim=-1 if k in ("action", "reward", "done", "log_prob", "opp_replies") else
                                     (2 if k in ("opp_action", "opp_logp") else 1)).cpu()
                        for k in ("obs", "mask", "action", "reward", "done", "log_prob", "opp_action", "opp_logp", "opp_replies")})
        outs.append(got)
    for a, b in zip(*outs):
        # a trace slot holds an answer only for the games that owed reply j (j < opp_replies); the rows of the others are not defined
        R = a["opp_action"].shape[1]
        owed = torch.arange(R).view(1, R, 1) < a["opp_replies"].long().unsqueeze(1)
        for k in a:
            x, y = (a[k][owed], b[k][owed]) if k in ("opp_action", "opp_logp") else (a[k], b[k])
            if k in ("log_prob", "opp_logp"):
                assert torch.allclose(x, y, atol=1e-5, rtol=1e-5), k
            else:
                assert torch.equal(x, y), k
    assert (outs[0][1]["opp_replies"] > 0).any()


def _trainer(tmp_path, seed=0):
    from azul_deep_reinforcement_learning_amd import BatchedActorCritic, BatchedTrainer, MultiplayerAzul
    rules = {"first_player": "Random", "tile_pool": "Lid"}
    probe = MultiplayerAzul(2, rules=rules, players=3, device="cuda:0")
    torch.manual_seed(seed)
    pol = BatchedActorCritic(probe.obs_size, probe.num_actions, 64)
    return BatchedTrainer(pol, n_games=256, window=24, rules=rules, device="cuda:0", players=3, results_dir=str(tmp_path), opponent="self",
                          opponent_refresh=2)


def test_trainer_against_a_past_self_trains_and_resumes_exactly(tmp_path):
    tr = _trainer(tmp_path)
    assert tr.rollout.opponent == "net"
    rows = [tr.run_batch() for _ in range(4)]
    # (no HIP graph on this path, so no warm-up window: the first window may hold no finished episode, hence no sample)
    for r in rows[1:]:
        for k in ("actor_loss", "critic_loss", "entropy_loss", "ac_loss"):
            assert np.isfinite(r[k]), (k, r)
    assert tr.rollout.counters()["episodes"] > 0
    # opponent_refresh=2: after update 4 the opponent is the policy of update 4
    for k, v in tr.rollout.policy.state_dict().items():
        if k.startswith("actor_linear2.weight"):
            assert torch.equal(tr.rollout.ow2a_t, v.t())
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    for _ in range(3):
        tr.run_batch()
    tr.rollout.synchronize()
    want = ({k: v.detach().cpu() for k, v in tr.rollout.policy.state_dict().items()}, tr.rollout.envs[0].get_records().view(np.uint8).copy(),
            tr.rollout.envs[0].get_rng_range(), tr.rollout.ow1t.cpu())
    tr2 = _trainer(tmp_path, seed=1)
    tr2.load_checkpoint(path)
    for _ in range(3):
        tr2.run_batch()
    tr2.rollout.synchronize()
    got = ({k: v.detach().cpu() for k, v in tr2.rollout.policy.state_dict().items()}, tr2.rollout.envs[0].get_records().view(np.uint8).copy(),
           tr2.rollout.envs[0].get_rng_range(), tr2.rollout.ow1t.cpu())
    for k in want[0]:
        assert torch.equal(want[0][k], got[0][k]), k
    assert np.array_equal(want[1], got[1])
    assert np.array_equal(want[2][0], got[2][0]) and np.array_equal(want[2][1], got[2][1])
    assert torch.equal(want[3], got[3])


def test_an_opponent_that_keeps_answering_illegally_raises():
    from azul_deep_reinforcement_learning_amd import PolicyRollout
    rules = {"first_player": "Random", "tile_pool": "Lid"}
    pol, opp = _nets(3, rules, seed=2)
    ro = PolicyRollout(pol, n_games=16, rules=rules, seed_base=5, device="cuda:0", window=4, opponent=opp, players=3)
    ro.MAX_REPLY_ROUNDS = 16
    bad = {k: torch.full_like(v, float("nan")) for k, v in opp.state_dict().items()}
    ro.set_opponent(bad)
    with pytest.raises(RuntimeError, match="reply rounds"):
        ro.run_window()
    torch.cuda.synchronize()


def test_wrong_shapes_and_two_player_batches_are_refused():
    from azul_deep_reinforcement_learning_amd import BatchedActorCritic, BatchedAzul, PolicyRollout
    from azul_deep_reinforcement_learning_amd import _lib as L
    pol = BatchedActorCritic(5 * 5 + 6 + 52 * 3 + 1, 180, 32)
    for bad in (BatchedActorCritic(5 * 5 + 6 + 52 * 3 + 1, 240, 32), BatchedActorCritic(5 * 5 + 6 + 52 * 4 + 1, 180, 32)):
        with pytest.raises(ValueError, match="ActorCritic\\(188, 180"):
            PolicyRollout(pol, n_games=8, device="cuda:0", window=4, opponent=bad, players=3)
    env = BatchedAzul(8, device="cuda:0", seed=1)
    net = env.net_state()
    one = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    u8 = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    h, p = env._h, lambda t: C.c_void_p(t.data_ptr())
    calls = {"azul_batch_net_step_begin": lambda: L.lib.azul_batch_mp_net_step_begin(h, p(one), p(net["pending"]), None, p(one), p(u8), p(u8),
                                                                                       None, None, p(net["owing"]), None),
             "azul_batch_net_step_reply": lambda: L.lib.azul_batch_mp_net_step_reply(h, p(one), p(net["pending"]), None, p(one), p(u8), p(u8),
                                                                                       None, None, p(net["owing"]), None),
             "azul_batch_net_reset_begin": lambda: L.lib.azul_batch_mp_net_reset_begin(h, None, p(net["pending"]), p(u8), None, None,
                                                                                         p(net["owing"]), None)}
    for name, fn in calls.items():
        assert fn() == L.ERR_INVALID
        assert name in L.lib.azul_last_error_string().decode()
    with pytest.raises(L.AzulHipError, match="GameRunner is two-player"):      # the two-player entries keep refusing wide batches
        wide = BatchedAzul(8, players=3, device="cuda:0")  # (the family is the class's: a plain BatchedAzul calls azul_batch_net_*)
        wide.net_reset_begin(wide.net_state(), torch.zeros(8, dtype=torch.uint8, device="cuda:0"))
