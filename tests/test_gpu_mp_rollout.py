"""GPU: PolicyRollout(players=3 | 4) and BatchedTrainer(players=3) -- every recorded step's env side replays through the model composed from the
oracle (tests/mp_runner_model.py), the actions are what the torch forward on the recorded observations gives, training runs with finite
losses and counted episodes, and a checkpointed run resumed equals the uninterrupted one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def replay(ro, windows, mode):
    """Run `windows` windows and replay every step of every game through the model (agent_step for "random", policy_step for None)."""
    from azul_deep_reinforcement_learning_amd.batch import parse_rules
    from tests.mp_runner_model import MPRunner
    env = ro.envs[0]
    first, pool = parse_rules(env.rules, env.players)
    models = [MPRunner(env.players, first, pool, env.ext, seed=ro.game_id_base + g) for g in range(ro.n)]      # game p * h + i: part p, row i
    for m in models:
        m.runner_init()
        if mode == "random":
            m.reset()
        else:
            m.runner_init()
    persp = (lambda m: 0) if mode == "random" else (lambda m: m.g.current_player - 1)
    obs0 = torch.cat([t["obs"][ro.T] for t in ro.traj]).cpu().numpy()
    for g, m in enumerate(models):
        assert np.array_equal(obs0[g], m.obs(persp(m)).astype(np.float32)), g
    pol = ro.policy
    for w in range(windows):
        parts = ro.run_window()
        torch.cuda.synchronize()
        tr = {k: torch.cat([part[k] for part in parts], dim=-1 if k in ("action", "reward", "done", "log_prob") else 1).cpu()
              for k in ("obs", "mask", "action", "reward", "done", "log_prob")}
        with torch.no_grad():
            for t in range(ro.T):
                obs, mask, act = tr["obs"][t].cuda(), tr["mask"][t].cuda().bool(), tr["action"][t].long()
                logits = pol.actor_linear2(torch.relu(pol.actor_linear1(obs))).masked_fill(~mask, float("-inf"))
                logp = torch.log_softmax(logits, dim=1).cpu()
                ok = act >= 0
                assert bool(mask.cpu()[ok, act[ok]].all())
                if ro.action_selection == "Max":
                    assert torch.equal(act[ok], logits.argmax(dim=1).cpu()[ok])
                assert torch.allclose(tr["log_prob"][t][ok], logp[ok.nonzero().squeeze(1), act[ok]], atol=1e-4, rtol=1e-4)
                for g, m in enumerate(models):
                    a = int(tr["action"][t][g])
                    st, rew, dn = m.agent_step(a) if mode == "random" else m.policy_step(a)
                    assert (int(tr["reward"][t][g]), int(tr["done"][t][g])) == (rew, dn), (w, t, g)
                    assert np.array_equal(tr["obs"][t + 1][g].numpy(), m.obs(persp(m)).astype(np.float32)), (w, t, g)
                    assert np.array_equal(tr["mask"][t + 1][g].numpy(), m.mask()), (w, t, g)
    recs = np.concatenate([e.get_records().view(np.uint8).reshape(ro.h, 256) for e in ro.envs])
    for g, m in enumerate(models):
        assert np.array_equal(recs[g], m.record()), g
    return models


@pytest.mark.parametrize("players,rules,opponent,selection,parts", [
    (3, {"first_player": "Random", "tile_pool": "Lid"}, "random", "Distribution", 1),
    (4, {"first_player": "Random", "tile_pool": "Random"}, "random", "Max", 2),
    (3, {"first_player": 1, "tile_pool": "Lid"}, None, "Distribution", 1),
    (4, {"first_player": "Random", "tile_pool": "Lid", "displays": "2P+1"}, None, "Max", 2),
    (3, {"first_player": "Random", "tile_pool": "Lid", "displays": "2P+1"}, "random", "Distribution", 1),
])
def test_policy_rollout_replays_through_the_model(players, rules, opponent, selection, parts):
    from azul_deep_reinforcement_learning_amd import BatchedActorCritic, MultiplayerAzul, PolicyRollout
    torch.manual_seed(players)
    probe = MultiplayerAzul(2, rules=rules, players=players, device="cuda:0")
    pol = BatchedActorCritic(probe.obs_size, probe.num_actions, 64)
    ro = PolicyRollout(pol, n_games=128, parts=parts, rules=rules, seed_base=600, device="cuda:0", window=12, opponent=opponent, players=players,
                       action_selection=selection, use_graph=False)          # (a graph's capture plays a warm-up window: compared below)
    assert not ro.fused_mlp and ro.traj[0]["mask"].shape[-1] == probe.num_actions
    replay(ro, 2, "random" if opponent == "random" else None)


@pytest.mark.parametrize("opponent", ["random", None])
def test_graph_replayed_windows_equal_eager_windows(opponent):
    from azul_deep_reinforcement_learning_amd import BatchedActorCritic, MultiplayerAzul, PolicyRollout
    rules = {"first_player": "Random", "tile_pool": "Lid", "displays": "2P+1"}
    probe = MultiplayerAzul(2, rules=rules, players=4, device="cuda:0")
    torch.manual_seed(3)
    pol = BatchedActorCritic(probe.obs_size, probe.num_actions, 64)
    mk = lambda g: PolicyRollout(pol, n_games=128, parts=2, rules=rules, seed_base=50, device="cuda:0", window=8, opponent=opponent, players=4,
                                 use_graph=g)
    rg, re = mk(True), mk(False)
    assert rg.use_graph and rg.graph_error is None
    re.run_window()                                     # the capture's warm-up window
    for _ in range(3):
        a, b = rg.run_window(), re.run_window()
        torch.cuda.synchronize()
        for pa, pb in zip(a, b):
            for k in ("obs", "mask", "player", "action", "reward", "done", "value", "log_prob", "entropy", "returns"):
                assert torch.equal(pa[k], pb[k]), k


def test_network_opponent_is_refused_for_wide_batches():
    from azul_deep_reinforcement_learning_amd import BatchedActorCritic, PolicyRollout
    pol = BatchedActorCritic(5 * 5 + 6 + 52 * 3 + 1, 180, 32)
    with pytest.raises(ValueError):
        PolicyRollout(pol, n_games=8, device="cuda:0", window=4, opponent=BatchedActorCritic(), players=3)


def _trainer(players, tmp_path, seed=0):
    from azul_deep_reinforcement_learning_amd import BatchedActorCritic, BatchedTrainer, MultiplayerAzul
    rules = {"first_player": "Random", "tile_pool": "Lid"}
    probe = MultiplayerAzul(2, rules=rules, players=players, device="cuda:0")
    torch.manual_seed(seed)
    pol = BatchedActorCritic(probe.obs_size, probe.num_actions, 64)
    return BatchedTrainer(pol, n_games=256, window=16, rules=rules, device="cuda:0", players=players, results_dir=str(tmp_path))


def test_trainer_three_players_trains_and_resumes_exactly(tmp_path):
    tr = _trainer(3, tmp_path)
    rows = [tr.run_batch() for _ in range(4)]
    for r in rows:
        for k in ("actor_loss", "critic_loss", "entropy_loss", "ac_loss"):
            assert np.isfinite(r[k]), (k, r)
    assert sum(1 for r in rows if not np.isnan(r["player_score"])) >= 1
    assert tr.rollout.counters()["episodes"] > 0
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    for _ in range(2):
        tr.run_batch()
    tr.rollout.synchronize()
    want = ({k: v.detach().cpu() for k, v in tr.rollout.policy.state_dict().items()}, tr.rollout.envs[0].get_records().view(np.uint8).copy(),
            tr.rollout.envs[0].get_rng_range())
    tr2 = _trainer(3, tmp_path, seed=1)
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
