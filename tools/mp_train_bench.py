"""Wide-batch training measurements (3 / 4 players): for every wide shape (p3_d5, p4_d5, p3_d7, p4_d9) at --games games, window --window and ring --ring,
  * the share of recorded agent steps that reach the learner: the complete-only selection of one window (today's wide path,
    update_from_windows) against the ring selection (PolicyRollout(fused_wide=True, wide_ring=k) + azul_select_episode_samples);
  * the time of one update on the same samples: fused (azul_a2c_gradients + azul_a2c_apply_adam_n) against A2CLearner(fused=False);
  * BatchedTrainer.run_batch batches/s: fused_wide=True (PyTorch learner) against fused_wide=True, fused_learner=True.
Prints one JSON document (--out writes it too).  --shapes selects shapes; --quick runs fewer windows (for a profiler run)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from azul_deep_reinforcement_learning_amd import _lib as L                          # noqa: E402
from azul_deep_reinforcement_learning_amd.learner import A2CLearner                 # noqa: E402
from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic          # noqa: E402
from azul_deep_reinforcement_learning_amd.rollout import PolicyRollout              # noqa: E402
from azul_deep_reinforcement_learning_amd.training import BatchedTrainer            # noqa: E402

SHAPES = {
    "p3_d5": (3, {"first_player": "Random", "tile_pool": "Lid"}, 188, 180),
    "p4_d5": (4, {"first_player": "Random", "tile_pool": "Lid"}, 240, 180),
    "p3_d7": (3, {"first_player": "Random", "tile_pool": "Lid", "displays": "2P+1"}, 198, 240),
    "p4_d9": (4, {"first_player": "Random", "tile_pool": "Random", "displays": "2P+1", "short_deal": True}, 260, 300),
}


def _p(t):
    return C.c_void_p(t.data_ptr())


def _ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def measure(name, games, window, ring, windows, reps, batches):
    players, rules, n_obs, n_act = SHAPES[name]
    torch.manual_seed(0)
    net = BatchedActorCritic(n_obs, n_act, 180).cuda()
    fl = A2CLearner(net, distributed=False, fused=True)
    ro = PolicyRollout(net, n_games=games, seed_base=1, window=window, rules=rules, players=players, opponent="random", fused_wide=True,
                       wide_ring=ring, kweights=fl.kweights())
    fl.optimizer = torch.optim.SGD(net.parameters(), lr=0.0)                   # selection only: the policy stays fixed
    T, N = window, games
    idx = torch.empty(T * N, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    recorded = complete = ringsel = 0
    warm = ring                                                                 # the ring's books start with the first window
    for w in range(windows):
        tr = ro.run_window()
        fl.update_from_rollout(ro)
        L.check(L.lib.azul_select_complete_samples(_p(tr[0]["done"]), _p(tr[0]["action"]), T, N, _p(idx), _p(cnt),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        if w >= warm:
            recorded += int((tr[0]["action"] >= 0).sum())
            complete += int(cnt[0])
            ringsel += int(fl._ring["count"][0])
    dropped = int(fl.dropped_steps[1])
    # one update on the ring's last selection: fused against PyTorch on the same samples
    st = fl._ring
    n_sel = int(st["count"][0])
    sel = st["index"][:n_sel].long()
    rg = ro.rings[0]
    R = ring * T
    obs, mask = rg["obs"][:R].reshape(R * N, -1)[sel].contiguous(), rg["mask"][:R].reshape(R * N, -1)[sel].contiguous()
    act, ret = rg["action"].reshape(-1)[sel].contiguous(), rg["returns"].reshape(-1)[sel].contiguous()
    f2 = A2CLearner(BatchedActorCritic(n_obs, n_act, 180).cuda(), distributed=False, fused=True)
    p2 = A2CLearner(BatchedActorCritic(n_obs, n_act, 180).cuda(), distributed=False, fused=False)
    fused_ms = _ms(lambda: f2.update(obs, mask, act, ret), reps)
    torch_ms = _ms(lambda: p2.update(obs, mask, act, ret), reps)
    grad_ms = _ms(lambda: f2._fused_gradients(obs, mask, act, ret, n_total=n_sel), reps)
    del ro, fl, f2, p2
    torch.cuda.empty_cache()
    # trainer batches/s, old (PyTorch learner, complete-only) against new (fused learner on the ring)
    rate = {}
    for key, kw in (("pytorch_learner", {}), ("fused_learner", {"fused_learner": True})):
        torch.manual_seed(0)
        trn = BatchedTrainer(BatchedActorCritic(n_obs, n_act, 180), n_games=games, window=window, ring=ring, players=players, rules=rules,
                             device="cuda:0", fused_wide=True, **kw)
        for _ in range(2):
            trn.run_batch(collect_stats=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(batches):
            trn.run_batch(collect_stats=False)
        torch.cuda.synchronize()
        rate[key] = batches / (time.perf_counter() - t0)
        del trn
        torch.cuda.empty_cache()
    return {"games": games, "window": window, "ring": ring, "windows_counted": windows - warm,
            "recorded_agent_steps": recorded, "trained_complete_only": complete, "trained_ring": ringsel,
            "share_complete_only": complete / max(recorded, 1), "share_ring": ringsel / max(recorded, 1), "ring_dropped_steps": dropped,
            "update_samples": n_sel, "update_ms_fused": fused_ms, "update_ms_pytorch": torch_ms, "gradients_ms_fused": grad_ms,
            "fused_speedup": torch_ms / fused_ms,
            "run_batch_per_s_pytorch_learner": rate["pytorch_learner"], "run_batch_per_s_fused_learner": rate["fused_learner"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--ring", type=int, default=3)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.quick:
        a.windows, a.reps, a.batches = a.ring + 2, 3, 3
    res = {"device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in a.shapes.split(","):
        res["shapes"][name] = measure(name, a.games, a.window, a.ring, a.windows, a.reps, a.batches)
        print(name, json.dumps(res["shapes"][name]), flush=True)
    s = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")
    print(s)


if __name__ == "__main__":
    main()
