"""GPU parity of the self-play kernel's round-end scoring paths (az2::count_score2_lone / count_score2) against the oracle, on the crafted
records of tests/lone_round_end_cases.py: a lone round end in the lower and in the upper half of a wave, both halves on the same move, a lone
round end that ends the game through either player's wall row, one whose next deal folds the lid tally into an empty box, and the single
game of an odd batch's last wave.  Records written through the zero-copy view run the default instantiation of the kernel; records handed in
with set_records run the marking (LIM) instantiation.  Both the benchmarked output shape (padded rows + compact records) and dense rows with
a record per move are checked; masks, actions, rewards, done flags, records, MT19937 words and positions and the counters must match."""
import numpy as np
import pytest

from oracle import oracle as oz
from tests import lone_round_end_cases as lc

pytestmark = pytest.mark.gpu

RULESETS = [
    ({"first_player": "Random", "tile_pool": "Lid"}, oz.FIRST_RANDOM, oz.POOL_LID),
    ({}, 1, oz.POOL_RANDOM),
]


@pytest.mark.parametrize("rules,fp,pool", RULESETS)
@pytest.mark.parametrize("handed_in", [False, True])
@pytest.mark.parametrize("shape", ["padded", "dense"])
def test_lone_and_shared_round_ends_on_the_device(rules, fp, pool, handed_in, shape):
    import torch
    from azul_deep_reinforcement_learning_amd import BatchedAzul
    assert torch.cuda.is_available()
    n, T, base = lc.N_GAMES, 48, 2600
    env = BatchedAzul(n, rules=rules)
    env.seed(base)
    env.runner_init()
    env.runner_init()
    streams = [oz.Stream(base + g, fp, pool) for g in range(n)]
    lc.apply(streams, pool, fp)
    rec = env.get_records()
    for g, s in enumerate(streams):
        rec[g] = np.frombuffer(s.record().tobytes(), dtype=rec.dtype)[0]
    env.set_rng_range(np.stack([s.rng_state()[0] for s in streams]), np.array([s.rng_state()[1] for s in streams], dtype=np.uint32))
    if handed_in:
        env.set_records(rec)
    else:
        raw = torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).reshape(n, -1).copy())
        env.records_dev().copy_(raw.to(env.device))
    env.reset_counters()
    ep0 = [int(s.episodes.value) for s in streams]
    if shape == "padded":
        t = env.alloc_trajectory(T, packed_mask=True, mask_pitch=192, mask_bits=False)
        env.selfplay(T, t["mask"], t["action"], t["reward"], t["done"], packed=t["packed"])
    else:
        t = env.alloc_trajectory(T, with_records=True)
        env.selfplay(T, t["mask"], t["action"], t["reward"], t["done"], t["records"])
    torch.cuda.synchronize()
    act, rew, dn, msk = (t[k].cpu().numpy() for k in ("action", "reward", "done", "mask"))
    recs = t["records"].cpu().numpy() if "records" in t else None
    packed = t["packed"].cpu().numpy() if "packed" in t else None
    final, cnt = env.get_records(), env.counters()
    mt, pos = env.get_rng_range()
    for g, s in enumerate(streams):
        o = s.advance(T)
        assert np.array_equal(o["action"], act[:, g]) and np.array_equal(o["reward"], rew[:, g]) and np.array_equal(o["done"], dn[:, g]), g
        assert np.array_equal(o["mask"], msk[:, g]), g
        if recs is not None:
            assert o["rec_after"].tobytes() == recs[:, g].tobytes(), g
        if packed is not None:
            p = packed[:, g].astype(np.uint32)
            a = (p & 0xFF).astype(np.int32)
            a[a == 0xFF] = -1
            assert np.array_equal(a, o["action"]) and np.array_equal((p >> 8) & 0xFF, o["done"]), g
            assert np.array_equal((p >> 16).astype(np.uint16).view(np.int16).astype(np.int32), o["reward"]), g
        assert s.record().tobytes() == final[g].tobytes(), g
        smt, spos = s.rng_state()
        assert np.array_equal(smt, mt[g]) and spos == int(pos[g]), g
        assert int(cnt["episodes"][g]) == int(s.episodes.value) - ep0[g] and int(cnt["stuck"][g]) == 0, g
        assert np.allclose(cnt["stat_sums"][g], s.stats_sum, rtol=0, atol=1e-9), g
    # the crafted game-ending round ends did end their games
    assert all(int(cnt["episodes"][g]) >= 1 for g, kind in lc.CASES.items() if kind.startswith("over"))
