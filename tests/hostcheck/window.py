"""The Python side of the two window shims (tests/hostcheck/simt_rollout2.cpp: sr2_window, simt_x_rollout.cpp: sxr_window): the ctypes mirror
of their one call block (simt_window_call.hpp), one loader per family, run(), and the helpers and fixtures the window test modules share
(tests/test_hostcheck_rollout2*.py, test_hostcheck_rollout_greedy.py, test_hostcheck_x_rollout*.py) -- none of them imports another."""
import ctypes as C
import os
import random

import numpy as np

from oracle import oracle as oz
from tests.hostcheck import hostcheck
from tests.mp_net_model import MPNetRunner
from tests.test_hostcheck_env2 import RULES, start_batch

KEYS = ("w1t", "b1", "w2c", "b2c", "w2a_t", "b2a")
ARGMAX = 0xFFFFFFFFFFFFFFFF
GROUP = 16                     # games of a league / arena group: one workgroup's
_I32, _U32, _U64, _PTR, _NET = C.c_int32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p * 6


class WindowCall(C.Structure):
    """SimtWindowCall, field by field in its order; every pointer a void pointer (load2 / load_x compare the sizes)."""
    _fields_ = ([(k, _I32) for k in ("n_games", "players", "displays", "first_player", "pool", "end_bonus", "short_deal")]
                + [("id_base", _U32), ("move_limit", _U32)] + [(k, _PTR) for k in ("state", "mt", "mtpos", "episodes", "stuck", "stat_sum")]
                + [("opp", _I32), ("agent", _NET), ("opponent", _NET), ("pool_size", _I32), ("opp_member", _PTR), ("agent_member", _PTR),
                   ("n_steps", _I32), ("max_replies", _I32)]
                + [(k, _PTR) for k in ("obs", "mask", "player", "action", "reward", "done", "value", "logp", "entropy", "status", "returns")]
                + [("gamma", C.c_float), ("seed", _U64), ("opp_seed", _U64), ("counter", _U64), ("opp_action", _PTR), ("opp_logp", _PTR),
                   ("opp_replies", _PTR), ("opp_slots", _I32)])


_TYPES = dict(WindowCall._fields_)


def load2(name=None):
    """The two-player shim (tests/hostcheck/run_sanitizers.sh: libsimt_rollout2_asan.so / _ubsan.so)."""
    L = C.CDLL(hostcheck.build(name or os.environ.get("AZUL_SIMT_ROLLOUT_LIB", "libsimt_rollout2.so")))
    L.sr2_window.restype, L.sr2_window.argtypes = C.c_longlong, [C.POINTER(WindowCall)]
    L.sr2_buffer_oob.restype = L.sr2_call_bytes.restype = C.c_ulonglong
    assert C.sizeof(WindowCall) == L.sr2_call_bytes()
    L.window = L.sr2_window
    return L


def load_x():
    """The wide shim."""
    L = C.CDLL(hostcheck.build("libsimt_x_rollout.so"))
    L.sxr_window.restype, L.sxr_window.argtypes = C.c_longlong, [C.POINTER(WindowCall)]
    L.sxr_buffer_oob.restype = L.sxr_call_bytes.restype = C.c_ulonglong
    assert C.sizeof(WindowCall) == L.sxr_call_bytes()
    L.window = L.sxr_window
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pointers(w):
    return (C.c_void_p * 6)(*[w[k].ctypes.data for k in KEYS])


def run(L, **fields):
    """One launch through the shim's entry.  Fields by the names of WindowCall: a NumPy array (or None) for a pointer, a dict of the six
    weight arrays (weights2 / weights_x; stacked for a pool) for agent / opponent, a number for the rest; what is not named stays zero /
    NULL.  Returns the entry's result.  (`fields` holds every array for the duration of the call.)"""
    call = WindowCall()
    for k, v in fields.items():
        if k not in _TYPES:
            raise TypeError("WindowCall has no field %r" % k)
        t = _TYPES[k]
        setattr(call, k, ptr(v) if t is _PTR else pointers(v) if t is _NET else float(v) if t is C.c_float else int(v))
    return L.window(C.byref(call))


# ---- the two-player tests --------------------------------------------------------------------------------------------------------------
def weights2(seed):
    rs = np.random.RandomState(seed)
    w = {"w1t": rs.randn(136, 360) * 0.08, "b1": rs.randn(360) * 0.05, "w2c": rs.randn(180) * 0.1, "b2c": rs.randn(1) * 0.1,
         "w2a_t": rs.randn(180, 180) * 0.12, "b2a": rs.randn(180) * 0.05}
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


def forward(w, obs, mask):
    """model.py:22-41 on one observation, fp32; masked log-softmax and the entropy term of agent.py:64-72 / nn_runner.py:32-40."""
    h = np.maximum(obs.astype(np.float32) @ w["w1t"] + w["b1"], np.float32(0))
    value = np.float32(h[:180] @ w["w2c"] + w["b2c"][0])
    logits = (h[180:] @ w["w2a_t"] + w["b2a"]).astype(np.float64)
    legal = mask.astype(bool)
    z = logits[legal]
    lse = z.max() + np.log(np.exp(z - z.max()).sum())
    logp = np.full(180, -np.inf)
    logp[legal] = z - lse
    return float(value), logp, float(-logp[legal].mean())


def to_agent_decision(rec, mt, pos, first, pool, rng):
    """Bring a flat self-play state to a point where GameRunner hands the turn to the agent (game_runner.py:46: player 1 to move with at
    least two legal moves, game not over) by letting a stand-in opponent play random legal moves."""
    run = oz.NetRunner(lambda s, m: int(rng.choice(np.flatnonzero(m))), first if first else oz.FIRST_RANDOM, pool, rec=rec, mt=mt, pos=pos)
    Lz = oz.lib()
    for _ in range(200):
        legal = int(run.get_valid_moves().sum())
        over = bool(Lz.oz_is_end_of_game(C.byref(run.q.game)))
        if over:
            assert run.reset() == 0
            continue
        if run.q.game.current_player == 1 and legal >= 2:
            break
        assert Lz.oz_runner_opponent_move_with(C.byref(run.q), C.byref(run.r), run._cb, None) == 0
    run.q.player_score = int(Lz.oz_potential(C.byref(run.q.game)))          # GameRunner.player_score follows the potential (game_runner.py:52)
    m, p = run.rng_state()
    return np.frombuffer(run.record().tobytes(), np.uint8).copy(), m, p


def games_fields(n, state, mt, pos, ep, stuck, ss, first, pool):
    """The games of a two-player call, id_base 1000 as every window test has it."""
    return dict(n_games=n, state=state, mt=mt, mtpos=pos, episodes=ep, stuck=stuck, stat_sum=ss, first_player=first, pool=pool, id_base=1000)


OUT2 = ("obs", "mask", "player", "action", "reward", "done", "value", "logp", "entropy", "status", "returns")
TRACE = ("opp_action", "opp_logp", "opp_replies")


# the batch and buffers of the two-player league and arena tests
N2, T2, SLOTS2, SEED0, WARM = 35, 5, 8, 300, 40
CASES2 = {"lid_distribution": ("lid_randomfirst", False), "lid_max": ("lid_randomfirst", True),
          "random_distribution": ("random_first1", False), "random_max": ("random_first1", True)}
_START2 = {}


def start2(ruleset):
    """The batch every run of a rule set starts from: games part-way through their episodes, at an agent decision."""
    if ruleset not in _START2:
        first, pool = RULES[ruleset]
        state, mt, pos = start_batch(N2, SEED0, first, pool, WARM)
        rng = np.random.default_rng(SEED0)
        for g in range(N2):
            state[g], mt[g], pos[g] = to_agent_decision(state[g].view(oz.RECORD_DTYPE)[0], mt[g], pos[g], first, pool, rng)
        _START2[ruleset] = (state, mt, pos)
    return tuple(x.copy() for x in _START2[ruleset])


def fresh2(ruleset):
    N, T, SLOTS = N2, T2, SLOTS2
    state, mt, pos = start2(ruleset)
    o = {"state": state, "mt": mt, "pos": pos, "ep": np.zeros(N, np.uint64), "stuck": np.zeros(N, np.uint32), "ss": np.zeros((N, 10)),
         "obs": np.full((T + 1, N, 136), -99, np.float32), "mask": np.full((T + 1, N, 180), 0xEE, np.uint8),
         "player": np.full((T + 1, N), 9, np.uint8), "action": np.full((T, N), -7, np.int32), "reward": np.full((T, N), -7777, np.int32),
         "done": np.full((T, N), 9, np.uint8), "value": np.full((T, N), np.nan, np.float32), "logp": np.full((T, N), np.nan, np.float32),
         "entropy": np.full((T, N), np.nan, np.float32), "status": np.full(N, 99, np.uint8), "returns": np.full((T, N), np.nan, np.float32),
         "opp_action": np.full((T, SLOTS, N), -9, np.int32), "opp_logp": np.full((T, SLOTS, N), np.nan, np.float32),
         "opp_replies": np.full((T, N), 200, np.uint8)}
    return o


def member_weights2(m):
    return weights2(SEED0 + 1 + m)


def window_fields2(o, ruleset, seed, argmax):
    """What the league, the arena and their single-opponent references share of a call on fresh2's buffers: all but who plays."""
    first, pool = RULES[ruleset]
    return dict(games_fields(N2, o["state"], o["mt"], o["pos"], o["ep"], o["stuck"], o["ss"], first, pool), n_steps=T2,
                **{k: o[k] for k in OUT2 + TRACE}, gamma=0.9, seed=seed, opp_seed=ARGMAX if argmax else 777, counter=17, opp_slots=SLOTS2)


GAME_AXIS = {"state": 0, "mt": 0, "pos": 0, "ep": 0, "stuck": 0, "ss": 0, "status": 0, "opp_action": 2, "opp_logp": 2}    # (the others: axis 1)


def games(o, k, idx):
    return np.ascontiguousarray(np.take(o[k], idx, axis=GAME_AXIS.get(k, 1))).tobytes()


# ---- the wide tests --------------------------------------------------------------------------------------------------------------------
GUARD = 7                      # guard cells past the end of every output array
OUT_X = ("obs", "mask", "player", "action", "reward", "done", "value", "logp", "entropy", "status")


def weights_x(n_obs, n_act, seed):
    rs = np.random.RandomState(seed)
    w = {"w1t": rs.randn(n_obs, 360) * 0.06, "b1": rs.randn(360) * 0.05, "w2c": rs.randn(180) * 0.1, "b2c": rs.randn(1) * 0.1,
         "w2a_t": rs.randn(180, n_act) * 0.12, "b2a": rs.randn(n_act) * 0.05}
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


def buf(shape, dtype, fill):
    """An output array with GUARD cells behind it: (the whole allocation, the view the kernel writes)."""
    n = int(np.prod(shape))
    whole = np.full(n + GUARD, fill, dtype)
    return whole, whole[:n].reshape(shape)


def games_fields_x(n, P, D, state, mt, pos, ep, stuck, ss, first, pool, ext, id_base):
    """The games of a wide call from the oracle's rule flags (`pool` / `ext`)."""
    xpool = 2 if ext & oz.EXT_FINITE_BAG else (1 if pool == oz.POOL_LID else 0)
    return dict(n_games=n, players=P, displays=D, state=state, mt=mt, mtpos=pos, episodes=ep, stuck=stuck, stat_sum=ss, first_player=first,
                pool=xpool, end_bonus=int(bool(ext & oz.EXT_END_BONUS)), short_deal=int(bool(ext & oz.EXT_SHORT_DEAL)), id_base=id_base)


# the batch and buffers of the wide league and arena tests
P, D, NX, TX, SLOTS_X, SEED, COUNTER, ID_BASE = 3, 5, 19, 5, 64, 0x5EED + 3, 40, 1000
NA, OBS = (D + 1) * 30, 5 * D + 6 + 52 * P + 1
CASES_X = {"lid_distribution": (oz.POOL_LID, False), "random_max": (oz.POOL_RANDOM, True)}
_START_X = {}


def start_x(pool):
    """Games part-way through their episodes (GameRunner() + reset() with a random stand-in opponent, then some agent steps)."""
    if pool not in _START_X:
        rnd = random.Random(100 * P + pool)

        def rand_answer(obs, mask, player):
            legal = np.flatnonzero(mask)
            return int(rnd.choice(list(legal))) if len(legal) else -1

        models = [MPNetRunner(P, oz.FIRST_RANDOM, pool, 0, seed=4000 + 17 * P + g) for g in range(NX)]
        for m in models:
            m.runner_init()
            m.reset_with(rand_answer)
            for _ in range(rnd.randrange(0, 45)):
                m.step_with(rand_answer(*m.opp_view()), rand_answer)
        _START_X[pool] = {"state": np.stack([m.record() for m in models]), "mt": np.stack([m.rng_state()[0] for m in models]).astype(np.uint32),
                          "pos": np.array([m.rng_state()[1] for m in models], np.uint32), "ep": np.array([m.episodes for m in models], np.uint64),
                          "stuck": np.array([m.stuck for m in models], np.uint32), "ss": np.stack([m.stat_sum for m in models]).astype(np.float64)}
    return {k: v.copy() for k, v in _START_X[pool].items()}


def fresh_x(pool):
    N, T, SLOTS = NX, TX, SLOTS_X
    o = start_x(pool)
    for k, shape, dt, fill in (("obs", (T + 1, N, OBS), np.float32, -99), ("mask", (T + 1, N, NA), np.uint8, 0xEE), ("player", (T + 1, N), np.uint8, 9),
                               ("action", (T, N), np.int32, -7), ("reward", (T, N), np.int32, -7777), ("done", (T, N), np.uint8, 9),
                               ("value", (T, N), np.float32, np.nan), ("logp", (T, N), np.float32, np.nan), ("entropy", (T, N), np.float32, np.nan),
                               ("status", (N,), np.uint8, 99), ("opp_action", (T, SLOTS, N), np.int32, -5), ("opp_logp", (T, SLOTS, N), np.float32, 55.0),
                               ("opp_replies", (T, N), np.uint8, 201)):
        o[k] = np.full(shape, fill, dt)
    return o


def member_weights_x(m):
    return weights_x(OBS, NA, SEED + 1 + m)


def head_fields(o, pool):
    return games_fields_x(NX, P, D, o["state"], o["mt"], o["pos"], o["ep"], o["stuck"], o["ss"], oz.FIRST_RANDOM, pool, 0, ID_BASE)


def tail_fields(o, argmax):
    return dict(n_steps=TX, **{k: o[k] for k in OUT_X + TRACE}, opp_slots=SLOTS_X, seed=SEED, opp_seed=ARGMAX if argmax else 0x0770 + P,
                counter=COUNTER, max_replies=512)
