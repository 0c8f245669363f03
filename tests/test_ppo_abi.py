"""azul_ppo_gradients, PPOLearner and BatchedTrainer(algorithm="ppo") without a device: the entry is declared, exported and bound; every
refusal of the header returns AZUL_ERR_INVALID before any HIP call; PPOLearner and BatchedTrainer refuse what PPO cannot serve with a
ValueError before anything is allocated; the trainer's default algorithm stays "a2c"."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "azul_ppo_gradients"


def _decl_args(header, name):
    decl = re.search(r"int %s\(([^;]*)\);" % name, header)
    assert decl, "%s is not declared in include/azul_hip.h" % name
    return [a.strip().split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", decl.group(1).replace("\n", " ")).split(",")]


def test_the_entry_is_declared_exported_and_bound():
    from azul_deep_reinforcement_learning_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "azul_hip.h")).read()
    args = _decl_args(header, ENTRY)
    a2c = _decl_args(header, "azul_a2c_gradients")
    assert args[:11] == ["obs_dev", "mask_dev", "action_dev", "returns_dev", "old_log_prob_dev", "advantage_dev", "n_samples", "inv_n_total",
                         "clip_eps", "value_coeff", "entropy_coeff"]
    assert args[11:-2] == a2c[6:-1] and args[-2:] == ["log_prob_out_dev", "stream"]       # "exactly as azul_a2c_gradients"
    assert ENTRY in L.SIGNATURES
    fn = getattr(L.lib, ENTRY)
    assert fn.restype is C.c_int and len(fn.argtypes) == len(args) == 29
    assert [fn.argtypes[i] for i in (7, 8, 9, 10)] == [C.c_float] * 4


def test_argument_checks_need_no_gpu():
    from azul_deep_reinforcement_learning_amd import _lib as L
    fn = L.lib.azul_ppo_gradients
    one = C.c_void_p(8)                                        # a non-NULL, 8-byte "aligned" placeholder; never dereferenced
    f32 = C.c_float
    ok = dict(obs=one, mask=one, action=one, ret=one, old=one, adv=one, n=16, eps=f32(0.2), cv=f32(0.5), ce=f32(0.01), shape=(136, 180, 180),
              ws=one, parts=256, grad=one)
    call = lambda **kw: (lambda a: fn(a["obs"], a["mask"], a["action"], a["ret"], a["old"], a["adv"], a["n"], f32(1.0), a["eps"], a["cv"], a["ce"],
                                      one, one, one, one, one, one, one, *a["shape"], a["ws"], a["parts"], a["grad"], None, None, None, None,
                                      None))({**ok, **kw})
    inf, nan = float("inf"), float("nan")
    refusals = [
        dict(shape=(136, 180, 181)), dict(shape=(136, 128, 180)), dict(shape=(188, 180, 240)), dict(shape=(260, 180, 180)),   # not compiled
        dict(old=None), dict(adv=None), dict(old=None, adv=None),                                       # NULL PPO inputs with samples
        dict(eps=f32(0.0)), dict(eps=f32(-0.2)), dict(eps=f32(inf)), dict(eps=f32(-inf)), dict(eps=f32(nan)),
        dict(cv=f32(-0.5)), dict(cv=f32(inf)), dict(cv=f32(nan)), dict(ce=f32(-0.01)), dict(ce=f32(inf)), dict(ce=f32(nan)),
        dict(obs=None), dict(ret=None), dict(ws=None), dict(grad=None), dict(parts=0), dict(n=-1),      # azul_a2c_gradients' own checks
    ]
    for kw in refusals:
        assert call(**kw) == L.ERR_INVALID, kw
        assert L.lib.azul_last_error_string().decode().startswith(ENTRY + ":"), kw
    for shape in ((136, 180, 180), (188, 180, 180), (240, 180, 180), (198, 180, 240), (260, 180, 300)):
        assert call(shape=shape, eps=f32(-1.0)) == L.ERR_INVALID and b"clip_eps" in L.lib.azul_last_error_string()    # the shape passes
    with pytest.raises(L.AzulHipError, match=ENTRY):
        L.check(call(eps=f32(0.0)))
    # the A2C entry keeps its name in its own messages
    assert L.lib.azul_a2c_gradients(one, one, one, one, 16, f32(1.0), one, one, one, one, one, one, one, 136, 180, 181, one, 256, one, None,
                                    None, None, None) == L.ERR_INVALID
    assert L.lib.azul_last_error_string().decode().startswith("azul_a2c_gradients:") and b"136, 180" in L.lib.azul_last_error_string()


def _net(obs=136, act=180, hidden=180):
    from azul_deep_reinforcement_learning_amd import BatchedActorCritic
    return BatchedActorCritic(obs, act, hidden)


def test_learner_refusals_come_before_any_allocation():
    from azul_deep_reinforcement_learning_amd.learner import A2CLearner, PPOLearner
    for kw, match in [({"distributed": True}, "single-process"), ({"epochs": 0}, "epochs and minibatches"), ({"epochs": -2}, "epochs and minibatches"),
                      ({"minibatches": 0}, "epochs and minibatches"), ({"clip_eps": 0.0}, "clip_eps"), ({"clip_eps": -0.1}, "clip_eps"),
                      ({"clip_eps": float("inf")}, "clip_eps"), ({"clip_eps": float("nan")}, "clip_eps"),
                      ({"value_coeff": -1.0}, "value_coeff"), ({"entropy_coeff": float("inf")}, "entropy_coeff")]:
        with pytest.raises(ValueError, match=match):
            PPOLearner(None, **kw)                             # (the policy is not even looked at)
    lrn = PPOLearner(_net(), clip_eps=1e30)                    # a huge finite clip range is admitted
    assert isinstance(lrn, A2CLearner) and lrn._ws is None and lrn.u == 0
    assert (lrn.clip_eps, lrn.value_coeff, lrn.entropy_coeff, lrn.epochs, lrn.minibatches, lrn.normalize_advantage) == (1e30, 0.5, 0.01, 4, 4, True)
    assert set(lrn.statistics) == {"actor_loss", "critic_loss", "entropy_loss", "ac_loss", "samples", "clip_fraction", "approx_kl"}
    assert lrn.optimizer_state()["ppo"] == {"u": 0}
    with pytest.raises(ValueError, match="fused=True is compiled"):
        PPOLearner(_net(100, 50), fused=True)


def test_trainer_refusals_come_before_any_allocation_and_the_default_is_a2c():
    from azul_deep_reinforcement_learning_amd.training import BatchedTrainer
    sig = inspect.signature(BatchedTrainer.__init__).parameters
    assert sig["algorithm"].default == "a2c"
    assert [(k, sig[k].default) for k in ("clip_eps", "value_coeff", "entropy_coeff", "epochs", "minibatches", "normalize_advantage")] == [
        ("clip_eps", 0.2), ("value_coeff", 0.5), ("entropy_coeff", 0.01), ("epochs", 4), ("minibatches", 4), ("normalize_advantage", True)]
    refusals = [
        ({"algorithm": "trpo"}, "algorithm must be"),
        ({"algorithm": "PPO", "ring": 1}, "algorithm must be"),
        ({"algorithm": "ppo"}, "ring=1"),                                                   # the trainer's default ring of three windows
        ({"algorithm": "ppo", "ring": 2}, "ring=1"),
        ({"algorithm": "ppo", "ring": 1, "opponent": None}, "opponent other than None"),
        ({"algorithm": "ppo", "ring": 1, "epochs": 0}, "epochs and minibatches"),
        ({"algorithm": "ppo", "ring": 1, "minibatches": 0}, "epochs and minibatches"),
        ({"algorithm": "ppo", "ring": 1, "clip_eps": 0.0}, "clip_eps"),
    ]
    for kw, match in refusals:
        with pytest.raises(ValueError, match=match):
            BatchedTrainer(_net(), n_games=8, window=8, **kw)
    with pytest.raises(ValueError, match="ring=1"):
        BatchedTrainer(_net(188), n_games=8, window=8, players=3, fused_wide=True, fused_learner=True, ring=3, algorithm="ppo")
