"""CPU: the host side of the wide fused learner -- compiled shapes, flat layouts and the refusals of the opt-in keywords
(A2CLearner(fused=True), PolicyRollout(wide_ring=k), BatchedTrainer(fused_learner=True)).  Nothing here touches a GPU."""
import pytest
import torch

from azul_deep_reinforcement_learning_amd import _lib as L
from azul_deep_reinforcement_learning_amd.learner import A2CLearner, REFERENCE_SHAPE, WIDE_SHAPES, flat_layout
from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic

P3 = {"first_player": "Random", "tile_pool": "Lid"}


@pytest.mark.parametrize("shape", (REFERENCE_SHAPE,) + WIDE_SHAPES)
def test_flat_size_of_every_compiled_shape(shape):
    IN, H, A = shape
    n = L.lib.azul_a2c_flat_size(IN, H, A)
    params = sum(p.numel() for p in BatchedActorCritic(IN, A, H).parameters())
    assert n == params + 1 == flat_layout(*shape)["size"]
    lay = flat_layout(*shape)
    assert lay["w2a_t"][0] % 2 == 0                      # the pad keeps dw2a_t 8-byte aligned
    assert lay["b2a"][0] + A == n


def test_reference_flat_size_is_unchanged():
    assert L.lib.azul_a2c_flat_size(136, 180, 180) == L.A2C_FLAT_SIZE


@pytest.mark.parametrize("shape", [(136, 180, 181), (188, 128, 180), (188, 180, 240), (100, 180, 180), (260, 180, 240)])
def test_shapes_that_are_not_compiled_are_refused(shape):
    assert L.lib.azul_a2c_flat_size(*shape) == L.ERR_INVALID
    args = [None] * 4 + [1e-3, 0.9, 0.999, 1e-8, 1] + list(shape) + [None] * 8 + [None, None, 0.0, None, None]
    assert L.lib.azul_a2c_apply_adam_n(*args) == L.ERR_INVALID


def test_fused_learner_refuses_a_shape_without_kernel():
    with pytest.raises(ValueError, match="compiled for"):
        A2CLearner(BatchedActorCritic(188, 180, 128), fused=True)
    A2CLearner(BatchedActorCritic(188, 180, 128))                 # default: PyTorch path, no refusal
    A2CLearner(BatchedActorCritic(188, 180, 180), fused=True)


def test_wide_ring_needs_the_fused_window_kernel_and_one_part():
    from azul_deep_reinforcement_learning_amd.rollout import PolicyRollout
    net = BatchedActorCritic(188, 180, 180)
    with pytest.raises(ValueError, match="wide_ring"):
        PolicyRollout(net, n_games=64, players=3, rules=P3, opponent="random", wide_ring=2)
    with pytest.raises(ValueError, match="wide_ring"):
        PolicyRollout(net, n_games=64, parts=2, players=3, rules=P3, opponent="random", fused_wide=True, wide_ring=2)
    with pytest.raises(ValueError, match="wide_ring"):
        PolicyRollout(net, n_games=64, players=3, rules=P3, opponent="random", fused_wide=True, wide_ring=0)


WIDE_BATCHES = [(3, P3, 188, 180), (4, P3, 240, 180), (3, dict(P3, displays="2P+1"), 198, 240), (4, dict(P3, displays="2P+1", bonuses="end"), 260, 300),
                (2, dict(P3, short_deal=True), 136, 180)]


@pytest.mark.parametrize("players,rules,n_obs,n_act", WIDE_BATCHES)
def test_batch_shape_is_the_librarys_formula(players, rules, n_obs, n_act):
    from azul_deep_reinforcement_learning_amd.batch import batch_shape
    assert batch_shape(players, rules) == (n_obs, n_act)


def test_reference_batch_shape():
    from azul_deep_reinforcement_learning_amd.batch import batch_shape
    assert batch_shape(2, P3) == (L.OBS_SIZE, L.NUM_ACTIONS)


@pytest.mark.parametrize("players,rules,n_obs,n_act", WIDE_BATCHES[:4:3])
def test_rollout_mode_refusals_need_no_gpu(players, rules, n_obs, n_act):
    """Every ValueError of PolicyRollout's mode checks is raised before a device is touched: the refusals the GPU suite asserts
    (test_fused_wide_refusals, test_fused_opponent_refusals, test_wrong_shapes_and_two_player_batches_are_refused), with CPU modules."""
    from azul_deep_reinforcement_learning_amd.rollout import PolicyRollout
    kw = dict(n_games=16, rules=rules, players=players)
    pol, opp = BatchedActorCritic(n_obs, n_act, 180), BatchedActorCritic(n_obs, n_act, 180)
    # a network opponent that does not take the batch's observation or give its actions (any hidden size is fine)
    for bad in (BatchedActorCritic(n_obs, n_act + 60, 32), BatchedActorCritic(n_obs + 52, n_act, 32)):
        with pytest.raises(ValueError, match="ActorCritic\\(%d, %d" % (n_obs, n_act)):
            PolicyRollout(BatchedActorCritic(n_obs, n_act, 32), window=4, opponent=bad, **kw)
    with pytest.raises(ValueError, match="move limit"):
        PolicyRollout(pol, opponent="random", move_limit=100, **kw)
    # fused_wide: wide batches, opponent None / "random" (or fused_opponent), the library's head, hidden 180 on the batch's shape
    with pytest.raises(ValueError, match="fused_wide"):
        PolicyRollout(BatchedActorCritic(), n_games=16, players=2, fused_wide=True)
    with pytest.raises(ValueError, match="fused_wide"):
        PolicyRollout(pol, opponent=opp, fused_wide=True, **kw)
    with pytest.raises(ValueError, match="fused_head"):
        PolicyRollout(pol, fused_head=False, fused_wide=True, **kw)
    for bad in (BatchedActorCritic(n_obs, n_act, 64), BatchedActorCritic(n_obs, n_act + 60, 180), BatchedActorCritic(n_obs + 52, n_act, 180)):
        with pytest.raises(ValueError, match="compiled for ActorCritic\\(%d, %d, hidden 180\\)" % (n_obs, n_act)):
            PolicyRollout(bad, fused_wide=True, **kw)
    # fused_opponent: fused_wide and a module of hidden 180
    with pytest.raises(ValueError, match="per-cut"):
        PolicyRollout(pol, opponent=BatchedActorCritic(n_obs, n_act, 64), fused_wide=True, fused_opponent=True, **kw)
    with pytest.raises(ValueError, match="fused_opponent"):
        PolicyRollout(pol, opponent=opp, fused_opponent=True, **kw)
    for o in (None, "random"):
        with pytest.raises(ValueError, match="fused_opponent"):
            PolicyRollout(pol, opponent=o, fused_wide=True, fused_opponent=True, **kw)
    # the opponent's shape is checked before the fused modes
    with pytest.raises(ValueError, match="network opponent"):
        PolicyRollout(pol, opponent=BatchedActorCritic(n_obs, n_act + 60, 180), fused_wide=True, fused_opponent=True, **kw)


def test_fused_learner_needs_fused_wide():
    from azul_deep_reinforcement_learning_amd.training import BatchedTrainer
    with pytest.raises(ValueError, match="fused_wide"):
        BatchedTrainer(BatchedActorCritic(188, 180, 180), n_games=64, players=3, rules=P3, fused_learner=True)


def test_learner_views_follow_the_shape():
    net = BatchedActorCritic(198, 240, 180)
    lr = A2CLearner(net, fused=True)
    flat = torch.arange(flat_layout(198, 180, 240)["size"], dtype=torch.float32)
    v = lr._views(flat)
    assert v["w1t"].shape == (198, 360) and v["w2a_t"].shape == (180, 240) and v["b2a"].numel() == 240
    assert int(v["b2a"][-1]) == flat.numel() - 1 and int(v["w2a_t"][0, 0]) == int(v["b2c"][0]) + 2
