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
