"""GPU: azul_policy_head_n, the sampling head for 180 / 240 / 300 actions -- the same bits as azul_policy_head at 180, the masked log-softmax /
entropy of torch f32 at 240 and 300 (the existing head test's tolerance), the first maximum in argmax mode and -1 for a row with no legal
action."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def head_n(logits, mask, seed, counter, na, id_base=0):
    from azul_deep_reinforcement_learning_amd import _lib as L
    n = logits.shape[0]
    out = (torch.full((n,), -9, dtype=torch.int32, device=logits.device), torch.full((n,), 9.0, device=logits.device),
           torch.full((n,), 9.0, device=logits.device))
    L.check(L.lib.azul_policy_head_n(_p(logits), _p(mask), seed, counter, None, n, na, id_base, _p(out[0]), _p(out[1]), _p(out[2]), None))
    return out


def inputs(n, na, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    logits = (torch.randn(n, na, generator=g) * 3).cuda()
    mask = (torch.rand(n, na, generator=g) < 0.3).to(torch.uint8)
    mask[0] = 0                                    # no legal action
    mask[1] = 0
    mask[1, na - 1] = 1                            # only the last action
    return logits, mask.cuda()


@pytest.mark.parametrize("seed", [1234, 0xFFFFFFFFFFFFFFFF])
def test_180_is_azul_policy_head_bit_for_bit(seed):
    from azul_deep_reinforcement_learning_amd import _lib as L
    n = 1027
    logits, mask = inputs(n, 180, 5)
    for counter in (0, 17):
        ref = (torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"))
        L.check(L.lib.azul_policy_head(_p(logits), _p(mask), seed, counter, None, n, 3, _p(ref[0]), _p(ref[1]), _p(ref[2]), None))
        got = head_n(logits, mask, seed, counter, 180, id_base=3)
        for a, b in zip(ref, got):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("na", [240, 300])
def test_240_and_300_match_the_torch_masked_softmax(na):
    n = 2049
    logits, mask = inputs(n, na, na)
    legal = mask.bool()
    ref_logp = torch.log_softmax(logits.masked_fill(~legal, float("-inf")), dim=1)
    ref_ent = -(torch.where(legal, ref_logp, torch.zeros_like(ref_logp)).sum(dim=1) / legal.sum(dim=1).clamp(min=1))
    counts = torch.zeros(n, na, device="cuda")
    for c in range(8):
        a, logp, ent = head_n(logits, mask, 99, c, na)
        assert int(a[0]) == -1 and float(logp[0]) == 0.0 and float(ent[0]) == 0.0
        assert int(a[1]) == na - 1
        keep = a >= 0
        rows = torch.arange(n, device="cuda")[keep]
        assert bool(legal[rows, a[keep].long()].all())
        assert torch.allclose(logp[keep], ref_logp[rows, a[keep].long()], atol=2e-5, rtol=1e-5)
        assert torch.allclose(ent[keep], ref_ent[keep], atol=2e-5, rtol=1e-5)
        counts[rows, a[keep].long()] += 1
    # the draws spread over the legal actions of every part of the row (all 16 lanes' slices are reachable)
    assert bool((counts.sum(dim=0)[(na // 16) * 15:] > 0).any())
    # argmax mode: np.argmax over the masked scores, the first maximum
    a, _, _ = head_n(logits, mask, 0xFFFFFFFFFFFFFFFF, 0, na)
    ties = logits.clone()
    ties[2:, :] = 1.0                              # every action ties: the first legal one wins
    at, _, _ = head_n(ties, mask, 0xFFFFFFFFFFFFFFFF, 0, na)
    ok = legal.any(dim=1)
    first_legal = legal.to(torch.int64).argmax(dim=1)
    assert torch.equal(at[2:][ok[2:]].long(), first_legal[2:][ok[2:]])
    best = logits.masked_fill(~legal, float("-inf")).argmax(dim=1)
    assert torch.equal(a[ok].long(), best[ok]) and int(a[0]) == -1


def test_bad_arguments_are_refused():
    from azul_deep_reinforcement_learning_amd import _lib as L
    logits, mask = inputs(8, 240, 1)
    one = torch.zeros(8, dtype=torch.int32, device="cuda")
    f = torch.zeros(8, device="cuda")
    assert L.lib.azul_policy_head_n(_p(logits), _p(mask), 1, 0, None, 8, 200, 0, _p(one), _p(f), _p(f), None) == L.ERR_INVALID
    assert L.lib.azul_policy_head_n(_p(logits), _p(mask), 1, 0, None, 0, 240, 0, _p(one), _p(f), _p(f), None) == L.ERR_INVALID
