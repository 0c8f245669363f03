"""PolicyRollout's mode checks against a recording, without a device: tests/golden/rollout_modes.json holds, for a grid of constructor
arguments (four record families x two policies x seven opponents x every setting of the seven switches x rings / parts x trace / move limit /
selection), what _check_modes made of each case before the modes were resolved in one place -- the attributes of an admitted case, or the
refusal's type and message (tools/record_rollout_modes.py).  Every case must come out as recorded, byte for byte; and `window_entry`, which
the recording predates, must name the C entry that the (wide, opponent) pair's window kernel is."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_rollout_modes as rec                          # noqa: E402

# (wide batch, opponent) -> the entry that plays its window in one launch when the modes ask for one
WINDOW_ENTRIES = {
    (False, None): "azul_batch_policy_rollout_returns", (False, "random"): "azul_batch_policy_rollout_returns",
    (False, "net"): "azul_batch_policy_rollout_vs", (False, "greedy"): "azul_batch_policy_rollout_greedy",
    (True, None): "azul_batch_mp_policy_rollout", (True, "random"): "azul_batch_mp_policy_rollout",
    (True, "net"): "azul_batch_mp_policy_rollout_vs", (True, "greedy_margin"): "azul_batch_mp_policy_rollout_greedy",
}


def _recording():
    with open(os.path.join(ROOT, "tests", "golden", "rollout_modes.json")) as fh:
        return json.load(fh)


def test_every_case_of_the_grid_resolves_or_refuses_as_recorded():
    golden = _recording()
    outcomes, index, grid = golden["outcomes"], golden["index"], golden["grid"]
    # the recording itself: the coverage it was made with
    assert len(outcomes) >= 129 and sum(o.startswith("ok ") for o in outcomes) >= 103 and len(set(outcomes)) == len(outcomes)
    assert sorted(set(index)) == list(range(len(outcomes)))
    n, wrong = 0, []
    for n, (case, want) in enumerate(zip(rec.cases(grid), index), 1):
        got = rec.outcome(grid, case)
        if got != outcomes[want]:
            wrong.append((case, outcomes[want], got))
    assert n == len(index) == sum(1 for _ in rec.cases(grid))
    assert not wrong, "%d of %d cases differ; the first: %r\nrecorded: %s\nnow:      %s" % ((len(wrong), n) + wrong[0])


def test_window_entry_names_the_kernel_of_every_admitted_window_configuration():
    from azul_deep_reinforcement_learning_amd import _lib as L
    golden = _recording()
    grid = golden["grid"]
    seen, admitted = set(), 0
    for case in rec.cases(grid):
        try:
            ro, _ = rec.check_modes(grid, case)
        except (ValueError, AssertionError):
            continue
        admitted += 1
        # one launch per window: exactly what `persistent` (two-player) and `fused_wide` (wide) say, as the launch code read them before
        one_launch = ro.persistent or ro.fused_wide
        assert (ro.window_entry is not None) == one_launch, case
        if one_launch:
            assert ro.window_entry == WINDOW_ENTRIES[ro.wide, ro.opponent], case
            assert ro.window_entry in L.SIGNATURES
            seen.add((ro.wide, ro.opponent))
    assert admitted == sum(golden["outcomes"][i].startswith("ok ") for i in golden["index"]) >= 1600
    assert seen == set(WINDOW_ENTRIES)
