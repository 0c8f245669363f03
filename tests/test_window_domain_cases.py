"""The conditions of tests/window_domain_cases.py on the model alone, before a kernel runs: every record comes back from its model slot byte
for byte, the `ended` records are what their names say, and the census holds per config -- every required class per case (config, opp),
every class of the issue's list per config over its two cases, with no game left out -- whatever the policy answers (eight seeded random
answer policies; the kernels' own answers are booked again in the emulation and GPU tests)."""
import numpy as np
import pytest

from oracle import oracle as oz
from tests import domain_records as dr
from tests import window_domain_cases as wd

CPU = [(cfg, wd.CPU_N, wd.CPU_ENDED, wd.CPU_T) for cfg in dr.TWO_CONFIGS + wd.CPU_WIDE]
GPU = [(cfg, wd.GPU_N, wd.GPU_ENDED, wd.GPU_T * wd.GPU_WINDOWS) for cfg in dr.TWO_CONFIGS + wd.GPU_WIDE]
_ids = lambda where, cases: ["%s-%s" % (where, dr.config_id(c[0])) for c in cases]


@pytest.mark.parametrize("cfg,n,n_ended,T", CPU + GPU, ids=_ids("cpu", CPU) + _ids("gpu", GPU))
def test_census_holds_for_every_answer_policy_and_no_game_is_left_out(cfg, n, n_ended, T):
    raw = wd.records(cfg, n, n_ended)
    assert len(raw) == n + n_ended and (dr.tiles_in_play(_structured(cfg, raw), cfg[0]) <= dr.CLOSURE).all()
    for policy in range(8):
        union = wd.new_census()
        for opp in (0, 1):
            census = wd.model_census(cfg, opp, raw, T, seed=policy)
            wd.assert_census(census, cfg, opp, (dr.config_id(cfg), opp, policy))
            for k, v in census.items():
                union[k] += v
        missing = [c for c in wd.CLASSES if union[c] == 0 and not (c == "box_empty" and c in dr.unreachable(cfg))]
        assert not missing, (dr.config_id(cfg), policy, missing, union)


def _structured(cfg, raw):
    return np.ascontiguousarray(raw).view(oz.RECORD_DTYPE if wd.is_two(cfg) else oz.RECORD_NP_DTYPE).reshape(-1)


@pytest.mark.parametrize("cfg", dr.TWO_CONFIGS + [wd.CPU_WIDE[0], wd.CPU_WIDE[3]], ids=dr.config_id)
def test_the_ended_records_are_what_they_are_called(cfg):
    P, ext, pool = cfg
    n = 9
    recs = dr.ended(n, P, dr.displays(cfg), 5, not wd.is_two(cfg))
    for i, r in enumerate(recs):
        g = dr.Game(r, cfg)
        assert g.pack().tobytes() == r.tobytes(), i
        flag = (int(r["flags"]) >> 6) & 1
        if i < 3:
            assert flag == 1 and g.g.end_of_game
        elif i < 6:
            assert flag == 0 and not g.mask().any() and g.flags() & 1            # nothing legal; the round is over
        else:
            assert flag == 0 and g.flags() & 2 and not g.g.end_of_game           # the walls say "over", the flag does not
