"""The self-play kernels' loop nest (blocks of moves between two priority changes, csrc/azul_selfplay_kernels.hpp) and the diagnostic build.

* Two launches of 256 moves give what one launch of 512 gives -- every stream of the trajectory, the final records, the MT19937 words and
  positions and the counters -- for 1, 2, 3 games (an odd batch's last wave plays one game) and for the benchmarked 4096, two players and the
  wide record (three players).  512 and 256 are both several blocks long, and the priority a wave holds in a block depends on where the
  hardware put it: nothing of that may show in what is computed.
* The diagnostic build (-DAZ_PROFILE_SEGMENTS: segment stamps, per-wave record, tools/wave_timeline.py) computes what the product build computes.
  Each library runs in a child process of its own; the digests of everything the launch wrote are compared.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("mask", "action", "reward", "done", "packed")


def _play(n, chunks, players=2):
    import torch
    from azul_deep_reinforcement_learning_amd import BatchedAzul
    env = BatchedAzul(n) if players == 2 else BatchedAzul(n, players=players)
    env.seed(4242)
    if players == 2:
        env.runner_init()
        env.runner_init()
    else:
        env.init()
        env.new_round()
    pitch = 192 if players == 2 else {5: 192, 7: 256, 9: 320}[env.displays]
    out = {k: [] for k in KEYS}
    for T in chunks:
        t = env.alloc_trajectory(T, packed_mask=True, mask_pitch=pitch, mask_bits=False)
        env.selfplay(T, t["mask"], t["action"], t["reward"], t["done"], packed=t["packed"])
        torch.cuda.synchronize()
        for k in KEYS:
            out[k].append(t[k].cpu().numpy())
    res = {k: np.concatenate(v, axis=0) for k, v in out.items()}
    res["records"] = np.frombuffer(env.get_records().tobytes(), np.uint8)
    mt, pos = env.get_rng_range()
    res["mt"], res["pos"] = np.asarray(mt), np.asarray(pos)
    cnt = env.counters()
    for k in ("episodes", "stuck", "stat_sums"):
        res["cnt_" + k] = np.asarray(cnt[k])
    return res


@pytest.mark.parametrize("players", [2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 4096])
def test_two_launches_of_256_moves_equal_one_of_512(n, players):
    one = _play(n, [512], players)
    two = _play(n, [256, 256], players)
    assert sorted(one) == sorted(two)
    for k in one:
        assert one[k].shape == two[k].shape and one[k].tobytes() == two[k].tobytes(), k
    assert int((one["done"] != 0).sum()) > 0          # episodes ended and were reset inside the window


_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, %(root)r)
import azul_deep_reinforcement_learning_amd._lib as L
if %(lib)r:
    L.LIB_PATH = %(lib)r
    L.lib = L._load()
from tests.test_gpu_launch_tail import _play
out = {}
for n in (3, 4096):
    r = _play(n, [512, 512])
    out[str(n)] = {k: hashlib.sha256(v.tobytes()).hexdigest() for k, v in r.items()}
print("DIGESTS " + json.dumps(out, sort_keys=True))
"""


def _digests(lib):
    p = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "lib": lib}], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [x for x in p.stdout.splitlines() if x.startswith("DIGESTS ")][-1]
    return json.loads(line[len("DIGESTS "):])


def test_the_diagnostic_build_computes_what_the_product_build_computes():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    lib = os.path.join(ge.PKG, "libazulhip_prof.so")
    srcs = [os.path.join(ge.CSRC, f) for f in sorted(os.listdir(ge.CSRC))] + [os.path.join(ROOT, "include", "azul_hip.h")]
    if ge._stale(lib, srcs):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + ge.HIPCC_FLAGS + ["-DAZ_PROFILE_SEGMENTS", "-I", os.path.join(ROOT, "include"),
                               "-o", lib, os.path.join(ge.CSRC, "azul_kernels.hip")], cwd=ge.CSRC)
    product, diagnostic = _digests(""), _digests(lib)
    assert product == diagnostic
    assert len(product["4096"]) >= 10
