"""The screened sampler with the pick screen's product forced onto the 192 x 96 tile (S2VT_PICK_TILE=1, read once: a fresh child
process).  At the small shapes of tests/test_gpu_pick_screen.py the tile rule would keep 128 x 128, so the knob is what puts the new tile
under the whole decode loop here: sampled and greedy ids equal s2vt_sample's and the oracle's, the survivor counters sit where they sit
with the other tile, and the launch profiler names the tile that ran."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = """
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import torch
import s2vt_amd
from s2vt_amd import ops
from oracle import s2vt_oracle as oracle
import test_gpu_pick_screen as T
oracle.lib()
out = []
for dims, B, K, seed in ((T.SMALL, 65, 2, 3), (T.SMALL, 13, 4, 7)):          # the R195 and R65 cases
    d, p, video = T._case(oracle, dims, B)
    s = T._Sampler(ops, d, p, video, B, K)
    ops.prof_enable(True)
    got_s, got_g = s.screened(seed)
    rows = ops.prof_collect()
    ops.prof_enable(False)
    total, most, every = s.counters()
    ref_s, ref_g = s.plain(seed)
    orc_s, orc_g = oracle.sample_captions(p, d, video, K=K, seed=seed, video_base=0)
    out.append(dict(R=s.rows, Tc=s.Tc, total=total, most=most, every=every,
                    plain=bool(np.array_equal(got_s, ref_s) and np.array_equal(got_g, ref_g)),
                    oracle=bool(np.array_equal(got_s, orc_s) and np.array_equal(got_g, orc_g)),
                    screen=[(r["name"], r["launches"]) for r in rows if "pick screen" in r["name"]]))
print(json.dumps(out))
"""


def test_sampler_on_the_forced_tile(gpu):
    env = dict(os.environ, S2VT_PICK_TILE="1")
    env.pop("S2VT_PICK_SCREEN", None)
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    cases = json.loads(p.stdout.strip().splitlines()[-1])
    assert [c["R"] for c in cases] == [195, 65]
    for c in cases:
        print(c)
        assert c["plain"], "ids differ from s2vt_sample's"
        assert c["oracle"], "ids differ from the oracle's"
        mean = c["total"] / (c["R"] * c["Tc"])
        assert 1.0 <= mean <= 8.0 and c["every"] == 0
        assert c["screen"] == [["x3_192x96(dma) pick screen", c["Tc"]]], "the forced tile did not run every step's product"
