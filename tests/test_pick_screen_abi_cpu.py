"""The screened sampler's boundary without a GPU: where its size query is zero, the new entry's argument validation, and the sampler
workspace it must leave exactly as it was (the literals of tests/test_sampler_workspace_sizes_cpu.py)."""
import ctypes
import json
import os
import subprocess
import sys

import s2vt_amd
from s2vt_amd import _lib

import test_sampler_workspace_sizes_cpu as base

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = """
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import s2vt_amd
from s2vt_amd import _lib
L = s2vt_amd.lib()
d = ctypes.byref(_lib.Dims(32, 300, 16, 136, 2, 6, 0, 0))
print(json.dumps([L.s2vt_sample_screen_workspace_bytes(d, 13, 4, 1), L.s2vt_sample_workspace_bytes(d, 13, 4, 1)]))
"""


def _pad(n, m):
    return (n + m - 1) // m * m


def test_size_query():
    L = s2vt_amd.lib()
    q = L.s2vt_sample_screen_workspace_bytes

    def dims(D=32, V=300, E=16, H=136, Tv=2, Tc=6, res=0):
        return ctypes.byref(_lib.Dims(D, V, E, H, Tv, Tc, 0, res))

    if os.environ.get("S2VT_PICK_SCREEN", "1")[:1] != "0":
        # head block, two planes of W^T [V][pad64(H)], W^T in fp32 [V][pad4(H)], two planes of the rows [R][pad64(H)], logits [R][pad4(V)],
        # each up to 256 bytes
        want = 256 + 2 * _pad(300 * 192 * 2, 256) + _pad(300 * 136 * 4, 256) + 2 * _pad(65 * 192 * 2, 256) + _pad(65 * 300 * 4, 256)
        assert q(dims(), 13, 4, 1) == want
        assert q(dims(), 65, 0, 1) > 0
        big = q(dims(1536, 12000, 500, 1000, 5, 20), 64, 5, 1)
        assert 110e6 < big < 125e6 and big % 256 == 0
    assert q(dims(), 16, 3, 1) == 0 and q(dims(), 16, 4, 0) == 0 and q(dims(), 1, 0, 1) == 0      # <= 64 rows
    assert q(None, 13, 4, 1) == 0 and q(dims(), 0, 4, 1) == 0 and q(dims(), 13, -1, 1) == 0
    assert q(dims(V=0), 13, 4, 1) == 0 and q(dims(H=0), 13, 4, 1) == 0
    assert q(dims(H=2052), 13, 4, 1) == 0                        # a row of h no longer fits the resolve kernel's LDS
    assert q(dims(res=_lib.MODEL_RESIDUAL), 13, 4, 1) == 0       # the residual sampler keeps the fp32 pick


def test_switch_turns_the_path_off_and_leaves_the_sampler_workspace():
    out = {}
    for v in ("0", "1"):
        env = {k: x for k, x in os.environ.items() if k not in ("S2VT_DECLOOP", "S2VT_DEC4")}
        env["S2VT_PICK_SCREEN"] = v
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[v] = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["0"][0] == 0 and out["1"][0] > 0
    assert out["0"][1] == out["1"][1] > 0


def test_sampler_workspace_bytes_are_unchanged():
    env = {k: v for k, v in os.environ.items() if k not in ("S2VT_DECLOOP", "S2VT_DEC4")}
    r = subprocess.run([sys.executable, "-c", base._CHILD, ROOT, json.dumps([c[0] for c in base.CASES])], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert [tuple(x) for x in got["sizes"]] == [c[1] for c in base.CASES]


def test_screened_entry_validates_arguments():
    L = s2vt_amd.lib()
    if L.s2vt_sample_screen_workspace_bytes(ctypes.byref(_lib.Dims(32, 300, 16, 136, 2, 6, 0, 0)), 13, 4, 1) == 0:
        return                                                   # switched off in this environment: every call is a bad argument
    P = ctypes.c_void_p(4096)                                   # never dereferenced: validation happens before any launch
    d = _lib.Dims(32, 300, 16, 136, 2, 6, 0, 0)
    dp = ctypes.byref(d)
    pp = ctypes.byref(_lib.Params(*([4096] * 9 + [None, None])))
    no_b = ctypes.byref(_lib.Params(*([4096] * 8 + [None, None, None])))
    nb = L.s2vt_sample_workspace_bytes(dp, 13, 4, 1)
    sb = L.s2vt_sample_screen_workspace_bytes(dp, 13, 4, 1)

    def f(dims=dp, prm=pp, video=P, B=13, K=4, G=1, ids=P, ws=P, nbytes=nb, sws=P, sbytes=sb):
        return L.s2vt_sample_screened(dims, prm, video, B, K, G, 7, 0, ids, ws, nbytes, sws, sbytes, None)

    assert f(prm=None) == -1 and f(video=None) == -1 and f(ids=None) == -1 and f(ws=None) == -1 and f(sws=None) == -1
    assert f(dims=None) == -1 and f(prm=no_b) == -1
    assert f(B=0) == -1 and f(K=-1) == -1
    assert f(K=3) == -1                                          # 52 rows: not a call this path serves
    assert f(dims=ctypes.byref(_lib.Dims(32, 300, 16, 136, 2, 6, 0, _lib.MODEL_RESIDUAL))) == -1
    assert f(ws=ctypes.c_void_p(4096 + 16)) == -2 and f(sws=ctypes.c_void_p(4096 + 128)) == -2
    assert f(nbytes=nb - 256) == -3 and f(sbytes=sb - 256) == -3
