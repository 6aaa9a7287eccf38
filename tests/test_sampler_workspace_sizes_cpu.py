"""The S2VT sampler's and beam search's workspaces and entry-point validation, pinned without a GPU.

s2vt_sample_workspace_bytes and s2vt_beam_workspace_bytes share the encode half's eight leading regions (csrc/api.hip:
carve_sample_enc inside carve_sample and carve_beam); train.hip and session.hip find the sampler's LSTM1 history by carving again, so
neither the order nor any region's size may move.  The sample size also depends on S2VT_DECLOOP / S2VT_DEC4, which the library reads
once per process: the sizes are queried in a child process (CPU only) whose environment has neither.

The expected byte counts and return codes are what the library built at commit a1038e6 returns (the parent of the change that
introduced SampleEnc and merged the twin entry points), written down as literals."""
import ctypes
import json
import os
import subprocess
import sys

import s2vt_amd
from s2vt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# dims (D, V, E, H, Tv, Tc), B, K, with_greedy, beam -> bytes of (sample workspace, beam workspace)
CASES = [
    (((16, 11, 3, 4, 2, 3), 4, 2, 1, 3), (406528, 402176)),
    (((32, 132, 16, 132, 2, 8), 16, 2, 1, 3), (5305344, 4357376)),               # R = 48, H = 132: decode-loop operands carved
    (((32, 132, 16, 128, 2, 8), 16, 2, 1, 3), (1495808, 1569024)),               # H < 132: not carved
    (((32, 132, 16, 132, 2, 8), 16, 4, 0, 16), (5355520, 5346560)),              # R = 64, the widest beam
    (((32, 132, 16, 132, 2, 8), 13, 4, 1, 5), (4153344, 4256512)),               # R = 65
    (((64, 300, 24, 136, 5, 6), 64, 5, 1, 5), (9329664, 9969152)),               # R = 384: not carved by default
    (((24, 37, 5, 12, 33, 5), 5, 0, 1, 1), (544000, 541184)),
    (((256, 2000, 300, 992, 5, 8), 16, 2, 1, 3), (39771648, 15563008)),
    (((256, 2000, 300, 992, 5, 8), 16, 4, 1, 3), (15009536, 15563008)),          # R = 80
    (((1536, 12000, 500, 1000, 5, 20), 64, 0, 1, 5), (127553280, 102092288)),
]

_CHILD = """
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import s2vt_amd
from s2vt_amd import _lib
L = s2vt_amd.lib()
out = []
for (D, V, E, H, Tv, Tc), B, K, G, beam in json.loads(sys.argv[2]):
    d = ctypes.byref(_lib.Dims(D, V, E, H, Tv, Tc, 0, 0))
    out.append([L.s2vt_sample_workspace_bytes(d, B, K, G), L.s2vt_beam_workspace_bytes(d, B, beam)])
d = ctypes.byref(_lib.Dims(16, 11, 3, 4, 2, 3, 0, 0))
bad = [L.s2vt_sample_workspace_bytes(None, 4, 2, 1), L.s2vt_sample_workspace_bytes(d, 0, 2, 1), L.s2vt_sample_workspace_bytes(d, 4, -1, 1),
       L.s2vt_sample_workspace_bytes(d, 4, 0, 0)]
print(json.dumps({"sizes": out, "bad": bad}))
"""


def test_workspace_bytes_are_those_of_the_parent():
    env = {k: v for k, v in os.environ.items() if k not in ("S2VT_DECLOOP", "S2VT_DEC4")}
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps([c[0] for c in CASES])], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert [tuple(x) for x in got["sizes"]] == [c[1] for c in CASES]
    assert all(n % 256 == 0 for x in got["sizes"] for n in x)
    # bad shapes size to zero; the size query does not reject "no rows" (K = 0 without the greedy block)
    assert got["bad"] == [0, 0, 0, 399616]


def test_sample_entry_points_validate_arguments():
    L = s2vt_amd.lib()
    P = ctypes.c_void_p(4096)                                   # never dereferenced: validation happens before any launch
    d = _lib.Dims(16, 11, 3, 4, 2, 3, 0, 0)
    dp = ctypes.byref(d)
    pp = ctypes.byref(_lib.Params(*([4096] * 9 + [None, None])))
    no_b = ctypes.byref(_lib.Params(*([4096] * 8 + [None, None, None])))     # embed_word_b missing
    nb = 406528

    def sample(dims=dp, prm=pp, video=P, B=4, K=2, G=1, ids=P, ws=P, nbytes=nb):
        return L.s2vt_sample(dims, prm, video, B, K, G, 7, 0, ids, ws, nbytes, None)

    def sample_ex(dims=dp, prm=pp, video=P, B=4, K=2, G=1, ids=P, ws=P, nbytes=nb, flags=0):
        return L.s2vt_sample_ex(dims, prm, video, B, K, G, 7, 0, flags, ids, ws, nbytes, None)

    for f in (sample, sample_ex):
        assert f(prm=None) == -1 and f(video=None) == -1 and f(ids=None) == -1 and f(ws=None) == -1
        assert f(B=0) == -1
        assert f(K=-1) == -1
        assert f(K=0, G=0) == -1                                # no rows
        assert f(dims=None) == -1
        assert f(prm=no_b) == -1
        assert f(ws=ctypes.c_void_p(4096 + 16)) == -2
        assert f(nbytes=nb - 256) == -3                         # workspace too small
    assert sample_ex(flags=2) == -1 and sample_ex(flags=3) == -1


def test_gemm_entry_points_validate_arguments():
    L = s2vt_amd.lib()
    P = ctypes.c_void_p(4096)                                   # never dereferenced: validation happens before any launch
    seg = ctypes.pointer(_lib.Operand(4096, None, 8, 8, 0, 0))  # one segment: k = 8, ld = 8

    for name in ("s2vt_gemm", "s2vt_gemm_nt"):
        def gemm(segs=seg, nseg=1, W=P, ldw=16, Cinit=None, ldcinit=0, C=P, ldc=16, M=4, N=16):
            return getattr(L, name)(segs, nseg, W, ldw, None, Cinit, ldcinit, C, ldc, M, N, 0, -1, None)
        assert gemm(segs=None) == -1
        assert gemm(nseg=0) == -1 and gemm(nseg=4) == -1
        assert gemm(W=None) == -1
        assert gemm(C=None) == -1
        assert gemm(M=-1) == -1
        assert gemm(N=0) == -1
        assert gemm(ldc=15) == -1
        assert gemm(Cinit=P, ldcinit=15) == -1
        assert gemm(M=0) == 0                                   # no rows: nothing to do
        if name == "s2vt_gemm":
            assert gemm(ldw=15) == -1                           # ldw < N
        else:
            assert gemm(ldw=7) == -1                            # ldw < K
