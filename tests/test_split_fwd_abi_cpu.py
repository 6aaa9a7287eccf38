"""The split forward's boundary without a GPU: the new symbols are declared in include/s2vt.h and bound in _lib.py with the header's
parameter lists, the split workspace's size is what it was, the entries validate their arguments before any launch, and
S2VT_SPLIT_FWD is parsed as documented (a fresh process per setting: the env is read once)."""
import ctypes as C
import os
import re
import subprocess
import sys

import s2vt_amd
from s2vt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("s2vt_gemm_bf16x3_nn", "s2vt_teacher_forced_fwd_split", "s2vt_split_fwd_stage", "s2vt_split_fwd_active")

# header type -> the ctypes class _lib.py must bind it to
_CTYPE = {"int32_t": C.c_int32, "int": C.c_int, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "float": C.c_float, "s2vt_stream": C.c_void_p}


def _header_params(name):
    src = open(os.path.join(ROOT, "include", "s2vt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/s2vt.h"
    args = [a.strip() for a in m.group(2).split(",")]
    if args == ["void"]:
        args = []
    return m.group(1), args


def _expected(arg):
    if "*" in arg:
        if "s2vt_dims" in arg:
            return C.POINTER(_lib.Dims)
        if "s2vt_params" in arg:
            return C.POINTER(_lib.Params)
        return C.c_void_p
    return _CTYPE[arg.split()[-2] if len(arg.split()) > 1 else arg]


def test_new_symbols_are_declared_and_bound_with_the_headers_signatures():
    L = s2vt_amd.lib()
    for name in NEW:
        ret, args = _header_params(name)
        assert ret == "int" and name in _lib.SIGNATURES and hasattr(L, name)
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int
        assert len(argtypes) == len(args), (name, len(argtypes), len(args))
        for a, t in zip(args, argtypes):
            assert t is _expected(a), (name, a, t)
    # the sibling entries: the live forward's list plus (split_ws, bytes) ahead of the stream; the TN product's list
    live = _lib.SIGNATURES["s2vt_teacher_forced_fwd_live"][1]
    assert _lib.SIGNATURES["s2vt_teacher_forced_fwd_split"][1] == live[:-1] + [C.c_void_p, C.c_size_t] + live[-1:]
    assert _lib.SIGNATURES["s2vt_gemm_bf16x3_nn"][1] == _lib.SIGNATURES["s2vt_gemm_bf16x3_tn"][1]


def test_split_workspace_bytes_are_unchanged():
    """s2vt_split_grad_workspace_bytes at the bench shape and at the two shapes of tests/test_gpu_split_fwd.py: the values of the library
    before the forward used this workspace."""
    L = s2vt_amd.lib()
    q = lambda dims, B, N: L.s2vt_split_grad_workspace_bytes(C.byref(_lib.Dims(*dims, 0, 0)), B, N)
    assert q((1536, 12000, 500, 1000, 5, 20), 64, 320) == WANT_BENCH
    assert q((128, 300, 40, 136, 2, 3), 64, 320) == WANT_A
    assert q((128, 1100, 500, 264, 2, 3), 33, 264) == WANT_B


WANT_BENCH, WANT_A, WANT_B = 713315328, 9407232, 24792064


def test_entries_validate_arguments():
    L = s2vt_amd.lib()
    P = C.c_void_p(4096)                                        # never dereferenced: validation happens before any launch
    nn = lambda **kw: L.s2vt_gemm_bf16x3_nn(*[kw.get(k, v) for k, v in (("Ah", P), ("Al", P), ("lda", 64), ("Bh", P), ("Bl", P), ("ldb", 64), ("C", P),
                                                                      ("ldc", 64), ("M", 8), ("N", 64), ("K", 64), ("acc", 0), ("bias", None),
                                                                      ("scratch", None), ("sbytes", 0), ("stream", None))])
    assert nn(Ah=None) == -1 and nn(Bl=None) == -1 and nn(C=None) == -1
    assert nn(lda=32) == -1 and nn(lda=68) == -1 and nn(ldb=56) == -1 and nn(ldc=63) == -1          # lda >= bf16_pad(K), % 8; ldb, ldc >= N
    assert nn(K=65, lda=64) == -1 and nn(acc=2) == -1 and nn(acc=1, bias=P) == -1 and nn(sbytes=256) == -1
    assert nn(ldb=(1 << 31) // (2 * 65) // 8 * 8 + 8) == -1                                          # gemm_bf16x3_tn_ok's 32-bit offset rule
    assert nn(Ah=C.c_void_p(4096 + 8)) == -2
    assert nn(M=0) == 0 and nn(N=0, ldb=8, ldc=0) == 0                                               # nothing to do: nothing launched

    d = _lib.Dims(128, 300, 40, 136, 2, 3, 0, 0)
    pp = C.byref(_lib.Params(*([4096] * 9 + [None, None])))
    tb = L.s2vt_train_workspace_bytes(C.byref(d), 64, 320)
    sb = L.s2vt_split_grad_workspace_bytes(C.byref(d), 64, 320)

    def f(dims=C.byref(d), prm=pp, video=P, B=64, N=320, cap=P, steps=3, live=None, n_live=0, keep=0.9, vid=P, sid=P, logits=P, ws=P, nbytes=tb,
          sws=P, sbytes=sb):
        return L.s2vt_teacher_forced_fwd_split(dims, prm, video, B, N, cap, steps, live, n_live, keep, 7, vid, sid, logits, ws, nbytes, None, 0, 0,
                                               sws, sbytes, None)

    assert f(dims=None) == -1 and f(prm=None) == -1 and f(video=None) == -1 and f(cap=None) == -1 and f(logits=None) == -1 and f(ws=None) == -1
    assert f(sws=None) == -1                                                                         # the split entry needs its workspace
    assert f(B=0) == -1 and f(N=321) == -1 and f(steps=0) == -1 and f(steps=4) == -1 and f(keep=0.0) == -1 and f(vid=None) == -1
    assert f(live=P, n_live=0) == -1 and f(live=None, n_live=3) == -1 and f(live=P, n_live=3 * 320 + 1) == -1
    assert f(ws=C.c_void_p(4096 + 16)) == -2 and f(sws=C.c_void_p(4096 + 128)) == -2
    assert f(nbytes=tb - 256) == -3 and f(sbytes=sb - 256) == -3
    assert f(B=8, N=64, nbytes=1 << 40, sbytes=256) == -3                                            # held to its size below 256 rows too


_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import s2vt_amd
L = s2vt_amd.lib()
print(json.dumps([L.s2vt_split_fwd_stage(), L.s2vt_split_fwd_active(320), L.s2vt_split_fwd_active(257), L.s2vt_split_fwd_active(256)]))
"""


def _stage(**env_over):
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("S2VT_SPLIT_FWD", "S2VT_SPLIT_GRADS", "S2VT_SPLIT_FUSED")}
    env.update(env_over)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_split_fwd_env_is_parsed_as_documented():
    default = _stage()
    assert default[0] in (0, 1, 2) and default == [default[0], default[0], default[0], 0]            # active above 256 rows only
    for v in ("0", "1", "2"):
        assert _stage(S2VT_SPLIT_FWD=v) == [int(v), int(v), int(v), 0]
    for junk in ("", "3", "-1", "on", "1x", "02"):                                                   # anything else: the default
        assert _stage(S2VT_SPLIT_FWD=junk) == default
    assert _stage(S2VT_SPLIT_FWD="2", S2VT_SPLIT_GRADS="0") == [2, 0, 0, 0]                          # no split mode: the fp32 forward
    assert _stage(S2VT_SPLIT_FWD="1", S2VT_SPLIT_FUSED="0") == [1, 1, 1, 0]                          # the backward's layout knob does not matter
