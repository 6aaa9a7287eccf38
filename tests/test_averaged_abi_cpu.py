"""s2vt_averaged_fwd / s2vt_averaged_scratch_bytes / s2vt_averaged_bptt_bwd / s2vt_embed_scatter_add2 (averaged-embedding training,
average_generate_words_tf_s2vt.py:88-165,358-371) without a GPU: the size query and the argument checks that come before any device work."""
import ctypes

import pytest

import s2vt_amd
from s2vt_amd import _lib

BADARG, ALIGN, WORKSPACE = -1, -2, -3
RESIDUAL = 1


def _dims(bits=0):
    return _lib.Dims(16, 11, 3, 4, 2, 3, 0, bits)


def _params():
    p = _lib.Params()
    for n in _lib.PARAM_FIELDS[:9]:
        setattr(p, n, 256)
    return p


ONE = ctypes.c_void_p(256)                                         # (never dereferenced: the checks come first)
FWD_POINTERS = ("video", "caption", "mask", "video_id", "sample_id", "logits", "generated", "coef_tm", "target_tm", "ws", "scratch")


def _fwd(L, d, p, B=4, N=8, keep=0.9, ws_bytes=1 << 20, scratch_bytes=1 << 20, **ptr):
    g = lambda k: ptr.get(k, ONE)
    return L.s2vt_averaged_fwd(d, p, g("video"), B, N, g("caption"), g("mask"), 1.0, keep, 3, g("video_id"), g("sample_id"), g("logits"),
                               g("generated"), g("coef_tm"), g("target_tm"), ptr.get("mask_sum"), ptr.get("mask_sum_copy"), g("ws"), ws_bytes,
                               g("scratch"), scratch_bytes, None)


def _bwd(L, d, p, grads, B=4, N=8, keep=0.9, ws_bytes=1 << 20, scratch_bytes=1 << 20, precision=0, grad_ws=None, grad_ws_bytes=0, **ptr):
    g = lambda k: ptr.get(k, ONE)
    return L.s2vt_averaged_bptt_bwd(d, p, grads, g("video"), B, N, g("dlogits"), keep, 3, g("video_id"), g("sample_id"), g("ws"), ws_bytes,
                                    g("scratch"), scratch_bytes, precision, grad_ws, grad_ws_bytes, None)


def test_size_query_zero_on_bad_arguments():
    L = s2vt_amd.lib()
    assert L.s2vt_averaged_scratch_bytes(None, 4) == 0
    assert L.s2vt_averaged_scratch_bytes(ctypes.byref(_dims()), 0) == 0
    assert L.s2vt_averaged_scratch_bytes(ctypes.byref(_dims()), -2) == 0
    assert L.s2vt_averaged_scratch_bytes(ctypes.byref(_lib.Dims(16, 11, 3, 4, 2, 0, 0, 0)), 4) == 0
    assert L.s2vt_averaged_scratch_bytes(ctypes.byref(_dims(RESIDUAL)), 4) == 0          # no residual averaged graph exists


@pytest.mark.parametrize("dims", [(16, 11, 3, 4, 2, 3), (256, 2000, 300, 992, 5, 8), (96, 300, 20, 48, 2, 7)])
def test_size_query_grows_with_the_rows(dims):
    """Per (step, row): one 128-byte line of packed picks, E floats of Xbar and the two ids; per row: the pick launches' sample id."""
    L = s2vt_amd.lib()
    d = _lib.Dims(*dims, 0, 0)
    E, Tc = dims[2], dims[5]
    rows = (1, 5, 16, 64, 150, 384)
    sizes = [L.s2vt_averaged_scratch_bytes(ctypes.byref(d), n) for n in rows]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    for n, s in zip(rows, sizes):
        assert s % 256 == 0 and s >= Tc * n * (128 + 4 * E + 8) + 4 * n
    wider = _lib.Dims(dims[0], dims[1], dims[2] + 64, dims[3], dims[4], dims[5], 0, 0)
    assert L.s2vt_averaged_scratch_bytes(ctypes.byref(wider), 16) > sizes[2]             # Xbar is [Tc N, E]
    other = _lib.Dims(dims[0] * 2, dims[1] + 7, dims[2], dims[3] * 2, dims[4], dims[5], 0, 0)
    assert L.s2vt_averaged_scratch_bytes(ctypes.byref(other), 16) == sizes[2]


def test_forward_takes_the_training_workspace_and_its_own_scratch():
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    dd, pp = ctypes.byref(d), ctypes.byref(p)
    need = L.s2vt_train_workspace_bytes(dd, 4, 8)
    scratch = L.s2vt_averaged_scratch_bytes(dd, 8)
    assert need > 0 and scratch > 0
    assert _fwd(L, dd, pp, ws_bytes=need - 256, scratch_bytes=scratch) == WORKSPACE
    assert _fwd(L, dd, pp, ws_bytes=need, scratch_bytes=scratch - 256) == WORKSPACE


def test_forward_badarg_null_dims_and_params():
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    assert _fwd(L, None, ctypes.byref(p)) == BADARG
    assert _fwd(L, ctypes.byref(d), None) == BADARG
    assert _fwd(L, ctypes.byref(d), ctypes.byref(_lib.Params())) == BADARG
    assert _fwd(L, ctypes.byref(_dims(RESIDUAL)), ctypes.byref(p)) == BADARG


@pytest.mark.parametrize("which", FWD_POINTERS)
def test_forward_badarg_each_null_pointer(which):
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    assert _fwd(L, ctypes.byref(d), ctypes.byref(p), **{which: None}) == BADARG


def test_forward_badarg_rows_and_keep():
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    dd, pp = ctypes.byref(d), ctypes.byref(p)
    assert _fwd(L, dd, pp, B=4, N=6) == BADARG                        # N % B != 0
    assert _fwd(L, dd, pp, B=0, N=8) == BADARG
    assert _fwd(L, dd, pp, B=4, N=0) == BADARG
    assert _fwd(L, dd, pp, keep=0.0) == BADARG
    assert _fwd(L, dd, pp, keep=-0.5) == BADARG
    assert _fwd(L, dd, pp, keep=float("nan")) == BADARG


def test_forward_misaligned_buffers():
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    assert _fwd(L, ctypes.byref(d), ctypes.byref(p), ws=ctypes.c_void_p(264)) == ALIGN
    assert _fwd(L, ctypes.byref(d), ctypes.byref(p), scratch=ctypes.c_void_p(264)) == ALIGN


def test_backward_argument_checks():
    L = s2vt_amd.lib()
    d, p, g = _dims(), _params(), _params()
    dd, pp, gg = ctypes.byref(d), ctypes.byref(p), ctypes.byref(g)
    scratch = L.s2vt_averaged_scratch_bytes(dd, 8)
    need = L.s2vt_train_workspace_bytes(dd, 4, 8)
    assert _bwd(L, None, pp, gg) == BADARG
    assert _bwd(L, ctypes.byref(_dims(RESIDUAL)), pp, gg) == BADARG
    assert _bwd(L, dd, None, gg) == BADARG
    assert _bwd(L, dd, pp, None) == BADARG
    for which in ("video", "dlogits", "ws", "scratch"):
        assert _bwd(L, dd, pp, gg, **{which: None}) == BADARG, which
    assert _bwd(L, dd, pp, gg, B=4, N=6) == BADARG
    assert _bwd(L, dd, pp, gg, N=0) == BADARG
    assert _bwd(L, dd, pp, gg, scratch=ctypes.c_void_p(264)) == ALIGN
    assert _bwd(L, dd, pp, gg, ws=ctypes.c_void_p(264)) == ALIGN
    assert _bwd(L, dd, pp, gg, scratch_bytes=scratch - 256) == WORKSPACE
    assert _bwd(L, dd, pp, gg, ws_bytes=need - 256, scratch_bytes=scratch) == WORKSPACE
    # the precision and the gradient scratch go together: 0 takes none, 1 and 2 need theirs
    assert _bwd(L, dd, pp, gg, precision=3) == BADARG
    assert _bwd(L, dd, pp, gg, precision=-1) == BADARG
    assert _bwd(L, dd, pp, gg, precision=0, grad_ws=ONE, grad_ws_bytes=1 << 20) == BADARG
    assert _bwd(L, dd, pp, gg, precision=1) == BADARG
    assert _bwd(L, dd, pp, gg, precision=2) == BADARG
    assert _bwd(L, dd, pp, gg, precision=2, grad_ws=ctypes.c_void_p(264), grad_ws_bytes=1 << 20) == ALIGN
    short = L.s2vt_split_grad_workspace_bytes(dd, 4, 8) - 256
    assert _bwd(L, dd, pp, gg, precision=2, grad_ws=ONE, grad_ws_bytes=short) == WORKSPACE
    short = L.s2vt_bf16_grad_workspace_bytes(dd, 4, 8) - 256
    assert _bwd(L, dd, pp, gg, precision=1, grad_ws=ONE, grad_ws_bytes=short) == WORKSPACE


def test_scatter_add2_badarg():
    L = s2vt_amd.lib()
    f = L.s2vt_embed_scatter_add2
    assert f(None, 4, ONE, ONE, 0.5, 3, 4, ONE, None) == BADARG
    assert f(ONE, 4, None, ONE, 0.5, 3, 4, ONE, None) == BADARG
    assert f(ONE, 4, ONE, None, 0.5, 3, 4, ONE, None) == BADARG
    assert f(ONE, 4, ONE, ONE, 0.5, 3, 4, None, None) == BADARG
    assert f(ONE, 4, ONE, ONE, 0.5, -1, 4, ONE, None) == BADARG
    assert f(ONE, 4, ONE, ONE, 0.5, 3, 0, ONE, None) == BADARG
    assert f(ONE, 3, ONE, ONE, 0.5, 3, 4, ONE, None) == BADARG       # ld < E
    assert f(ONE, 4, ONE, ONE, 0.5, 0, 4, ONE, None) == 0            # R = 0: nothing is launched
