"""s2vt_topk_feed_scratch_bytes / _fwd / _bptt_bwd, s2vt_topk_feed_decode_workspace_bytes / _decode and the single-op entries
s2vt_topk_mix_fwd / _bwd / s2vt_embed_scatter_addk (top-k score-weighted embedding training, sum_generate_words_tf_s2vt.py:101-275)
without a GPU: the size queries and the argument checks that come before any device work."""
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
BWD_POINTERS = ("video", "dlogits", "video_id", "sample_id", "ws", "scratch")


def _fwd(L, d, p, B=4, N=8, keep=0.9, k=5, ws_bytes=1 << 20, scratch_bytes=1 << 20, **ptr):
    g = lambda key: ptr.get(key, ONE)
    return L.s2vt_topk_feed_fwd(d, p, g("video"), B, N, g("caption"), g("mask"), 1.0, keep, 3, g("video_id"), g("sample_id"), k, g("logits"),
                                g("generated"), g("coef_tm"), g("target_tm"), ptr.get("mask_sum"), ptr.get("mask_sum_copy"), g("ws"), ws_bytes,
                                g("scratch"), scratch_bytes, None)


def _bwd(L, d, p, grads, B=4, N=8, keep=0.9, k=5, ws_bytes=1 << 20, scratch_bytes=1 << 20, **ptr):
    g = lambda key: ptr.get(key, ONE)
    return L.s2vt_topk_feed_bptt_bwd(d, p, grads, g("video"), B, N, g("dlogits"), keep, 3, g("video_id"), g("sample_id"), k, g("ws"), ws_bytes,
                                     g("scratch"), scratch_bytes, None)


def _dec(L, d, p, B=4, k=5, mode=1, unshifted=1, ws_bytes=1 << 22, **ptr):
    g = lambda key: ptr.get(key, ONE)
    return L.s2vt_topk_feed_decode(d, p, g("video"), B, k, mode, unshifted, g("ids"), ptr.get("logits"), g("ws"), ws_bytes, None)


def test_size_queries_zero_on_bad_arguments():
    L = s2vt_amd.lib()
    for f in (L.s2vt_topk_feed_scratch_bytes, L.s2vt_topk_feed_decode_workspace_bytes):
        assert f(None, 4, 5) == 0
        assert f(ctypes.byref(_dims()), 0, 5) == 0
        assert f(ctypes.byref(_dims()), -2, 5) == 0
        assert f(ctypes.byref(_lib.Dims(16, 11, 3, 4, 2, 0, 0, 0)), 4, 5) == 0
        assert f(ctypes.byref(_dims(RESIDUAL)), 4, 5) == 0          # no residual top-k graph exists
        assert f(ctypes.byref(_dims()), 4, 0) == 0 and f(ctypes.byref(_dims()), 4, 9) == 0 and f(ctypes.byref(_dims()), 4, -1) == 0
        assert f(ctypes.byref(_lib.Dims(16, 4, 3, 4, 2, 3, 0, 0)), 4, 5) == 0              # k > n_words
        assert f(ctypes.byref(_lib.Dims(16, 5, 3, 4, 2, 3, 0, 0)), 4, 5) > 0


@pytest.mark.parametrize("dims", [(16, 11, 3, 4, 2, 3), (256, 2000, 300, 992, 5, 8), (96, 300, 20, 48, 2, 7)])
def test_scratch_size_is_monotone_in_rows_and_k(dims):
    """Per (step, row): one 128-byte line of packed picks, E floats of X, k ids, k weights and the raw sum; per row: the pick launches'
    sample id."""
    L = s2vt_amd.lib()
    d = _lib.Dims(*dims, 0, 0)
    E, Tc = dims[2], dims[5]
    rows = (1, 5, 16, 64, 150, 384)
    for k in (1, 5, 8):
        sizes = [L.s2vt_topk_feed_scratch_bytes(ctypes.byref(d), n, k) for n in rows]
        assert all(b > a for a, b in zip(sizes, sizes[1:]))
        for n, s in zip(rows, sizes):
            assert s % 256 == 0 and s >= Tc * n * (128 + 4 * E + 8 * k + 4) + 4 * n
    by_k = [L.s2vt_topk_feed_scratch_bytes(ctypes.byref(d), 150, k) for k in range(1, 9)]
    assert all(b >= a for a, b in zip(by_k, by_k[1:])) and by_k[-1] > by_k[0]
    wider = _lib.Dims(dims[0], dims[1], dims[2] + 64, dims[3], dims[4], dims[5], 0, 0)
    assert L.s2vt_topk_feed_scratch_bytes(ctypes.byref(wider), 16, 5) > L.s2vt_topk_feed_scratch_bytes(ctypes.byref(d), 16, 5)


@pytest.mark.parametrize("dims", [(16, 11, 3, 4, 2, 3), (96, 300, 20, 48, 2, 7)])
def test_decode_workspace_is_monotone_in_videos_and_k(dims):
    L = s2vt_amd.lib()
    d = _lib.Dims(*dims, 0, 0)
    sizes = [L.s2vt_topk_feed_decode_workspace_bytes(ctypes.byref(d), b, 5) for b in (1, 5, 16, 64, 150)]
    assert all(b > a for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    by_k = [L.s2vt_topk_feed_decode_workspace_bytes(ctypes.byref(d), 150, k) for k in range(1, 9)]
    assert all(b >= a for a, b in zip(by_k, by_k[1:])) and by_k[-1] > by_k[0]
    assert sizes[2] > L.s2vt_sample_workspace_bytes(ctypes.byref(d), 16, 0, 1) > 0          # the sampler's for B rows, and the mix's blocks


def test_forward_takes_the_training_workspace_and_its_own_scratch():
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    dd, pp = ctypes.byref(d), ctypes.byref(p)
    need = L.s2vt_train_workspace_bytes(dd, 4, 8)
    scratch = L.s2vt_topk_feed_scratch_bytes(dd, 8, 5)
    assert need > 0 and scratch > 0
    assert _fwd(L, dd, pp, ws_bytes=need - 256, scratch_bytes=scratch) == WORKSPACE
    assert _fwd(L, dd, pp, ws_bytes=need, scratch_bytes=scratch - 256) == WORKSPACE
    assert _fwd(L, dd, pp, k=8, ws_bytes=need, scratch_bytes=scratch) == WORKSPACE           # (a scratch sized for another k)


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


def test_forward_badarg_rows_keep_and_k():
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    dd, pp = ctypes.byref(d), ctypes.byref(p)
    assert _fwd(L, dd, pp, B=4, N=6) == BADARG                        # N % B != 0
    assert _fwd(L, dd, pp, B=0, N=8) == BADARG
    assert _fwd(L, dd, pp, B=4, N=0) == BADARG
    assert _fwd(L, dd, pp, keep=0.0) == BADARG
    assert _fwd(L, dd, pp, keep=-0.5) == BADARG
    assert _fwd(L, dd, pp, keep=float("nan")) == BADARG
    for k in (0, -1, 9):
        assert _fwd(L, dd, pp, k=k) == BADARG
    assert _fwd(L, ctypes.byref(_lib.Dims(16, 4, 3, 4, 2, 3, 0, 0)), pp, k=5) == BADARG      # k > n_words


def test_forward_misaligned_buffers():
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    assert _fwd(L, ctypes.byref(d), ctypes.byref(p), ws=ctypes.c_void_p(264)) == ALIGN
    assert _fwd(L, ctypes.byref(d), ctypes.byref(p), scratch=ctypes.c_void_p(264)) == ALIGN


def test_backward_argument_checks():
    L = s2vt_amd.lib()
    d, p, g = _dims(), _params(), _params()
    dd, pp, gg = ctypes.byref(d), ctypes.byref(p), ctypes.byref(g)
    scratch = L.s2vt_topk_feed_scratch_bytes(dd, 8, 5)
    need = L.s2vt_train_workspace_bytes(dd, 4, 8)
    assert _bwd(L, None, pp, gg) == BADARG
    assert _bwd(L, ctypes.byref(_dims(RESIDUAL)), pp, gg) == BADARG
    assert _bwd(L, dd, None, gg) == BADARG
    assert _bwd(L, dd, pp, None) == BADARG
    for which in BWD_POINTERS:
        assert _bwd(L, dd, pp, gg, **{which: None}) == BADARG, which
    assert _bwd(L, dd, pp, gg, B=4, N=6) == BADARG
    assert _bwd(L, dd, pp, gg, N=0) == BADARG
    assert _bwd(L, dd, pp, gg, keep=0.0) == BADARG
    for k in (0, 9):
        assert _bwd(L, dd, pp, gg, k=k) == BADARG
    assert _bwd(L, dd, pp, gg, scratch=ctypes.c_void_p(264)) == ALIGN
    assert _bwd(L, dd, pp, gg, ws=ctypes.c_void_p(264)) == ALIGN
    assert _bwd(L, dd, pp, gg, ws_bytes=need, scratch_bytes=scratch - 256) == WORKSPACE
    assert _bwd(L, dd, pp, gg, ws_bytes=need - 256, scratch_bytes=scratch) == WORKSPACE


def test_decode_argument_checks():
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    dd, pp = ctypes.byref(d), ctypes.byref(p)
    need = L.s2vt_topk_feed_decode_workspace_bytes(dd, 4, 5)
    assert need > 0
    assert _dec(L, None, pp) == BADARG and _dec(L, dd, None) == BADARG
    assert _dec(L, ctypes.byref(_dims(RESIDUAL)), pp) == BADARG
    for which in ("video", "ids", "ws"):
        assert _dec(L, dd, pp, **{which: None}) == BADARG, which
    assert _dec(L, dd, pp, B=0) == BADARG
    for k in (0, 9):
        assert _dec(L, dd, pp, k=k) == BADARG
    assert _dec(L, dd, pp, mode=2) == BADARG and _dec(L, dd, pp, mode=-1) == BADARG and _dec(L, dd, pp, unshifted=2) == BADARG
    assert _dec(L, dd, pp, mode=1, unshifted=0) == BADARG            # the probability plane is the unshifted softmax's
    assert _dec(L, dd, pp, ws=ctypes.c_void_p(264)) == ALIGN
    assert _dec(L, dd, pp, ws_bytes=need - 256) == WORKSPACE


def test_single_op_badarg():
    L = s2vt_amd.lib()
    f = L.s2vt_topk_mix_fwd            # (logits, ld, plane, ldp, mode, R, V, k, Wemb, E, ids, w, S, x, ldx, stream)
    ok = [ONE, 11, None, 0, 0, 3, 11, 5, ONE, 4, ONE, ONE, ONE, ONE, 4, None]
    assert f(*ok[:5], 0, *ok[6:]) == 0                               # R = 0: nothing is launched
    for i in (0, 8, 10, 11, 12, 13):
        a = list(ok); a[i] = None
        assert f(*a) == BADARG, i
    for i, v in ((1, 10), (5, -1), (6, 0), (7, 0), (7, 9), (7, 12), (9, 0), (14, 3), (4, 2), (2, ONE)):
        a = list(ok); a[i] = v
        assert f(*a) == BADARG, (i, v)
    plane = [None, 0, ONE, 11, 1, 0, 11, 5, ONE, 4, ONE, ONE, ONE, ONE, 4, None]
    assert f(*plane) == 0
    a = list(plane); a[2] = None
    assert f(*a) == BADARG
    a = list(plane); a[3] = 10
    assert f(*a) == BADARG
    b = L.s2vt_topk_mix_bwd            # (dx, lddx, ids, w, S, Wemb, E, Wout, V, H, k, R, dscores, lds, dO, ldo, stream)
    ok = [ONE, 4, ONE, ONE, ONE, ONE, 4, ONE, 11, 6, 5, 3, ONE, 11, ONE, 6, None]
    assert b(*ok[:11], 0, *ok[12:]) == 0
    for i in (0, 2, 3, 4, 5, 7, 12):
        a = list(ok); a[i] = None
        assert b(*a) == BADARG, i
    for i, v in ((1, 3), (6, 0), (8, 0), (9, 0), (10, 0), (10, 9), (11, -1), (13, 10), (15, 5)):
        a = list(ok); a[i] = v
        assert b(*a) == BADARG, (i, v)
    a = list(ok); a[14] = None; a[7] = None; a[11] = 0                # no dO: Wout is not needed
    assert b(*a) == 0
    s = L.s2vt_embed_scatter_addk      # (dE, ld, ids, w, k, R, E, dWemb, stream)
    ok = [ONE, 4, ONE, ONE, 5, 3, 4, ONE, None]
    assert s(*ok[:5], 0, *ok[6:]) == 0
    for i in (0, 2, 3, 7):
        a = list(ok); a[i] = None
        assert s(*a) == BADARG, i
    for i, v in ((1, 3), (4, 0), (4, 9), (5, -1), (6, 0)):
        a = list(ok); a[i] = v
        assert s(*a) == BADARG, (i, v)
