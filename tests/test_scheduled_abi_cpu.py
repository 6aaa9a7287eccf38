"""s2vt_scheduled_fwd / s2vt_scheduled_scratch_bytes / s2vt_sgd_guarded (scheduled-sampling training, generate_words_tf_s2vt.py:101-211,
412-418) without a GPU: the size query, the argument checks that come before any device work, and the inverse-sigmoid schedule."""
import ctypes
import math

import pytest

import s2vt_amd
from s2vt_amd import _lib

BADARG, ALIGN = -1, -2


def _dims():
    return _lib.Dims(16, 11, 3, 4, 2, 3, 0, 0)


def _params():
    p = _lib.Params()
    for n in _lib.PARAM_FIELDS[:9]:
        setattr(p, n, 256)
    return p


ONE = ctypes.c_void_p(256)                                         # (never dereferenced: the checks come first)
POINTERS = ("video", "caption", "video_id", "sample_id", "logits", "generated", "fed", "mask", "coef_tm", "target_tm", "ws", "scratch")


def _call(L, d, p, B=4, N=8, p_gt=0.5, keep=0.9, **ptr):
    g = lambda k: ptr.get(k, ONE)
    return L.s2vt_scheduled_fwd(d, p, g("video"), B, N, g("caption"), p_gt, 7, 1.0, keep, 3, g("video_id"), g("sample_id"), g("logits"),
                                g("generated"), g("fed"), g("mask"), g("coef_tm"), g("target_tm"), ptr.get("mask_sum"), ptr.get("mask_sum_copy"),
                                g("ws"), 1 << 20, g("scratch"), 1 << 20, None)


def test_size_query_zero_on_bad_arguments():
    L = s2vt_amd.lib()
    assert L.s2vt_scheduled_scratch_bytes(None, 4) == 0
    assert L.s2vt_scheduled_scratch_bytes(ctypes.byref(_dims()), 0) == 0
    assert L.s2vt_scheduled_scratch_bytes(ctypes.byref(_dims()), -2) == 0
    assert L.s2vt_scheduled_scratch_bytes(ctypes.byref(_lib.Dims(16, 11, 3, 4, 2, 0, 0, 0)), 4) == 0


@pytest.mark.parametrize("dims", [(16, 11, 3, 4, 2, 3), (256, 2000, 300, 992, 5, 8), (96, 300, 20, 48, 2, 7)])
def test_size_query_monotone_in_rows_and_independent_of_the_model_width(dims):
    """Per-step packed picks (one 128-byte line per row and step), the running mask and the pick launches' sample ids: it grows with N,
    holds at least those bytes, and does not depend on the layer widths."""
    L = s2vt_amd.lib()
    d = _lib.Dims(*dims, 0, 0)
    Tc = dims[5]
    sizes = [L.s2vt_scheduled_scratch_bytes(ctypes.byref(d), n) for n in (1, 5, 16, 64, 150, 384)]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    for n, s in zip((1, 5, 16, 64, 150, 384), sizes):
        assert s % 256 == 0 and s >= Tc * n * 128 + 8 * n
    wide = _lib.Dims(dims[0] * 2, dims[1] + 7, dims[2] + 1, dims[3] * 2, dims[4], dims[5], 0, 0)
    assert L.s2vt_scheduled_scratch_bytes(ctypes.byref(wide), 16) == sizes[2]


def test_train_workspace_size_is_the_teacher_forced_one():
    """The scheduled forward takes s2vt_train_workspace_bytes' workspace as it is: a workspace one byte-granule short is refused
    (no device work has happened by then), by the same check s2vt_teacher_forced_fwd makes."""
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    need = L.s2vt_train_workspace_bytes(ctypes.byref(d), 4, 8)
    assert need > 0
    g = ONE
    rc = L.s2vt_scheduled_fwd(ctypes.byref(d), ctypes.byref(p), g, 4, 8, g, 0.5, 7, 1.0, 0.9, 3, g, g, g, g, g, g, g, g, None, None, g, need - 256,
                              g, 1 << 20, None)
    assert rc == -3                                                  # S2VT_E_WORKSPACE
    short = L.s2vt_scheduled_scratch_bytes(ctypes.byref(d), 8) - 256
    rc = L.s2vt_scheduled_fwd(ctypes.byref(d), ctypes.byref(p), g, 4, 8, g, 0.5, 7, 1.0, 0.9, 3, g, g, g, g, g, g, g, g, None, None, g, need,
                              g, short, None)
    assert rc == -3


def test_badarg_null_dims_and_params():
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    assert _call(L, None, ctypes.byref(p)) == BADARG
    assert _call(L, ctypes.byref(d), None) == BADARG
    assert _call(L, ctypes.byref(d), ctypes.byref(_lib.Params())) == BADARG       # every weight pointer NULL


@pytest.mark.parametrize("which", POINTERS)
def test_badarg_each_null_pointer(which):
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    assert _call(L, ctypes.byref(d), ctypes.byref(p), **{which: None}) == BADARG


@pytest.mark.parametrize("p_gt", [-0.1, 1.5, float("nan")])
def test_badarg_probability_outside_unit_interval(p_gt):
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    assert _call(L, ctypes.byref(d), ctypes.byref(p), p_gt=p_gt) == BADARG


def test_badarg_rows_and_keep():
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    dd, pp = ctypes.byref(d), ctypes.byref(p)
    assert _call(L, dd, pp, B=4, N=6) == BADARG                       # N % B != 0
    assert _call(L, dd, pp, B=0, N=8) == BADARG
    assert _call(L, dd, pp, B=4, N=0) == BADARG
    assert _call(L, dd, pp, keep=0.0) == BADARG
    assert _call(L, dd, pp, keep=-0.5) == BADARG
    assert _call(L, dd, pp, keep=float("nan")) == BADARG


def test_misaligned_buffers_are_reported_before_any_device_work():
    L = s2vt_amd.lib()
    d, p = _dims(), _params()
    assert _call(L, ctypes.byref(d), ctypes.byref(p), ws=ctypes.c_void_p(264)) == ALIGN
    assert _call(L, ctypes.byref(d), ctypes.byref(p), scratch=ctypes.c_void_p(264)) == ALIGN


def test_sgd_badarg():
    L = s2vt_amd.lib()
    assert L.s2vt_sgd_guarded(None, ONE, 4, ONE, 10.0, 1e-3, 1, None, None) == BADARG
    assert L.s2vt_sgd_guarded(ONE, None, 4, ONE, 10.0, 1e-3, 1, None, None) == BADARG
    assert L.s2vt_sgd_guarded(ONE, ONE, -1, ONE, 10.0, 1e-3, 1, None, None) == BADARG
    assert L.s2vt_sgd_guarded(ONE, ONE, 4, ONE, 10.0, 1e-3, 0, None, None) == BADARG          # step >= 1, as s2vt_adam_tf


@pytest.mark.parametrize("k", [5000.0, 50.0, 1.0])
def test_inverse_sigmoid_schedule_is_the_closed_form(k):
    """generate_words_tf_s2vt.py:134 (commented there): p = k / (k + exp(steps / k)), float64."""
    from s2vt_amd.model import Video_Caption_Generator as G
    for steps in (0, 1, 17, 5000, 40000, 10 ** 7):
        x = steps / k
        want = k / (k + math.exp(x)) if x < 700 else 0.0
        got = G.inverse_sigmoid_prob(k, steps)
        assert got == want and 0.0 <= got <= k / (k + 1.0)
    assert G.inverse_sigmoid_prob(k, 0) == k / (k + 1.0)
    ps = [G.inverse_sigmoid_prob(k, s) for s in range(0, int(20 * k) + 1, max(1, int(k)))]
    assert all(b < a for a, b in zip(ps, ps[1:]))                    # strictly decreasing while it is representable
