"""s2vt_sample_mix (the mixed decode of build_mix_sample) without a GPU: the size query and the argument checks that come before any
device work."""
import ctypes

import pytest

import s2vt_amd
from s2vt_amd import _lib

BADARG = -1


def _dims():
    return _lib.Dims(16, 11, 3, 4, 2, 3, 0, 0)


def test_size_query_null_dims_and_bad_batch():
    L = s2vt_amd.lib()
    assert L.s2vt_sample_mix_workspace_bytes(None, 4, 1) == 0
    assert L.s2vt_sample_mix_workspace_bytes(ctypes.byref(_dims()), 0, 1) == 0


@pytest.mark.parametrize("dims", [(16, 11, 3, 4, 2, 3), (1536, 2000, 300, 992, 5, 8), (96, 300, 20, 48, 2, 7)])
@pytest.mark.parametrize("B", [1, 5, 16, 40, 150])
def test_size_query_holds_the_sampler_carve_and_the_fed_words(dims, B):
    """The layout is the plain sampler's carve for the SAME R = (1 + with_greedy) * B rows, then int32 word[R].  The plain query with
    K = 0 blocks has with_greedy * B rows -- fewer -- and is a lower bound too wherever a smaller row count cannot carve MORE: the
    fragment-order operands of the persistent decode loop exist at <= 64 rows and lstm_dim >= 132 only, so there the K = 0 query (0 or B
    rows) may hold megabytes that the carve for R rows does not (dims 992, B = 40 or 150), and the bound is the same-R one alone.  For the
    same reason the size grows with with_greedy except where the second block takes R across 64 rows (dims 992, B = 40): carve_sample's
    own step, which this entry point inherits unchanged."""
    L = s2vt_amd.lib()
    d = _lib.Dims(*dims, 0, 0)
    sizes = []
    for g in (0, 1):
        R = (1 + g) * B
        n = L.s2vt_sample_mix_workspace_bytes(ctypes.byref(d), B, g)
        assert n >= L.s2vt_sample_workspace_bytes(ctypes.byref(d), B, 1, g) + 4 * R
        assert n <= L.s2vt_sample_workspace_bytes(ctypes.byref(d), B, 1, g) + 4 * R + 255          # one region, 256-byte granules
        if d.lstm_dim < 132 or R <= 64:
            assert n >= L.s2vt_sample_workspace_bytes(ctypes.byref(d), B, 0, g) + 4 * R
        sizes.append(n)
    if d.lstm_dim < 132 or 2 * B <= 64 or B > 64:
        assert sizes[1] > sizes[0]


def test_badarg_null_pointers():
    L = s2vt_amd.lib()
    d = _dims()
    p = _lib.Params()                                              # every weight pointer NULL
    one = ctypes.c_void_p(256)                                     # (never dereferenced: the checks come first)
    assert L.s2vt_sample_mix(None, ctypes.byref(p), one, 4, one, 0.5, 1, 0, 0, one, one, 1 << 20, None) == BADARG
    assert L.s2vt_sample_mix(ctypes.byref(d), None, one, 4, one, 0.5, 1, 0, 0, one, one, 1 << 20, None) == BADARG
    assert L.s2vt_sample_mix(ctypes.byref(d), ctypes.byref(p), one, 4, one, 0.5, 1, 0, 0, one, one, 1 << 20, None) == BADARG
    for n in _lib.PARAM_FIELDS[:9]:
        setattr(p, n, 256)
    args = lambda video=one, B=4, cap=one, ids=one, ws=one: (ctypes.byref(d), ctypes.byref(p), video, B, cap, 0.5, 1, 0, 0, ids, ws, 1 << 20, None)
    assert L.s2vt_sample_mix(*args(video=None)) == BADARG
    assert L.s2vt_sample_mix(*args(cap=None)) == BADARG
    assert L.s2vt_sample_mix(*args(ids=None)) == BADARG
    assert L.s2vt_sample_mix(*args(ws=None)) == BADARG
    assert L.s2vt_sample_mix(*args(B=0)) == BADARG
    assert L.s2vt_sample_mix(*args(B=-3)) == BADARG


@pytest.mark.parametrize("p_gt", [-0.1, 1.5, float("nan")])
def test_badarg_probability_outside_unit_interval(p_gt):
    L = s2vt_amd.lib()
    d = _dims()
    p = _lib.Params()
    for n in _lib.PARAM_FIELDS[:9]:
        setattr(p, n, 256)
    one = ctypes.c_void_p(256)
    assert L.s2vt_sample_mix(ctypes.byref(d), ctypes.byref(p), one, 4, one, p_gt, 1, 0, 0, one, one, 1 << 20, None) == BADARG


def test_misaligned_workspace_is_reported_before_any_device_work():
    L = s2vt_amd.lib()
    d = _dims()
    p = _lib.Params()
    for n in _lib.PARAM_FIELDS[:9]:
        setattr(p, n, 256)
    one = ctypes.c_void_p(256)
    assert L.s2vt_sample_mix(ctypes.byref(d), ctypes.byref(p), one, 4, one, 0.5, 1, 0, 0, one, ctypes.c_void_p(264), 1 << 20, None) == -2
