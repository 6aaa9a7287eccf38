"""The entry points of the attention captioner's REINFORCE stage (rows that share image blocks) without a GPU: exported, present in
the ctypes table, and refusing NULL / non-positive arguments on the host before anything is launched."""
import ctypes

import s2vt_amd
from s2vt_amd import _lib

NEW = ["s2vt_attention_fwd_rows", "s2vt_attention_bwd_rows", "s2vt_attn_sample_workspace_bytes", "s2vt_attn_sample",
       "s2vt_attn_rows_workspace_bytes", "s2vt_attn_teacher_forced_fwd_rows", "s2vt_attn_step_scalars_rows", "s2vt_attn_bptt_bwd_rows"]


def _dims():
    return _lib.Dims(16, 11, 0, 4, 2, 3, 0, 0)


def test_new_symbols_exported_and_in_the_ctypes_table():
    L = ctypes.CDLL(_lib.lib_path())
    for n in NEW:
        assert hasattr(L, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} is missing from _lib.SIGNATURES"


def test_workspace_sizes_zero_on_bad_arguments_positive_on_good_ones():
    L = s2vt_amd.lib()
    d = _dims()
    assert L.s2vt_attn_sample_workspace_bytes(None, 4, 2, 1) == 0
    assert L.s2vt_attn_rows_workspace_bytes(None, 4, 2) == 0
    for B, K, g in [(0, 2, 1), (-1, 2, 1), (4, -1, 1), (4, 0, 0)]:
        assert L.s2vt_attn_sample_workspace_bytes(ctypes.byref(d), B, K, g) == 0, (B, K, g)
    for nv, S in [(0, 2), (4, 0), (-3, 2), (4, -1)]:
        assert L.s2vt_attn_rows_workspace_bytes(ctypes.byref(d), nv, S) == 0, (nv, S)
    too_many_frames = _lib.Dims(16, 11, 0, 4, 65, 3, 0, 0)
    assert L.s2vt_attn_sample_workspace_bytes(ctypes.byref(too_many_frames), 4, 2, 1) == 0
    assert L.s2vt_attn_rows_workspace_bytes(ctypes.byref(too_many_frames), 4, 2) == 0
    a = L.s2vt_attn_sample_workspace_bytes(ctypes.byref(d), 4, 2, 1)
    b = L.s2vt_attn_sample_workspace_bytes(ctypes.byref(d), 4, 0, 1)
    assert a > b > 0 and a % 256 == 0
    r1 = L.s2vt_attn_rows_workspace_bytes(ctypes.byref(d), 4, 1)
    r3 = L.s2vt_attn_rows_workspace_bytes(ctypes.byref(d), 4, 3)
    assert r3 > r1 > 0 and r3 % 256 == 0
    # the image blocks are counted once per video: three samples of four videos take less than twelve videos of one sample
    assert r3 < L.s2vt_attn_rows_workspace_bytes(ctypes.byref(d), 12, 1)


def test_entry_points_refuse_null_pointers():
    L = s2vt_amd.lib()
    d = ctypes.byref(_dims())
    assert L.s2vt_attn_sample(d, None, None, 4, 2, 1, 0, 0, None, None, None, 0, None) == -1
    assert L.s2vt_attn_sample(None, None, None, 4, 2, 1, 0, 0, None, None, None, 0, None) == -1
    assert L.s2vt_attn_teacher_forced_fwd_rows(d, None, None, 4, 2, None, 3, 1.0, 0, None, None, None, None, None, 0, None) == -1
    assert L.s2vt_attn_bptt_bwd_rows(d, None, None, None, 4, 2, None, 3, None, 0.5, 1.0, 0, None, None, None, 0, None) == -1
    assert L.s2vt_attn_step_scalars_rows(None, None, 0, None, 0.5, None, None, None, None, None, d, 4, 2, None, 0, None) == -1
    assert L.s2vt_attention_fwd_rows(None, None, None, None, None, None, None, None, 5, 2, 2, 8, None) == -1
    assert L.s2vt_attention_bwd_rows(None, None, None, None, None, None, None, None, None, None, None, 5, 2, 2, 8, 0, None) == -1


def test_single_ops_refuse_bad_sizes_before_touching_a_pointer():
    """Sizes are checked on the host with the pointers: a non-NULL pointer is never followed when a size is refused."""
    L = s2vt_amd.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for Tv, nv, S, H in [(0, 2, 2, 8), (65, 2, 2, 8), (5, 0, 2, 8), (5, 2, 0, 8), (5, 2, 2, 0)]:
        assert L.s2vt_attention_fwd_rows(p, p, p, p, p, p, p, p, Tv, nv, S, H, None) == -1, (Tv, nv, S, H)
        assert L.s2vt_attention_bwd_rows(p, p, p, p, p, p, p, p, p, p, p, Tv, nv, S, H, 0, None) == -1, (Tv, nv, S, H)
