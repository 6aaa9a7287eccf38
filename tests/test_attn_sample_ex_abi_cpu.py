"""s2vt_attn_sample_ex (the attention captioner's sampler with flags: S2VT_SAMPLE_STOP_AT_EOS) without a GPU: exported, present in the
ctypes table, refusing unknown flag bits and NULL arguments on the host before anything is launched, and the sampler workspace grown by
the two live-row lists and the per-step counts.

Workspace of the shape used here -- dims (D 16, V 11, H 4, Tv 2, Tc 3), B = 4, K = 2, with the greedy block, so R = 12 rows -- before
the live lists were added: 8192 bytes (fourteen regions of one 256-byte granule each and the 4608 bytes of packed picks)."""
import ctypes

import s2vt_amd
from s2vt_amd import _lib

PARENT_WORKSPACE_BYTES = 8192
B, K, G, TC = 4, 2, 1, 3
R = (K + G) * B


def _dims():
    return _lib.Dims(16, 11, 0, 4, 2, TC, 0, 0)


def test_symbol_exported_and_in_the_ctypes_table():
    L = ctypes.CDLL(_lib.lib_path())
    assert hasattr(L, "s2vt_attn_sample_ex"), "s2vt_attn_sample_ex is not exported"
    assert "s2vt_attn_sample_ex" in _lib.SIGNATURES, "s2vt_attn_sample_ex is missing from _lib.SIGNATURES"
    # s2vt_attn_sample's arguments with `flags` behind video_base
    plain, ex = _lib.SIGNATURES["s2vt_attn_sample"], _lib.SIGNATURES["s2vt_attn_sample_ex"]
    assert ex[0] is plain[0] and len(ex[1]) == len(plain[1]) + 1
    assert list(ex[1][:8]) == list(plain[1][:8]) and ex[1][8] is ctypes.c_int32 and list(ex[1][9:]) == list(plain[1][8:])


def test_unknown_flag_bits_and_null_arguments_are_refused():
    L = s2vt_amd.lib()
    d = ctypes.byref(_dims())
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    params = _lib.AttnParams(*([p] * len(_lib.AttnParams._fields_)))
    # valid dims, params, pointers and sizes: only the flag is wrong (checked before anything is followed or launched)
    for flags in (2, 3, 4, -2):
        assert L.s2vt_attn_sample_ex(d, ctypes.byref(params), p, B, K, G, 0, 0, flags, p, p, p, 1 << 20, None) == -1, flags
    for flags in (0, 1):
        assert L.s2vt_attn_sample_ex(d, None, p, B, K, G, 0, 0, flags, p, p, p, 1 << 20, None) == -1          # NULL params
        assert L.s2vt_attn_sample_ex(None, ctypes.byref(params), p, B, K, G, 0, 0, flags, p, p, p, 1 << 20, None) == -1
        assert L.s2vt_attn_sample_ex(d, ctypes.byref(params), None, B, K, G, 0, 0, flags, p, p, p, 1 << 20, None) == -1
        assert L.s2vt_attn_sample_ex(d, ctypes.byref(params), p, B, K, G, 0, 0, flags, None, p, p, 1 << 20, None) == -1   # K > 0 needs ids_out
        assert L.s2vt_attn_sample_ex(d, ctypes.byref(params), p, B, K, G, 0, 0, flags, p, None, p, 1 << 20, None) == -1   # greedy needs greedy_out
        assert L.s2vt_attn_sample_ex(d, ctypes.byref(params), p, B, 0, 0, 0, 0, flags, p, p, p, 1 << 20, None) == -1      # nothing to sample
        assert L.s2vt_attn_sample_ex(d, ctypes.byref(params), p, B, K, G, 0, 0, flags, p, p, None, 0, None) == -1         # no workspace


def test_workspace_holds_the_live_lists_and_counts():
    L = s2vt_amd.lib()
    n = L.s2vt_attn_sample_workspace_bytes(ctypes.byref(_dims()), B, K, G)
    assert n >= PARENT_WORKSPACE_BYTES + (2 * R + TC) * 4, n
    assert n % 256 == 0
