"""The four workspace-size functions of the attention captioner, pinned without a GPU: s2vt_attn_workspace_bytes,
s2vt_attn_rows_workspace_bytes (the shared-block form: n_video > 0), s2vt_attn_sample_workspace_bytes and
s2vt_attn_beam_workspace_bytes at a handful of tiny dims.  The regions are carved by three structs that share the image blocks
(csrc/attn_model.hip: AttnImg inside AttnWs, AttnSampleWs, AttnBeamWs); callers and tests index the workspaces by carve order, so
neither the order nor any region's size may move.

The expected byte counts are what the library built at commit bff3dab88f4301ca520af1bcd90d50462f9e549d returns (the parent of the
change that introduced AttnImg), written down as literals."""
import ctypes

import pytest

import s2vt_amd
from s2vt_amd import _lib

# dims (D, V, H, Tv, Tc), B (= n_video of the rows form), K, with_greedy, beam, samples
#   -> bytes of (workspace, rows workspace, sample workspace, beam workspace)
CASES = [
    (((16, 11, 4, 2, 3), 4, 2, 1, 3, 3), (511232, 527616, 8960, 4352)),          # the dims of test_attn_sample_ex_abi_cpu.py
    (((16, 11, 4, 2, 3), 1, 0, 1, 1, 1), (507648, 508160, 4864, 3840)),          # one video, greedy only, beam 1, one sample
    (((32, 50, 128, 9, 4), 3, 2, 0, 2, 2), (1007104, 1185024, 54272, 54528)),    # H = 128, more than 8 frames, no greedy block
    (((64, 300, 64, 5, 8), 64, 5, 1, 5, 5), (4263168, 17299968, 1262080, 1213440)),   # 64 videos x 5 samples = the 320-row REINFORCE shape
    (((24, 37, 12, 33, 5), 5, 1, 1, 16, 4), (586496, 712704, 29696, 71168)),     # odd sizes, Tv > 32, the widest beam
]


@pytest.mark.parametrize("shape,expected", CASES, ids=[f"H{c[0][0][2]}_Tv{c[0][0][3]}_B{c[0][1]}" for c in CASES])
def test_workspace_bytes_are_those_of_the_parent(shape, expected):
    (D, V, H, Tv, Tc), B, K, G, beam, samples = shape
    L = s2vt_amd.lib()
    d = ctypes.byref(_lib.Dims(D, V, 0, H, Tv, Tc, 0, 0))
    got = (L.s2vt_attn_workspace_bytes(d, B), L.s2vt_attn_rows_workspace_bytes(d, B, samples),
           L.s2vt_attn_sample_workspace_bytes(d, B, K, G), L.s2vt_attn_beam_workspace_bytes(d, B, beam))
    assert got == expected
    assert all(n % 256 == 0 for n in got)


def test_bad_shapes_size_to_zero():
    L = s2vt_amd.lib()
    d = ctypes.byref(_lib.Dims(16, 11, 0, 4, 2, 3, 0, 0))
    assert L.s2vt_attn_workspace_bytes(d, 0) == 0 and L.s2vt_attn_workspace_bytes(None, 4) == 0
    assert L.s2vt_attn_rows_workspace_bytes(d, 0, 3) == 0 and L.s2vt_attn_rows_workspace_bytes(d, 4, 0) == 0
    assert L.s2vt_attn_sample_workspace_bytes(d, 4, 0, 0) == 0 and L.s2vt_attn_sample_workspace_bytes(d, 4, -1, 1) == 0
    assert L.s2vt_attn_beam_workspace_bytes(d, 4, 0) == 0 and L.s2vt_attn_beam_workspace_bytes(d, 4, 17) == 0
