"""Beam search for the temporal-attention captioner without a GPU: s2vt_attn_beam_workspace_bytes / _encode / _step validate their
arguments before any launch (the cases of test_beam_batched_cpu.py), and the beam_eval tool picks the model class from a
checkpoint's variable names."""
import ctypes

import pytest

import s2vt_amd
from s2vt_amd import _lib


def test_attn_beam_entry_points_validate_arguments():
    L = s2vt_amd.lib()
    P = ctypes.c_void_p(4096)                                   # never dereferenced: validation happens before any launch
    d = _lib.Dims(16, 11, 4, 4, 2, 3, 0, 0)                     # D 16, V 11, H 4, Tv 2, Tc 3
    dp = ctypes.byref(d)
    wide = _lib.Dims(16, 11, 4, 4, 65, 3, 0, 0)                 # Tv > 64: more frames than the attention step holds
    wp = ctypes.byref(wide)
    # workspace query
    assert L.s2vt_attn_beam_workspace_bytes(None, 4, 3) == 0
    assert L.s2vt_attn_beam_workspace_bytes(dp, 4, 17) == 0
    assert L.s2vt_attn_beam_workspace_bytes(dp, 4, 0) == 0
    assert L.s2vt_attn_beam_workspace_bytes(dp, 0, 3) == 0
    assert L.s2vt_attn_beam_workspace_bytes(wp, 4, 3) == 0
    nb = L.s2vt_attn_beam_workspace_bytes(dp, 4, 3)
    assert nb > 0 and nb % 256 == 0
    assert L.s2vt_attn_beam_workspace_bytes(dp, 4, 5) > nb > L.s2vt_attn_beam_workspace_bytes(dp, 4, 1)      # grows with the beam
    sizes = [L.s2vt_attn_beam_workspace_bytes(dp, 4, beam) for beam in range(1, 17)]            # (256-byte granules: never shrinks)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[15] > sizes[7] > sizes[3]
    # encode(d, p, video, B, beam, ws, bytes, stream)
    params = _lib.AttnParams(*([4096] * len(_lib.ATTN_PARAM_FIELDS)))
    pp = ctypes.byref(params)
    holed = _lib.AttnParams(*([4096] * (len(_lib.ATTN_PARAM_FIELDS) - 1) + [None]))
    assert L.s2vt_attn_beam_encode(dp, None, P, 4, 3, P, nb, None) == -1
    assert L.s2vt_attn_beam_encode(dp, ctypes.byref(holed), P, 4, 3, P, nb, None) == -1
    assert L.s2vt_attn_beam_encode(dp, pp, None, 4, 3, P, nb, None) == -1
    assert L.s2vt_attn_beam_encode(dp, pp, P, 4, 3, None, nb, None) == -1
    assert L.s2vt_attn_beam_encode(None, pp, P, 4, 3, P, nb, None) == -1
    assert L.s2vt_attn_beam_encode(dp, pp, P, 4, 17, P, nb, None) == -1
    assert L.s2vt_attn_beam_encode(wp, pp, P, 4, 3, P, 1 << 30, None) == -1
    assert L.s2vt_attn_beam_encode(dp, pp, P, 4, 3, ctypes.c_void_p(4096 + 16), nb, None) == -2
    assert L.s2vt_attn_beam_encode(dp, pp, P, 4, 3, P, nb - 256, None) == -3

    # step(d, p, B, beam, t, R, video_of_row, parent, word, k, top_ids, top_logp, logits_out, alphas_out, ws, bytes, stream)
    def step(B=4, beam=3, t=1, R=12, vid=P, par=P, word=P, k=3, ids=P, lp=P, ws=P, nbytes=nb, prm=pp, dims=dp):
        return L.s2vt_attn_beam_step(dims, prm, B, beam, t, R, vid, par, word, k, ids, lp, None, None, ws, nbytes, None)
    assert step(k=17) == -1
    assert step(k=0) == -1
    assert step(k=12) == -1                                     # k > V
    assert step(beam=17) == -1
    assert step(R=13) == -1                                     # R > B * beam
    assert step(R=-1) == -1
    assert step(t=3) == -1 and step(t=-1) == -1                 # t >= Tc
    assert step(vid=None) == -1 and step(par=None) == -1 and step(word=None) == -1
    assert step(ids=None) == -1 and step(lp=None) == -1 and step(ws=None) == -1
    assert step(prm=None) == -1 and step(dims=None) == -1
    assert step(dims=wp, nbytes=1 << 30) == -1                  # Tv > 64
    assert step(ws=ctypes.c_void_p(4096 + 64)) == -2
    assert step(nbytes=nb - 256) == -3                          # workspace too small
    assert step(R=0) == 0 and step(R=0, t=0) == 0               # no rows: nothing to do


def test_beam_eval_model_choice_from_variable_names():
    from s2vt_amd.beam_eval import model_kind
    attention = {"Wemb": 0, "encode_image_W": 0, "embed_att_w": 0, "embed_att_Wa": 0, "embed_att_Ua": 0, "embed_word_W": 0,
                 "s2vt/LSTM3/basic_lstm_cell/weights": 0}
    s2vt = {"Wemb": 0, "encode_image_W": 0, "embed_word_W": 0, "lstm1_W": 0, "lstm2_W": 0}
    assert model_kind(attention) == "attention"
    assert model_kind(s2vt) == "s2vt"
    assert model_kind(list(attention)) == "attention" and model_kind(iter(s2vt)) == "s2vt"       # any iterable of names
    assert model_kind({}) == "s2vt"
    assert model_kind(attention, "s2vt") == "s2vt" and model_kind(s2vt, "attention") == "attention"   # --model overrides
    assert model_kind(attention, "auto") == "attention"
    with pytest.raises(ValueError):
        model_kind(s2vt, "transformer")
