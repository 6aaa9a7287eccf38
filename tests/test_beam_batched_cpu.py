"""Batched beam search without a GPU: the new entry points of include/s2vt.h validate their arguments before any launch, and the
caption file of the beam_eval tool has the reference's format (final_beam_search.py:530-545)."""
import ctypes

import s2vt_amd
from s2vt_amd import _lib


def test_beam_entry_points_validate_arguments():
    L = s2vt_amd.lib()
    P = ctypes.c_void_p(4096)                                   # never dereferenced: validation happens before any launch
    d = _lib.Dims(16, 11, 3, 4, 2, 3, 0, 0)
    dp = ctypes.byref(d)
    # s2vt_vocab_topk(logits, ld, R, V, k, ids, logp, stream)
    assert L.s2vt_vocab_topk(None, 11, 2, 11, 3, P, P, None) == -1
    assert L.s2vt_vocab_topk(P, 11, 2, 11, 17, P, P, None) == -1               # k > 16
    assert L.s2vt_vocab_topk(P, 11, 2, 11, 0, P, P, None) == -1
    assert L.s2vt_vocab_topk(P, 10, 2, 11, 3, P, P, None) == -1                # ld < V
    assert L.s2vt_vocab_topk(P, 11, 2, 11, 12, P, P, None) == -1               # k > V
    assert L.s2vt_vocab_topk(P, 11, 0, 11, 3, P, P, None) == 0                 # no rows: nothing to do
    # workspace query
    assert L.s2vt_beam_workspace_bytes(None, 4, 3) == 0
    assert L.s2vt_beam_workspace_bytes(dp, 4, 17) == 0
    assert L.s2vt_beam_workspace_bytes(dp, 0, 3) == 0
    nb = L.s2vt_beam_workspace_bytes(dp, 4, 3)
    assert nb > 0 and nb % 256 == 0 and L.s2vt_beam_workspace_bytes(dp, 4, 5) > nb
    # encode
    params = _lib.Params(*([4096] * 9 + [None, None]))
    pp = ctypes.byref(params)
    assert L.s2vt_beam_encode(dp, None, P, 4, 3, P, nb, None) == -1
    assert L.s2vt_beam_encode(dp, pp, None, 4, 3, P, nb, None) == -1
    assert L.s2vt_beam_encode(dp, pp, P, 4, 3, ctypes.c_void_p(4096 + 16), nb, None) == -2
    assert L.s2vt_beam_encode(dp, pp, P, 4, 3, P, nb - 256, None) == -3
    # step(d, p, B, beam, t, R, video_of_row, parent, word, k, top_ids, top_logp, logits_out, ws, bytes, stream)
    def step(B=4, beam=3, t=1, R=12, vid=P, par=P, word=P, k=3, ids=P, lp=P, ws=P, nbytes=nb, prm=pp):
        return L.s2vt_beam_step(dp, prm, B, beam, t, R, vid, par, word, k, ids, lp, None, ws, nbytes, None)
    assert step(k=17) == -1
    assert step(k=0) == -1
    assert step(R=13) == -1                                     # R > B * beam
    assert step(t=3) == -1 and step(t=-1) == -1                 # t >= Tc
    assert step(vid=None) == -1 and step(par=None) == -1 and step(word=None) == -1
    assert step(ids=None) == -1 and step(lp=None) == -1 and step(ws=None) == -1
    assert step(prm=None) == -1
    assert step(ws=ctypes.c_void_p(4096 + 64)) == -2
    assert step(nbytes=nb - 256) == -3                          # workspace too small
    assert step(R=0) == 0


def test_caption_file_format(tmp_path):
    from s2vt_amd.beam_eval import caption_text, read_captions, write_captions
    ix = {0: "<eos>", 1: "<bos>", 2: "a", 3: "man", 4: "is", 5: "running"}
    assert caption_text([2, 3, 4, 5, 0, 2, 2], ix) == "a man is running"       # cut at the first <eos>
    assert caption_text([1, 2, 3, 0], ix) == "a man"                           # <bos> dropped
    assert caption_text([0, 2], ix) == ""
    assert caption_text([2, 3, 4, 5], ix) == "a man is running"                # no <eos>: the whole caption
    p = tmp_path / "out.txt"
    write_captions(p, [("vid1", "a man is running"), ("vid2", "")])
    assert p.read_text() == "vid1\ta man is running\nvid2\t\n"
    assert read_captions(p) == {"vid1": "a man is running", "vid2": ""}
