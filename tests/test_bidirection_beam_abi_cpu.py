"""s2vt_bidir_beam_workspace_bytes / s2vt_bidir_beam_encode / s2vt_bidir_beam_step, s2vt_lstm_cell_fwd_gather and beam_eval's model
detection without a GPU: every argument check answers before anything touches the device, as elsewhere in the C ABI (S2VT_E_BADARG = -1,
S2VT_E_ALIGN = -2, S2VT_E_WORKSPACE = -3, sizes = 0)."""
import ctypes as C

import pytest

import s2vt_amd
from s2vt_amd import _lib

OK, BADARG, ALIGN, WORKSPACE = 0, -1, -2, -3


@pytest.fixture(scope="module")
def L():
    return s2vt_amd.lib()


def _dims(**kw):
    base = dict(dim_image=16, n_words=30, word_dim=4, lstm_dim=8, n_video_lstm_step=2, n_caption_lstm_step=3, label_dim=0, reserved=0)
    base.update(kw)
    return _lib.Dims(*[base[n] for n, _ in _lib.Dims._fields_])


def _bparams(**kw):
    """device pointers that are never followed: the checks under test return first"""
    p = _lib.BidirParams()
    for i, n in enumerate(_lib.BIDIR_PARAM_FIELDS):
        setattr(p, n, 0x10000 * (i + 1))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_DIMS = (dict(lstm_dim=0), dict(n_words=1), dict(n_caption_lstm_step=0), dict(n_video_lstm_step=0), dict(word_dim=0), dict(dim_image=0),
            dict(reserved=1), dict(n_caption_lstm_step=129))


def test_beam_workspace_bytes(L):
    f = L.s2vt_bidir_beam_workspace_bytes
    d = _dims()
    by_b = [f(C.byref(d), B, 3) for B in (1, 2, 16, 65, 150)]
    by_beam = [f(C.byref(d), 4, beam) for beam in (1, 2, 3, 5, 16)]
    for sizes in (by_b, by_beam):
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    assert f(None, 4, 3) == 0 and f(C.byref(d), 0, 3) == 0 and f(C.byref(d), -1, 3) == 0
    assert f(C.byref(d), 4, 0) == 0 and f(C.byref(d), 4, 17) == 0 and f(C.byref(d), 4, -1) == 0
    assert f(C.byref(d), 1 << 30, 16) == 0                                     # B * beam beyond int
    for bad in BAD_DIMS:
        assert f(C.byref(_dims(**bad)), 4, 3) == 0, bad


@pytest.mark.parametrize("dims", [dict(), dict(lstm_dim=1000, word_dim=500, n_words=12000, dim_image=1024, n_video_lstm_step=25, n_caption_lstm_step=35),
                                  dict(lstm_dim=18, word_dim=10, n_words=97)])
@pytest.mark.parametrize("B,beam", [(1, 1), (3, 4), (32, 3), (150, 16)])
def test_beam_workspace_holds_no_gathered_copies(L, dims, B, beam):
    """Behind the once-per-video part: two parities of (c | h), the logits and the three index rows of the B * beam hypotheses, nothing more
    -- no gathered [Rmax, 4H] partial, no second set of state copies."""
    d = _dims(**dims)
    H, V, Rmax = d.lstm_dim, d.n_words, B * beam
    extra = L.s2vt_bidir_beam_workspace_bytes(C.byref(d), B, beam) - L.s2vt_bidir_decode_workspace_bytes(C.byref(d), B)
    assert extra <= 4 * Rmax * (4 * H + V) + 12 * Rmax + 64 * 256


def test_beam_encode_argument_checks(L):
    d, p = _dims(), _bparams()

    def call(d=d, p=p, video=0x100, B=4, beam=3, form=-1, ws=0x400, nbytes=1 << 30):
        return L.s2vt_bidir_beam_encode(None if d is None else C.byref(d), None if p is None else C.byref(p), video, B, beam, form, ws, nbytes, None)
    for kw in (dict(d=None), dict(p=None), dict(p=_bparams(lstm2_W=None)), dict(p=_bparams(lstm1_bw_b=None)), dict(video=None), dict(B=0), dict(B=-2),
               dict(beam=0), dict(beam=17), dict(ws=None), dict(form=3), dict(form=-2), dict(d=_dims(reserved=1)), dict(d=_dims(n_words=1)),
               dict(B=1 << 30, beam=16)):
        assert call(**kw) == BADARG, kw
    assert call(ws=0x401) == ALIGN and call(nbytes=512) == WORKSPACE
    need = L.s2vt_bidir_beam_workspace_bytes(C.byref(d), 4, 3)
    assert call(nbytes=need - 1) == WORKSPACE
    assert call(nbytes=L.s2vt_bidir_decode_workspace_bytes(C.byref(d), 4)) == WORKSPACE     # the greedy decode's workspace is too short for 12 rows


def test_beam_step_argument_checks(L):
    d, p = _dims(), _bparams()

    def call(d=d, p=p, B=4, beam=3, t=0, R=12, vid=0x100, par=0x200, word=0x300, k=3, ids=0x500, logp=0x600, logits=None, ws=0x400, nbytes=1 << 30):
        return L.s2vt_bidir_beam_step(None if d is None else C.byref(d), None if p is None else C.byref(p), B, beam, t, R, vid, par, word, k, ids, logp,
                                      logits, ws, nbytes, None)
    for kw in (dict(d=None), dict(p=None), dict(p=_bparams(Wemb=None)), dict(p=_bparams(embed_word_W=None)), dict(B=0), dict(beam=0), dict(beam=17),
               dict(t=-1), dict(t=3), dict(R=-1), dict(R=13), dict(k=0), dict(k=17), dict(d=_dims(n_words=10), k=11), dict(vid=None), dict(par=None),
               dict(word=None), dict(ids=None), dict(logp=None), dict(ws=None), dict(d=_dims(reserved=1)), dict(d=_dims(lstm_dim=0))):
        assert call(**kw) == BADARG, kw
    assert call(ws=0x408) == ALIGN and call(nbytes=512) == WORKSPACE
    need = L.s2vt_bidir_beam_workspace_bytes(C.byref(d), 4, 3)
    assert call(nbytes=need - 1) == WORKSPACE
    assert call(R=0, nbytes=need) == OK                                        # no rows: nothing is launched
    assert call(R=0, t=2, k=16, nbytes=need) == OK


def test_lstm_cell_fwd_gather_argument_checks(L):
    H, M = 8, 5
    x = _lib.Operand(0x9000, None, 4, 4, 0, 0)

    def call(x0=x, h=0x1000, c=0x2000, sidx=0x3000, ci=0x4000, ld=4 * H, cidx=0x5000, W=0x6000, b=0x7000, cn=0x8000, hn=0xA000, gates=None, M=M, H=H):
        return L.s2vt_lstm_cell_fwd_gather(None if x0 is None else C.byref(x0), None, h, c, sidx, ci, ld, cidx, W, b, cn, hn, gates, M, H, -1, None)
    for kw in (dict(h=None), dict(c=None), dict(W=None), dict(b=None), dict(cn=None), dict(hn=None), dict(M=-1), dict(H=0), dict(ld=4 * H - 1), dict(ld=0),
               dict(cn=0x2000), dict(hn=0x1000),                           # gathered state advanced in place: another workgroup owns the source row
               dict(x0=_lib.Operand(0x9000, None, 3, 4, 0, 0)), dict(x0=_lib.Operand(0x9000, None, 4, -1, 0, 0))):
        assert call(**kw) == BADARG, kw
    assert call(M=0) == OK                                                     # no rows: no device is needed
    assert call(M=0, ci=None, ld=0, cidx=None, sidx=None, cn=0x2000, hn=0x1000) == OK     # in place is legal without a gather
    assert call(M=0, ci=None, ld=0) == OK                                      # ldcinit is read with Cinit only


def test_model_kind_bidirectional():
    from s2vt_amd import bidirection
    from s2vt_amd.beam_eval import model_kind
    bidir = {name: 0 for name in bidirection.TF_NAMES.values()}
    rl = dict(bidir, g_step=0, beta1_power=0, **{bidirection.TF_NAMES["lstm2_W"] + "/Adam": 0})
    attention = {"Wemb": 0, "encode_image_W": 0, "embed_att_w": 0, "embed_att_Wa": 0, "embed_att_Ua": 0, "embed_word_W": 0,
                 "s2vt/LSTM3/basic_lstm_cell/weights": 0}
    s2vt = {"Wemb": 0, "encode_image_W": 0, "embed_word_W": 0, "lstm1_W": 0, "lstm2_W": 0, "s2vt/LSTM1/basic_lstm_cell/weights": 0}
    assert model_kind(bidir) == "bidirectional" and model_kind(rl) == "bidirectional" and model_kind(list(bidir)) == "bidirectional"
    assert model_kind(s2vt, "bidirectional") == "bidirectional" and model_kind(bidir, "s2vt") == "s2vt"      # --model overrides
    assert model_kind(attention) == "attention" and model_kind(s2vt) == "s2vt" and model_kind({}) == "s2vt"  # as before
    assert model_kind(attention, "s2vt") == "s2vt" and model_kind(s2vt, "attention") == "attention"
    with pytest.raises(ValueError):
        model_kind(bidir, "transformer")


def test_beam_eval_refuses_residual_for_a_bidirectional_checkpoint(tmp_path):
    """--residual is an S2VT variant: with a bidirectional checkpoint it is a SystemExit, before any model is built."""
    import numpy as np
    from s2vt_amd import beam_eval, bidirection
    vocab = ["<en_unk>", "a", "man", "is", "running"]
    (tmp_path / "vocab.txt").write_text("\n".join(vocab) + "\n")
    (tmp_path / "sents.txt").write_text("vid0\ta man is running\n")
    (tmp_path / "feats.txt").write_text("".join(f"vid0_frame_{k}," + ",".join("0.5" for _ in range(6)) + "\n" for k in range(2)))
    from s2vt_amd import hostglue
    V = len(hostglue.preProBuildWordVocab(vocab)[0])
    shapes = bidirection.param_shapes(6, V, 4, 8)
    np.savez(tmp_path / "ckpt.npz", **{bidirection.TF_NAMES[n]: np.zeros(s, np.float32) for n, s in shapes.items()})
    with pytest.raises(SystemExit, match="bidirectional"):
        beam_eval.main(["--checkpoint", str(tmp_path / "ckpt.npz"), "--test-sents", str(tmp_path / "sents.txt"), "--test-feats",
                        str(tmp_path / "feats.txt"), "--vocab", str(tmp_path / "vocab.txt"), "--residual", "--n-caption-lstm-step", "3"])
