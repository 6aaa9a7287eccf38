"""s2vt_bidir_sample / s2vt_bidir_teacher_forced_fwd_rows / s2vt_bidir_bptt_bwd_rows and their size functions without a GPU: every
argument check answers before anything touches the device, as elsewhere in the C ABI (S2VT_E_BADARG = -1, S2VT_E_ALIGN = -2,
S2VT_E_WORKSPACE = -3, sizes = 0)."""
import ctypes as C

import pytest

import s2vt_amd
from s2vt_amd import _lib

BADARG, ALIGN, WORKSPACE = -1, -2, -3


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


def test_sample_workspace_bytes(L):
    f = L.s2vt_bidir_sample_workspace_bytes
    d = _dims()
    by_b = [f(C.byref(d), B, 2, 1) for B in (1, 2, 16, 65, 150)]
    by_k = [f(C.byref(d), 4, K, 1) for K in (0, 1, 2, 5, 9)]
    for sizes in (by_b, by_k):
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    assert f(C.byref(d), 4, 2, 0) < f(C.byref(d), 4, 2, 1)                     # the greedy block is B more rows
    assert f(C.byref(d), 4, 0, 1) == L.s2vt_bidir_decode_workspace_bytes(C.byref(d), 4) - 256 * ((4 * 30 * 4 + 255) // 256)   # K = 0: the greedy decode's, without its logits rows
    assert f(None, 4, 2, 1) == 0 and f(C.byref(d), 0, 2, 1) == 0 and f(C.byref(d), -1, 2, 1) == 0
    assert f(C.byref(d), 4, -1, 1) == 0 and f(C.byref(d), 4, 0, 0) == 0        # K < 0; no rows at all
    assert f(C.byref(d), 1 << 20, 1 << 20, 1) == 0                             # (K + 1) * B beyond int
    for bad in BAD_DIMS:
        assert f(C.byref(_dims(**bad)), 4, 2, 1) == 0, bad


def test_rows_workspace_bytes(L):
    f = L.s2vt_bidir_rows_workspace_bytes
    d = _dims()
    by_b = [f(C.byref(d), B, 3) for B in (1, 2, 16, 65, 150)]
    by_s = [f(C.byref(d), 4, S) for S in (1, 2, 3, 8)]
    for sizes in (by_b, by_s):
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    for B in (1, 5, 64):
        assert f(C.byref(d), B, 1) >= L.s2vt_bidir_workspace_bytes(C.byref(d), B)
    assert f(None, 4, 2) == 0 and f(C.byref(d), 0, 2) == 0 and f(C.byref(d), -3, 2) == 0
    assert f(C.byref(d), 4, 0) == 0 and f(C.byref(d), 4, -1) == 0              # S < 1
    assert f(C.byref(d), 1 << 16, 1 << 16) == 0                                # S * B beyond int
    for bad in BAD_DIMS:
        assert f(C.byref(_dims(**bad)), 4, 2) == 0, bad


def test_sample_argument_checks(L):
    d, p = _dims(), _bparams()

    def call(d=d, p=p, video=0x100, B=4, K=2, greedy=1, base=0, form=-1, sampled=0x200, ids=0x300, ws=0x400, nbytes=1 << 30):
        return L.s2vt_bidir_sample(None if d is None else C.byref(d), None if p is None else C.byref(p), video, B, K, greedy, 11, base, form, sampled, ids,
                                   ws, nbytes, None)
    for kw in (dict(d=None), dict(p=None), dict(p=_bparams(lstm2_W=None)), dict(p=_bparams(Wemb=None)), dict(video=None), dict(B=0), dict(B=-2),
               dict(K=-1), dict(K=0, greedy=0), dict(sampled=None), dict(ids=None), dict(ws=None), dict(form=3), dict(form=-2),
               dict(d=_dims(reserved=1)), dict(d=_dims(n_words=1)), dict(B=1 << 20, K=1 << 20)):
        assert call(**kw) == BADARG, kw
    assert call(ws=0x401) == ALIGN and call(nbytes=512) == WORKSPACE
    assert call(K=0, sampled=None, nbytes=512) == WORKSPACE                    # legal without a sampled block: the next check answers
    assert call(greedy=0, ids=None, nbytes=512) == WORKSPACE
    need = L.s2vt_bidir_sample_workspace_bytes(C.byref(d), 4, 2, 1)
    assert call(nbytes=need - 1) == WORKSPACE


def test_teacher_forced_fwd_rows_argument_checks(L):
    d, p = _dims(), _bparams()

    def call(d=d, p=p, video=0x100, B=4, S=3, caption=0x200, keep=1.0, vid=None, sid=None, form=-1, out=0x300, ws=0x400, nbytes=1 << 30):
        return L.s2vt_bidir_teacher_forced_fwd_rows(None if d is None else C.byref(d), None if p is None else C.byref(p), video, B, S, caption, keep, 0,
                                                    vid, sid, form, out, ws, nbytes, None)
    for kw in (dict(d=None), dict(p=None), dict(p=_bparams(lstm1_bw_W=None)), dict(p=_bparams(embed_word_b=None)), dict(video=None), dict(caption=None),
               dict(out=None), dict(ws=None), dict(B=0), dict(S=0), dict(S=-1), dict(keep=0.0), dict(keep=1.5), dict(keep=0.9),
               dict(keep=0.9, vid=0x500), dict(keep=0.9, sid=0x500), dict(form=3), dict(form=-2), dict(d=_dims(reserved=1)), dict(d=_dims(lstm_dim=0)),
               dict(B=1 << 16, S=1 << 16)):
        assert call(**kw) == BADARG, kw
    assert call(ws=0x404) == ALIGN and call(nbytes=1024) == WORKSPACE
    need = L.s2vt_bidir_rows_workspace_bytes(C.byref(d), 4, 3)
    assert call(nbytes=need - 1) == WORKSPACE
    assert call(nbytes=L.s2vt_bidir_workspace_bytes(C.byref(d), 4)) == WORKSPACE      # the plain drivers' workspace is too short for three samples


def test_bptt_bwd_rows_argument_checks(L):
    d, p, g = _dims(), _bparams(), _bparams()

    def call(d=d, p=p, g=g, video=0x100, B=4, S=3, dl=0x200, keep=1.0, vid=None, sid=None, ws=0x400, nbytes=1 << 30):
        return L.s2vt_bidir_bptt_bwd_rows(None if d is None else C.byref(d), None if p is None else C.byref(p), None if g is None else C.byref(g), video,
                                          B, S, dl, keep, 0, vid, sid, ws, nbytes, None)
    for kw in (dict(d=None), dict(p=None), dict(g=None), dict(g=_bparams(Wemb=None)), dict(p=_bparams(lstm2_b=None)), dict(video=None), dict(dl=None),
               dict(B=0), dict(S=0), dict(S=-2), dict(keep=0.0), dict(keep=1.01), dict(keep=0.9), dict(keep=0.9, vid=0x500), dict(ws=None),
               dict(d=_dims(reserved=1)), dict(B=1 << 16, S=1 << 16)):
        assert call(**kw) == BADARG, kw
    assert call(ws=0x410) == ALIGN and call(nbytes=4096) == WORKSPACE
    need = L.s2vt_bidir_rows_workspace_bytes(C.byref(d), 4, 3)
    assert call(nbytes=need - 1) == WORKSPACE


def test_sample_sum_argument_checks(L):
    def call(dz=0x1000, out=0x2000, T=3, B=4, S=2, Cc=32):
        return L.s2vt_bidir_sample_sum(dz, out, T, B, S, Cc, None)
    for kw in (dict(dz=None), dict(out=None), dict(T=0), dict(B=0), dict(S=0), dict(S=-1), dict(Cc=0), dict(Cc=30), dict(B=1 << 16, S=1 << 16)):
        assert call(**kw) == BADARG, kw
    assert call(dz=0x1004) == ALIGN and call(out=0x2008) == ALIGN
