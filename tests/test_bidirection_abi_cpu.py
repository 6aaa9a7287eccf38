"""s2vt_lstm_birecurrence_fwd / _scratch_bytes without a GPU: the size function and every argument check answer before
anything touches the device, as elsewhere in the C ABI (S2VT_E_BADARG = -1, sizes = 0)."""
import ctypes as C

import pytest

import s2vt_amd
from s2vt_amd import _lib

BADARG = -1


@pytest.fixture(scope="module")
def L():
    return s2vt_amd.lib()


def _dir(H=8, **kw):
    """a description whose pointers are never followed: the checks under test return first"""
    d = _lib.LstmDir()
    d.W, d.kw0, d.b = 0x1000, 4, 0x2000
    d.C_hist, d.H_hist, d.gates = 0x3000, 0x4000, 0x5000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(L, fw, bw, M=4, H=8, T=3, persistent=-1):
    return L.s2vt_lstm_birecurrence_fwd(None if fw is None else C.byref(fw), None if bw is None else C.byref(bw), M, H, T, persistent,
                                        None, 0, None)


def test_struct_layout_matches_the_header():
    # const float* W; int32 kw0; const float* b; const float* cinit; int64 tstride; int32 ld, t0, steps; float* C, H, gates
    assert C.sizeof(_lib.LstmDir) == 80
    assert [getattr(_lib.LstmDir, n).offset for n in ("W", "kw0", "b", "cinit", "cinit_tstride", "ldcinit", "cinit_t0", "cinit_steps",
                                                     "C_hist", "H_hist", "gates")] == [0, 8, 16, 24, 32, 40, 44, 48, 56, 64, 72]


def test_scratch_bytes(L):
    assert L.s2vt_lstm_birecurrence_scratch_bytes(0) == 0 and L.s2vt_lstm_birecurrence_scratch_bytes(-4) == 0
    small, big = L.s2vt_lstm_birecurrence_scratch_bytes(64), L.s2vt_lstm_birecurrence_scratch_bytes(1000)
    assert 0 < small < big and small % 256 == 0 and big % 256 == 0
    # the fallback runs one s2vt_lstm_recurrence_fwd per direction in the same scratch; the one-launch form needs two directions x
    # two parities x four row tiles x 64 KB of state images (1 MiB) + the counters
    assert big >= L.s2vt_lstm_recurrence_scratch_bytes(1000)
    assert big >= 2 * 2 * 4 * 64 * 1024 + 9 * 128


@pytest.mark.parametrize("kw", [dict(M=0), dict(M=-3), dict(H=0), dict(T=-1), dict(persistent=3), dict(persistent=-2)])
def test_bad_scalars(L, kw):
    assert _call(L, _dir(), _dir(), **kw) == BADARG


def test_null_descriptions(L):
    assert _call(L, None, _dir()) == BADARG
    assert _call(L, _dir(), None) == BADARG


@pytest.mark.parametrize("field", ["W", "b", "C_hist", "H_hist"])
@pytest.mark.parametrize("which", [0, 1])
def test_null_pointers_in_either_direction(L, field, which):
    dirs = [_dir(), _dir()]
    setattr(dirs[which], field, None)
    assert _call(L, *dirs) == BADARG


@pytest.mark.parametrize("kw", [dict(kw0=-1), dict(cinit=0x6000, ldcinit=31, cinit_steps=1), dict(cinit=0x6000, ldcinit=32, cinit_t0=-1, cinit_steps=1),
                                dict(cinit=0x6000, ldcinit=32, cinit_steps=-1)])
@pytest.mark.parametrize("which", [0, 1])
def test_odd_windows(L, kw, which):
    dirs = [_dir(), _dir()]
    for k, v in kw.items():
        setattr(dirs[which], k, v)
    assert _call(L, *dirs) == BADARG


# ---- the model's drivers: s2vt_bidir_*
def _dims(**kw):
    base = dict(dim_image=16, n_words=30, word_dim=4, lstm_dim=8, n_video_lstm_step=2, n_caption_lstm_step=3, label_dim=0, reserved=0)
    base.update(kw)
    return _lib.Dims(*[base[n] for n, _ in _lib.Dims._fields_])


def _bparams(**kw):
    p = _lib.BidirParams()
    for i, n in enumerate(_lib.BIDIR_PARAM_FIELDS):
        setattr(p, n, 0x10000 * (i + 1))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_bidir_params_layout():
    assert len(_lib.BIDIR_PARAM_FIELDS) == 11 and C.sizeof(_lib.BidirParams) == 88


@pytest.mark.parametrize("fn", ["s2vt_bidir_workspace_bytes", "s2vt_bidir_decode_workspace_bytes"])
def test_bidir_size_functions(L, fn):
    f = getattr(L, fn)
    d = _dims()
    sizes = [f(C.byref(d), B) for B in (1, 2, 16, 65, 150)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)       # grow with B
    assert f(None, 4) == 0 and f(C.byref(d), 0) == 0 and f(C.byref(d), -1) == 0
    for bad in (dict(lstm_dim=0), dict(n_words=1), dict(n_caption_lstm_step=0), dict(n_video_lstm_step=0), dict(word_dim=0), dict(dim_image=0),
                dict(reserved=1), dict(n_caption_lstm_step=129)):
        assert f(C.byref(_dims(**bad)), 4) == 0, bad
    assert L.s2vt_bidir_workspace_bytes(C.byref(d), 4) > L.s2vt_bidir_decode_workspace_bytes(C.byref(d), 4)     # the training workspace also holds gates and gradients


def _tf(L, d=None, p="ok", video=0x100, B=4, caption=0x200, keep=1.0, vid=None, sid=None, form=-1, out=0x300, ws=0x400, nbytes=1 << 30):
    d = _dims() if d is None else d
    p = _bparams() if p == "ok" else p
    return L.s2vt_bidir_teacher_forced_fwd(C.byref(d), None if p is None else C.byref(p), video, B, caption, keep, 0, vid, sid, form, out, ws, nbytes, None)


def test_bidir_teacher_forced_fwd_argument_checks(L):
    for kw in (dict(B=0), dict(video=None), dict(caption=None), dict(out=None), dict(ws=None), dict(keep=0.0), dict(keep=1.5), dict(keep=0.9),
               dict(keep=0.9, vid=0x500), dict(form=3), dict(form=-2), dict(p=None), dict(p=_bparams(lstm1_bw_W=None)), dict(p=_bparams(embed_word_b=None)),
               dict(d=_dims(reserved=1)), dict(d=_dims(lstm_dim=0))):
        assert _tf(L, **kw) == BADARG, kw
    assert L.s2vt_bidir_teacher_forced_fwd(None, C.byref(_bparams()), 0x100, 4, 0x200, 1.0, 0, None, None, -1, 0x300, 0x400, 1 << 30, None) == BADARG
    assert _tf(L, ws=0x404) == -2                              # S2VT_E_ALIGN: the workspace is 256-byte aligned
    assert _tf(L, nbytes=1024) == -3                           # S2VT_E_WORKSPACE


def test_bidir_bptt_bwd_argument_checks(L):
    d, p, g = _dims(), _bparams(), _bparams()

    def call(d=d, p=p, g=g, video=0x100, B=4, dl=0x200, keep=1.0, vid=None, sid=None, ws=0x400, nbytes=1 << 30):
        return L.s2vt_bidir_bptt_bwd(None if d is None else C.byref(d), None if p is None else C.byref(p), None if g is None else C.byref(g), video, B, dl,
                                     keep, 0, vid, sid, ws, nbytes, None)
    for kw in (dict(d=None), dict(p=None), dict(g=None), dict(g=_bparams(Wemb=None)), dict(video=None), dict(dl=None), dict(B=0), dict(keep=0.0),
               dict(keep=0.9), dict(ws=None), dict(d=_dims(reserved=1))):
        assert call(**kw) == BADARG, kw
    assert call(ws=0x410) == -2 and call(nbytes=4096) == -3


def test_bidir_decode_greedy_argument_checks(L):
    d, p = _dims(), _bparams()

    def call(d=d, p=p, video=0x100, B=4, unshifted=0, base=0, form=-1, ids=0x200, logits=None, ws=0x400, nbytes=1 << 30):
        return L.s2vt_bidir_decode_greedy(None if d is None else C.byref(d), None if p is None else C.byref(p), video, B, unshifted, base, form, ids, logits,
                                          ws, nbytes, None)
    for kw in (dict(d=None), dict(p=None), dict(p=_bparams(lstm2_W=None)), dict(video=None), dict(B=0), dict(B=-2), dict(ids=None), dict(ws=None),
               dict(form=3), dict(d=_dims(reserved=1)), dict(d=_dims(n_words=1))):
        assert call(**kw) == BADARG, kw
    assert call(ws=0x401) == -2 and call(nbytes=512) == -3
