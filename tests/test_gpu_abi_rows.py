"""Row kernels of the C ABI at their dispatch boundaries, inside guard bands (tests/guardband.py): the softmax-NLL forms (register
4 / 12 float4s per thread, streaming vector + tail, streaming scalar) by vocabulary size, row stride and pointer alignment, the split
planes at the same boundaries, s2vt_vocab_topk below one element per thread, s2vt_softmax_unshifted_argmax, and the host-side
refusals of s2vt_vocab_topk.  Every output lies in a Guarded buffer; inputs do too, so a read outside a row meets a NaN."""
import ctypes as C

import numpy as np
import pytest

from guardband import Guarded

pytestmark = pytest.mark.gpu

R = 8
# (V, ld, misaligned base), by the kernel form launch_softmax_nll picks
SOFTMAX_CASES = [
    (4, 4, False), (1024, 1024, False), (1028, 1032, False), (4096, 4096, False),          # register, 4 float4s per thread
    (4100, 4100, False), (12288, 12288, False),                                            # register, 12 float4s per thread
    (12292, 12292, False), (5, 8, False), (1023, 1024, False), (4097, 4100, False),        # streaming, vector + tail
    (1023, 1023, False), (4096, 4099, False), (4096, 4096, True),                          # streaming, scalar
]
SMOOTHINGS = ["zero", "0.05", "rows"]


def _lead(misaligned):
    return 65 if misaligned else 64


def _targets(V):
    t = [0, 1, 3, 4, V // 2, (V & ~3) - 1, V & ~3, V - 1]
    out = []
    for x in t:
        x = min(max(x, 0), V - 1)
        if x not in out:
            out.append(x)
    return out


def _target_rows(V, rot=0):
    tg = _targets(V)
    return np.array([tg[(r + rot) % len(tg)] for r in range(R)], np.int32)


def _rows(rng, V):
    """Eight rows: randn x 3 (0, 1; 6 with coef == 0), randn x 30 (2, 3, 7: the beam fixtures' regime), one logit 80 above the rest (4),
    a constant row (5)."""
    l = np.empty((R, V), np.float64)
    for r, s in ((0, 3), (1, 3), (2, 30), (3, 30), (6, 3), (7, 30)):
        l[r] = rng.standard_normal(V) * s
    l[4] = rng.standard_normal(V)
    l[4, (2 * V) // 3] = l[4].max() + 80.0
    l[5] = 1.25
    coef = rng.standard_normal(R)
    coef[np.abs(coef) < 0.1] = 0.5
    coef[6] = 0.0
    return l.astype(np.float32), coef.astype(np.float32)


def _ref(l, tgt, coef, s):
    """float64: nll, lp and coef * (softmax - q), q = onehot * (1 - s) + s / V, with a label smoothing s per row."""
    l = l.astype(np.float64)
    V = l.shape[1]
    mx = l.max(1, keepdims=True)
    lse = mx + np.log(np.exp(l - mx).sum(1, keepdims=True))
    logp = l - lse
    q = np.repeat(s[:, None] / V, V, 1)
    q[np.arange(len(tgt)), tgt] += 1.0 - s
    return -(q * logp).sum(1), logp[np.arange(len(tgt)), tgt], coef.astype(np.float64)[:, None] * (np.exp(logp) - q)


def _check_rows(tag, nll, lp, dl, ref, coef):
    """The bounds of test_gpu_train.py::test_softmax_nll_rows; prints the measured maxima (error / allowed, worst element)."""
    nll_ref, lp_ref, dl_ref = ref
    worst = {}
    for name, got, want, rtol, atol in (("nll", nll, nll_ref, 1e-5, 1e-5), ("lp", lp, lp_ref, 1e-5, 1e-5), ("dlogits", dl, dl_ref, 1e-4, 1e-6)):
        if got is None:                                              # (s2vt_xent_smooth_fwd_bwd returns no lp)
            continue
        err = np.abs(got.astype(np.float64) - want)
        worst[name] = (float(err.max()), float((err / (atol + rtol * np.abs(want))).max()))
    print(f"\n{tag}: " + ", ".join(f"{k} max err {e:.3e} ({f:.3f} of bound)" for k, (e, f) in worst.items()))
    for k, (e, f) in worst.items():
        assert f <= 1.0, (tag, k, e, f)
    zero = np.flatnonzero(coef == 0)
    assert len(zero) and not dl[zero].any()                          # coef == 0: zeros of either sign, never NaN
    return worst


def _smoothing(kind, rng, dev):
    if kind == "zero":
        return np.zeros(R), None
    if kind == "0.05":
        return np.full(R, np.float32(0.05), np.float64), None
    s = (rng.random(R) * 0.1).astype(np.float32)
    s[0] = 0.0
    return s.astype(np.float64), Guarded.of(s, lead=64, device=dev, name="smoothing_rows")


@pytest.mark.parametrize("smoothing", SMOOTHINGS)
@pytest.mark.parametrize("V,ld,misaligned", SOFTMAX_CASES)
def test_softmax_nll_forms(gpu, V, ld, misaligned, smoothing):
    import s2vt_amd
    L = s2vt_amd.lib()
    rng = np.random.default_rng(V * 7 + ld + SMOOTHINGS.index(smoothing))
    l, coef = _rows(rng, V)
    tg = _targets(V)
    s64, srows = _smoothing(smoothing, rng, "cuda")
    lead = _lead(misaligned)
    for rot in range(len(tg)):                                       # every row content meets every target position
        tgt = _target_rows(V, rot)
        ref = _ref(l, tgt, coef, s64)
        gl = Guarded.of(l, ld=ld, lead=lead, name="logits")
        gt = Guarded.of(tgt, lead=lead, name="target")
        gc = Guarded.of(coef, lead=lead, name="coef")
        nll = Guarded(1, R, lead=lead, name="nll")
        lp = Guarded(1, R, lead=lead, name="lp")
        assert gl.aligned16 != misaligned
        if srows is not None:
            rc = L.s2vt_softmax_nll_fwd_bwd_rows(gl.ptr, ld, R, V, gt.ptr, gc.ptr, srows.ptr, nll.ptr, lp.ptr, gpu._stream())
        else:
            rc = L.s2vt_softmax_nll_fwd_bwd(gl.ptr, ld, R, V, gt.ptr, gc.ptr, float(s64[0]), nll.ptr, lp.ptr, gpu._stream())
        assert rc == 0
        _check_rows(f"softmax V={V} ld={ld} mis={misaligned} s={smoothing} rot={rot}", nll.numpy()[0], lp.numpy()[0], gl.numpy(), ref, coef)
        for g in (gl, gt, gc, nll, lp):                              # the logits' pad columns [V, ld) keep their sentinel bits
            g.assert_intact()
    if srows is not None:
        srows.assert_intact()


def test_pg_nll_and_xent_smooth_by_name(gpu):
    """s2vt_pg_nll_fwd_bwd at (1023, 1024) and s2vt_xent_smooth_fwd_bwd at (4097, 4100): the streaming kernel's vector + tail form."""
    import s2vt_amd
    L = s2vt_amd.lib()
    rng = np.random.default_rng(11)
    # policy gradient: coef[t * N + n] = adv[n] * mask[n, t] formed on the device, smoothing 0
    V, ld, N, Tc = 1023, 1024, 4, 2
    l, _ = _rows(rng, V)
    tgt = _target_rows(V)
    adv = rng.standard_normal(N).astype(np.float32)
    mask = np.ones((N, Tc), np.float32); mask[1, 1] = 0.0
    coef = (mask * adv[:, None]).T.reshape(-1).astype(np.float32)
    gl, gt = Guarded.of(l, ld=ld, name="logits"), Guarded.of(tgt, name="target")
    ga, gm = Guarded.of(adv, name="adv"), Guarded.of(mask, name="mask")
    gco, nll, lp = Guarded(1, R, name="coef_scratch"), Guarded(1, R, name="nll"), Guarded(1, R, name="lp")
    assert L.s2vt_pg_nll_fwd_bwd(gl.ptr, ld, N, Tc, V, gt.ptr, ga.ptr, gm.ptr, gco.ptr, nll.ptr, lp.ptr, gpu._stream()) == 0
    assert np.array_equal(gco.numpy()[0], coef)
    _check_rows("pg_nll V=1023 ld=1024", nll.numpy()[0], lp.numpy()[0], gl.numpy(), _ref(l, tgt, coef, np.zeros(R)), coef)
    for g in (gl, gt, ga, gm, gco, nll, lp):
        g.assert_intact()
    # label-smoothed cross entropy: nll only
    V, ld = 4097, 4100
    l, coef = _rows(rng, V)
    tgt = _target_rows(V)
    gl, gt, gc, nll = Guarded.of(l, ld=ld, name="logits"), Guarded.of(tgt, name="target"), Guarded.of(coef, name="coef"), Guarded(1, R, name="nll")
    assert L.s2vt_xent_smooth_fwd_bwd(gl.ptr, ld, R, V, gt.ptr, gc.ptr, 0.05, nll.ptr, gpu._stream()) == 0
    ref = _ref(l, tgt, coef, np.full(R, np.float32(0.05), np.float64))
    _check_rows("xent_smooth V=4097 ld=4100", nll.numpy()[0], None, gl.numpy(), ref, coef)
    for g in (gl, gt, gc, nll):
        g.assert_intact()


# ---------------------------------------------------------------------------------------------------- split planes
@pytest.mark.parametrize("row_smoothing", [False, True])
@pytest.mark.parametrize("V", [4, 4096, 4100, 12288, 12292])
def test_softmax_split_planes_at_the_boundaries(gpu, V, row_smoothing):
    """The assertions of test_gpu_split_fused.py at the register kernel's size boundaries; at V = 12292 the call falls back and leaves
    the plain call's bits in place."""
    import torch
    import s2vt_amd
    from test_gpu_split_grads import _split_ref
    L = s2vt_amd.lib()
    Rr, B, N, Tc = 9, 64, 320, 20
    assert gpu.split_grad_active(N)
    dims = gpu.make_dims(128, V, 32, 64, 5, Tc)
    rng = np.random.default_rng(V + row_smoothing)
    l = (rng.standard_normal((Rr, V)) * 3).astype(np.float32)
    tgt = np.array([_targets(V)[r % len(_targets(V))] for r in range(Rr)], np.int32)
    coef = rng.standard_normal(Rr).astype(np.float32); coef[::7] = 0.0
    srows = Guarded.of((rng.random(Rr) * 0.1).astype(np.float32), name="smoothing_rows") if row_smoothing else None
    gt, gc = Guarded.of(tgt, name="target"), Guarded.of(coef, name="coef")
    want, nll0, lp0 = Guarded.of(l, name="dlogits(plain)"), Guarded(1, Rr, name="nll0"), Guarded(1, Rr, name="lp0")
    if row_smoothing:
        assert L.s2vt_softmax_nll_fwd_bwd_rows(want.ptr, V, Rr, V, gt.ptr, gc.ptr, srows.ptr, nll0.ptr, lp0.ptr, gpu._stream()) == 0
    else:
        assert L.s2vt_softmax_nll_fwd_bwd(want.ptr, V, Rr, V, gt.ptr, gc.ptr, 0.05, nll0.ptr, lp0.ptr, gpu._stream()) == 0
    gl, nll, lp = Guarded.of(l, name="logits"), Guarded(1, Rr, name="nll"), Guarded(1, Rr, name="lp")
    sws = gpu.split_grad_workspace(dims, B, N, "cuda")
    rc = L.s2vt_softmax_nll_fwd_bwd_split(gl.ptr, V, Rr, V, gt.ptr, gc.ptr, 0.05, None if srows is None else srows.ptr, nll.ptr, lp.ptr,
                                          C.byref(dims), B, N, C.c_void_p(sws.data_ptr()), sws.numel(), gpu._stream())
    assert rc == (1 if V > 12288 else 0)
    assert np.array_equal(nll.bits(), nll0.bits()) and np.array_equal(lp.bits(), lp0.bits())
    if rc == 1:                                                      # in_planes False: fp32 dlogits in place, as the plain call
        assert np.array_equal(gl.bits(), want.bits())
    else:
        hi, lo = gpu.split_grad_dlogits_planes(dims, B, N, Rr, "cuda")
        Kv = (V + 63) // 64 * 64
        assert hi.shape == (Rr, Kv) and lo.shape == (Rr, Kv)
        wh, wl = _split_ref(want.view)
        assert torch.equal(hi[:, :V].view(torch.int16), wh.view(torch.int16)) and torch.equal(lo[:, :V].view(torch.int16), wl.view(torch.int16))
        assert not hi[:, V:].view(torch.int16).any() and not lo[:, V:].view(torch.int16).any()
        assert np.array_equal(gl.bits(), l.view(np.int32))           # logits untouched
    for g in (gl, gt, gc, nll, lp, want, nll0, lp0) + (() if srows is None else (srows,)):
        g.assert_intact()


# ---------------------------------------------------------------------------------------------------- top-k
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("V,k", [(1, 1), (3, 3), (16, 16), (17, 16), (255, 16), (257, 16)])
def test_vocab_topk_small_vocabularies(gpu, V, k, pad):
    """k == V, and V below one element per thread (most per-thread candidate lists stay empty)."""
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    Rr, ld = 3, V + pad
    rng = np.random.default_rng(V * 31 + pad)
    l = (rng.standard_normal((Rr, V)) * 3).astype(np.float32)
    l[1, :] = 0.5                                                    # every value equal: ids 0 .. k-1
    if V >= 3:
        l[2, [0, V - 1]] = l[2].max() + 1.0                          # a tie between the first and the last column
    gl = Guarded.of(l, ld=ld, name="logits")
    ids, logp = Guarded(Rr, k, dtype=torch.int32, name="ids"), Guarded(Rr, k, name="logp")
    assert L.s2vt_vocab_topk(gl.ptr, ld, Rr, V, k, ids.ptr, logp.ptr, gpu._stream()) == 0
    order = np.argsort(-l, axis=1, kind="stable")[:, :k]             # value descending, index ascending on ties
    l64 = l.astype(np.float64)
    lp64 = l64 - (np.log(np.exp(l64 - l64.max(1, keepdims=True)).sum(1, keepdims=True)) + l64.max(1, keepdims=True))
    got_ids, got_lp = ids.numpy(), logp.numpy()
    assert np.array_equal(got_ids, order)
    assert got_ids[1].tolist() == list(range(k))
    err = np.abs(got_lp - np.take_along_axis(lp64, order.astype(np.int64), 1)).max()
    print(f"\ntopk V={V} k={k} ld={ld}: logp max err {err:.3e} (bound 1e-5)")
    assert err <= 1e-5
    for g in (gl, ids, logp):
        g.assert_intact()


@pytest.mark.parametrize("what,ld,V,k", [("ld < V", 10, 11, 3), ("k = 0", 11, 11, 0), ("k = 17", 32, 32, 17), ("k > V", 11, 11, 12)])
def test_vocab_topk_refusals(gpu, what, ld, V, k):
    """Checked on the host before any launch (beam.hip, s2vt_vocab_topk's first line): an error, and nothing is written."""
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    gl = Guarded.of(np.zeros((2, 32), np.float32), name="logits")
    ids, logp = Guarded(2, 17, dtype=torch.int32, name="ids"), Guarded(2, 17, name="logp")
    ids.view.zero_(); logp.view.zero_()
    assert L.s2vt_vocab_topk(gl.ptr, ld, 2, V, k, ids.ptr, logp.ptr, gpu._stream()) == -1, what
    torch.cuda.synchronize()
    assert not ids.bits().any() and not logp.bits().any()
    for g in (gl, ids, logp):
        g.assert_intact()


# ---------------------------------------------------------------------------------------------------- build_generator's argmax
@pytest.mark.parametrize("Rr,V,ld", [(3, 1, 1), (3, 255, 255), (5, 257, 260), (4, 12000, 12004)])
def test_softmax_unshifted_argmax_layouts(gpu, oracle, Rr, V, ld):
    """Ids and probabilities bit for bit the oracle's (the reference of test_gpu_beam.py), with a row stride, a tie (the lower index
    wins) and a logit above exp's overflow (>= 88.73: NaN there, zeros elsewhere, and the choice is <eos> = 0)."""
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    rng = np.random.default_rng(V)
    l = (rng.standard_normal((Rr, V)) * 3).astype(np.float32)
    l[0, V - 1] = 90.0                                               # the <eos> quirk
    if V >= 3:
        l[1, :] = 0.0; l[1, [V // 3, V // 2, V - 1]] = 3.0           # an exact tie
        l[2, V - 1] = 87.5                                           # large but finite: still the argmax
    ref_ids, ref_p = oracle.softmax_unshifted_argmax(l, True)
    assert ref_ids[0] == 0 and (V < 3 or (ref_ids[1] == V // 3 and ref_ids[2] == V - 1))
    gl = Guarded.of(l, ld=ld, name="logits")
    ids, probs = Guarded(1, Rr, dtype=torch.int32, name="ids"), Guarded(Rr, V, name="probs")
    assert L.s2vt_softmax_unshifted_argmax(gl.ptr, ld, Rr, V, ids.ptr, probs.ptr, gpu._stream()) == 0
    assert np.array_equal(ids.numpy()[0], ref_ids)
    assert np.array_equal(probs.bits(), ref_p.view(np.int32))        # NaNs included
    ids2 = Guarded(1, Rr, dtype=torch.int32, name="ids (no probs)")
    assert L.s2vt_softmax_unshifted_argmax(gl.ptr, ld, Rr, V, ids2.ptr, None, gpu._stream()) == 0
    assert np.array_equal(ids2.numpy()[0], ref_ids)
    for g in (gl, ids, probs, ids2):
        g.assert_intact()
