"""Top-k score-weighted embedding training (sum_generate_words_tf_s2vt.py:101-275): s2vt_topk_mix_fwd / _bwd, s2vt_embed_scatter_addk,
s2vt_topk_feed_fwd / _bptt_bwd / _decode and their ops wrappers, Video_Caption_Generator.topk_feed_update / generate_topk_feed.

The reference values come from tests/topk_feed_cases.py: a restatement of the unroll from the C oracle's pieces with the mix formed in
numpy float32, on cases tests/test_topk_feed_cases_cpu.py holds to the conditions that make these tests mean something (|S| >= 0.25, a
weights-detached backward ten times outside the gradient bound, a selected word in no caption).  Ids, weights, sums, operands and logits
are compared with array_equal; gradients with float64 autograd under the bound of tests/test_gpu_train.py's and test_gpu_averaged.py's
fp32 products (2e-4 of the tensor's largest entry); the single-op backward and the scatter with rtol 2e-5 / atol 2e-6."""
import ctypes

import numpy as np
import pytest

import topk_feed_cases as tc
from guardband import Guarded, GuardedWorkspace

pytestmark = pytest.mark.gpu

_models = {}
_refs = {}


@pytest.fixture(autouse=True)
def _no_chain_timeouts(gpu):
    """After every test of this file: no persistent recurrence has timed out."""
    yield
    assert gpu.chain_timeouts() == 0


def _model(oracle, name, keep=0.9, decay=None):
    """A model holding the case's parameters, and the device inputs: built once per (shape, keep, decay)."""
    key = (name, keep, decay)
    if key not in _models:
        import torch
        from s2vt_amd import model as M
        dims, B = tc.SHAPES[name]
        p, d, video, gt, mask, vid, sid = tc.case(oracle, name)
        mdl = M.Video_Caption_Generator(dims["dim_image"], dims["n_words"], dims["word_dim"], dims["lstm_dim"], B, 0, dims["n_video_lstm_step"],
                                        dims["n_caption_lstm_step"], seed=3, multisample=1, dropout_rate=keep)
        if decay is not None:
            mdl.decay_value = decay
        mdl.store.load(p)
        dev = lambda a: torch.as_tensor(a).cuda()
        _models[key] = (mdl, dev(video), dev(gt), dev(mask), dev(vid), dev(sid))
    return _models[key]


def _ref(oracle, name, keep, loss_weight=1.0, k=tc.K):
    """The restatement's result of a case: computed once, shared, never written to."""
    key = (name, keep, loss_weight, k)
    if key not in _refs:
        p, d, video, gt, mask, vid, sid = tc.case(oracle, name)
        _refs[key] = tc.unroll(oracle, p, d, video, gt, mask, vid, sid, k=k, keep=keep, loss_weight=loss_weight)
    return _refs[key]


def _fwd(gpu, mdl, video, cap, mask, vid, sid, keep, loss_weight=1.0, k=tc.K, **kw):
    return gpu.topk_feed_fwd(mdl.dims, mdl.store.params, video, cap, mask, cap.shape[0], k, loss_weight, keep, tc.DROP_SEED, vid, sid, **kw)


def _assert_forward(f, r):
    for key in ("generated", "coef_tm", "target_tm"):
        assert np.array_equal(f[key].cpu().numpy(), r[key]), key
    assert np.array_equal(f["logits"].cpu().numpy(), r["logits"])
    assert float(f["mask_sum"]) == r["mask_sum"]


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------- 1. the mix alone
def _scores(rng, R, V):
    """Rows of one sign (so that |S| >= 0.5): even rows positive, odd rows negative -- row 1 of every block has a negative S --, every
    third row quantised to quarters, which makes exact ties, also across the k-th place; R == 1: one positive row with ties."""
    s = rng.uniform(0.5, 1.5, (R, V)).astype(np.float32)
    s[::3] = np.round(s[::3] * 4) / 4
    s[1::2] *= -1
    if V >= 6:
        s[0, :6] = [1.25, 1.5, 1.25, 1.5, 1.25, 1.25]             # ties inside the selection and across its edge for k = 1, 5
    return s


@pytest.mark.parametrize("V", [5, 6, 131])
@pytest.mark.parametrize("R", [1, 5, 257])
def test_topk_mix_fwd_in_guard_bands(gpu, oracle, R, V):
    """ids, w, S and x array_equal the numpy restatement: E in {1, 24, 25}, k in {1, 5, 8} (k <= V), wide and odd row strides, ties
    across the k-th place (the lowest index wins), rows with a negative S; then the same on an unshifted-softmax plane (weights_mode 1)."""
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    rng = np.random.default_rng(R * 1000 + V)
    s = _scores(rng, R, V)
    _, probs = oracle.softmax_unshifted_argmax(s, want_probs=True)
    seen_tie = seen_negative = False
    for E in (1, 24, 25):
        W = rng.uniform(-0.1, 0.1, (V, E)).astype(np.float32)
        W[rng.integers(0, V), rng.integers(0, E)] = -0.0
        Wg = Guarded.of(W, lead=65, name="Wemb")
        for k in (k for k in (1, 5, 8) if k <= V):
            for mode, plane in ((0, s), (1, probs)):
                ld = V + 3 + 4 * (E == 24)
                sg = Guarded.of(plane, ld=ld, lead=67, name="scores")
                ids = Guarded(R, k, dtype=torch.int32, lead=65, name="ids")
                w = Guarded(R, k, lead=66, name="w")
                S = Guarded(1, R, lead=65, name="S")
                x = Guarded(R, E, ld=E + 7, lead=69, name="x")
                args = (sg.ptr, ld, None, 0) if mode == 0 else (None, 0, sg.ptr, ld)
                rc = L.s2vt_topk_mix_fwd(*args, mode, R, V, k, Wg.ptr, E, ids.ptr, w.ptr, S.ptr, x.ptr, x.ld, _stream())
                assert rc == 0
                ri, rw, rS, rx = tc.mix(plane, W, k)
                assert np.array_equal(ids.numpy(), ri), (E, k, mode)
                assert np.array_equal(w.numpy(), rw) and np.array_equal(S.numpy().ravel(), rS) and np.array_equal(x.numpy(), rx), (E, k, mode)
                for g in (sg, ids, w, S, x, Wg):
                    g.assert_intact()
                if mode == 0:
                    if k < V:
                        nxt = np.sort(plane, 1)[:, ::-1][:, k]
                        seen_tie |= bool((np.take_along_axis(plane, ri, 1)[:, -1] == nxt).any())
                    seen_negative |= bool((rS < 0).any())
                    if k == 1:
                        assert (rw == 1.0).all()
    assert seen_negative or R == 1
    assert seen_tie or V < 6


def test_topk_mix_wrapper_on_a_strided_view(gpu):
    import torch
    rng = np.random.default_rng(3)
    full = torch.as_tensor(rng.uniform(0.5, 1.5, (9, 40)).astype(np.float32)).cuda()
    W = torch.as_tensor(rng.uniform(-0.1, 0.1, (23, 7)).astype(np.float32)).cuda()
    ids, w, S, x = gpu.topk_mix_fwd(full[:, 5:28], W, 5)
    ri, rw, rS, rx = tc.mix(full[:, 5:28].cpu().numpy(), W.cpu().numpy(), 5)
    assert np.array_equal(ids.cpu().numpy(), ri) and np.array_equal(w.cpu().numpy(), rw)
    assert np.array_equal(S.cpu().numpy(), rS) and np.array_equal(x.cpu().numpy(), rx)


@pytest.mark.parametrize("V", [5, 6, 131])
@pytest.mark.parametrize("R", [1, 5, 257])
def test_topk_mix_bwd_and_scatter_in_guard_bands(gpu, R, V):
    """dscores[r][id_j] += (ds_j - g) / S, dO[r] += sum_j that * Wout[:, id_j] and dWemb[id_j] += w_j dx against float64, rtol 2e-5 /
    atol 2e-6 (tests/test_gpu_averaged.py's SGD replay bound); every buffer in guard bands; a column of dscores that no id names keeps
    its bits."""
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    rng = np.random.default_rng(R * 77 + V)
    s = _scores(rng, R, V)
    for E, H in ((1, 3), (24, 64), (25, 65)):
        W = rng.uniform(-0.1, 0.1, (V, E)).astype(np.float32)
        Wout = rng.uniform(-0.1, 0.1, (H, V)).astype(np.float32)
        dx = (0.05 * rng.standard_normal((R, E))).astype(np.float32)
        for k in (k for k in (1, 5, 8) if k <= V):
            ids, w, S, _ = tc.mix(s, W, k)
            d0 = rng.standard_normal((R, V)).astype(np.float32)
            o0 = rng.standard_normal((R, H)).astype(np.float32)
            e = W.astype(np.float64)[ids]                                        # [R, k, E]
            ds = np.einsum("re,rke->rk", dx.astype(np.float64), e)
            g = (w.astype(np.float64) * ds).sum(1, keepdims=True)
            dl = (ds - g) / S.astype(np.float64)[:, None]
            ref_d = d0.astype(np.float64)
            np.put_along_axis(ref_d, ids.astype(np.int64), np.take_along_axis(ref_d, ids.astype(np.int64), 1) + dl, 1)
            ref_o = o0.astype(np.float64) + np.einsum("rk,hrk->rh", dl, Wout.astype(np.float64)[:, ids])
            dxg = Guarded.of(dx, ld=E + 3, lead=65, name="dx")
            idg = Guarded.of(ids, lead=65, name="ids", fill=0)
            wg, Sg = Guarded.of(w, lead=67, name="w"), Guarded.of(S, lead=65, name="S")
            Wg, Og = Guarded.of(W, lead=66, name="Wemb"), Guarded.of(Wout, lead=65, name="Wout")
            dg = Guarded.of(d0, ld=V + 5, lead=69, name="dscores")
            og = Guarded.of(o0, ld=H + 2, lead=65, name="dO")
            rc = L.s2vt_topk_mix_bwd(dxg.ptr, dxg.ld, idg.ptr, wg.ptr, Sg.ptr, Wg.ptr, E, Og.ptr, V, H, k, R, dg.ptr, dg.ld, og.ptr, og.ld, _stream())
            assert rc == 0
            got_d, got_o = dg.numpy(), og.numpy()
            assert np.allclose(got_d, ref_d, rtol=2e-5, atol=2e-6), (E, k)
            assert np.allclose(got_o, ref_o, rtol=2e-5, atol=2e-6), (E, k)
            assert np.abs(got_o - o0).max() > 0 or k == 1                        # (k = 1: w = 1, ds - g = 0 exactly)
            named = np.zeros((R, V), bool)
            np.put_along_axis(named, ids.astype(np.int64), True, 1)
            assert np.array_equal(got_d.view(np.int32)[~named], d0.view(np.int32)[~named])
            # the weighted scatter of the same rows
            W0 = rng.standard_normal((V, E)).astype(np.float32)
            ref_w = W0.astype(np.float64)
            np.add.at(ref_w, ids.astype(np.int64), w.astype(np.float64)[:, :, None] * dx.astype(np.float64)[:, None, :])
            dWg = Guarded.of(W0, lead=66, name="dWemb")
            assert L.s2vt_embed_scatter_addk(dxg.ptr, dxg.ld, idg.ptr, wg.ptr, k, R, E, dWg.ptr, _stream()) == 0
            assert np.allclose(dWg.numpy(), ref_w, rtol=2e-5, atol=2e-6), (E, k)
            assert np.abs(dWg.numpy() - W0).max() > 0
            for gd in (dxg, idg, wg, Sg, Wg, Og, dg, og, dWg):
                gd.assert_intact()
            assert np.array_equal(dxg.numpy(), dx)


def test_mix_bwd_and_scatter_wrappers(gpu):
    import torch
    rng = np.random.default_rng(11)
    R, V, E, H, k = 12, 37, 20, 9, 5
    s = rng.uniform(0.5, 1.5, (R, V)).astype(np.float32)
    W = rng.uniform(-0.1, 0.1, (V, E)).astype(np.float32)
    Wout = rng.uniform(-0.1, 0.1, (H, V)).astype(np.float32)
    ids, w, S, _ = tc.mix(s, W, k)
    dev = lambda a: torch.as_tensor(a).cuda()
    full = dev((0.05 * rng.standard_normal((R, 30))).astype(np.float32))
    dx = full[:, 6:26]                                               # a row-strided view, as the embed slice of dX2 is
    dsc, dO = torch.zeros(R, V, device="cuda"), torch.zeros(R, H, device="cuda")
    gpu.topk_mix_bwd(dx, dev(ids), dev(w), dev(S), dev(W), dsc, dev(Wout), dO)
    ds = dx.double().cpu().numpy() @ W.astype(np.float64).T
    dsk = np.take_along_axis(ds, ids.astype(np.int64), 1)
    dl = (dsk - (w * dsk).sum(1, keepdims=True)) / S[:, None]
    ref = np.zeros((R, V)); np.put_along_axis(ref, ids.astype(np.int64), dl, 1)
    assert np.allclose(dsc.cpu().numpy(), ref, rtol=2e-5, atol=2e-6) and np.allclose(dO.cpu().numpy(), ref @ Wout.T.astype(np.float64), rtol=2e-5, atol=2e-6)
    dW = torch.zeros(V, E, device="cuda")
    gpu.embed_scatter_addk(dx, dev(ids), dev(w), dW)
    refw = np.zeros((V, E)); np.add.at(refw, ids.astype(np.int64), w[:, :, None].astype(np.float64) * dx.double().cpu().numpy()[:, None, :])
    assert np.allclose(dW.cpu().numpy(), refw, rtol=2e-5, atol=2e-6)


# ---------------------------------------------------------------------------------------------------------------- 2. the forward
@pytest.mark.parametrize("keep", tc.KEEPS)
@pytest.mark.parametrize("name", list(tc.SHAPES))
def test_forward_equals_the_restatement(gpu, oracle, name, keep):
    mdl, video, cap, mask, vid, sid = _model(oracle, name)
    r = _ref(oracle, name, keep)
    tc.assert_visible(r)
    _assert_forward(_fwd(gpu, mdl, video, cap, mask, vid, sid, keep), r)
    assert gpu.chain_timeouts() == 0


def test_scratch_holds_operands_ids_weights_and_sums(gpu, oracle):
    mdl, video, cap, mask, vid, sid = _model(oracle, "small-odd")
    r = _ref(oracle, "small-odd", 0.9)
    tc.assert_visible(r)
    f = _fwd(gpu, mdl, video, cap, mask, vid, sid, 0.9)
    v = gpu.topk_feed_scratch_views(mdl.dims, cap.shape[0], tc.K, f["scratch"])
    for key in ("X", "ids", "w", "S"):
        assert np.array_equal(v[key].cpu().numpy(), r[key]), key
    assert (r["ids"][0] == 1).all() and (r["S"][0] == 1).all()


def test_loss_weight_scales_the_coefficients(gpu, oracle):
    mdl, video, cap, mask, vid, sid = _model(oracle, "small-odd")
    r = _ref(oracle, "small-odd", 0.9, loss_weight=0.3)
    f = _fwd(gpu, mdl, video, cap, mask, vid, sid, 0.9, loss_weight=0.3)
    assert np.array_equal(f["coef_tm"].cpu().numpy(), r["coef_tm"])
    assert set(np.unique(r["coef_tm"])) == {np.float32(0.0), np.float32(0.3)}


@pytest.mark.parametrize("name", ["small-odd", "many-rows", "odd-width"])
def test_k_1_is_the_scheduled_unroll_on_its_own_picks(gpu, oracle, name):
    """k = 1: every weight is 1.0f and the operand is the picked word's row, so the logits are s2vt_scheduled_fwd(p_gt = 0)'s.  Compared
    with array_equal, not by bytes: the zero-started chain can turn a -0 operand into +0."""
    mdl, video, cap, mask, vid, sid = _model(oracle, name)
    f = _fwd(gpu, mdl, video, cap, mask, vid, sid, 0.9, k=1)
    v = gpu.topk_feed_scratch_views(mdl.dims, cap.shape[0], 1, f["scratch"])
    assert bool((v["w"] == 1.0).all())
    s = gpu.scheduled_fwd(mdl.dims, mdl.store.params, video, cap, cap.shape[0], 0.0, 5, 1.0, 0.9, tc.DROP_SEED, vid, sid)
    assert np.array_equal(f["logits"].cpu().numpy(), s["logits"].cpu().numpy())
    assert np.array_equal(f["generated"].cpu().numpy(), s["generated"].cpu().numpy())
    r = _ref(oracle, name, 0.9, k=1)
    _assert_forward(f, r)
    assert gpu.chain_timeouts() == 0


# ---------------------------------------------------------------------------------------------------------------- 3. gradients
def _grad_check(got, want, rel, what=""):
    """Per tensor: rel of the largest reference entry + 1e-9 (rel = 2e-4: tests/test_gpu_train.py::test_gradients_vs_float64_autograd's)."""
    for n in want:
        g, w = np.asarray(got[n], np.float64), np.asarray(want[n], np.float64)
        scale = np.abs(w).max() + 1e-12
        err = np.abs(g - w).max()
        print(f"{what}{n}: max |diff| = {err:.3e}, largest reference entry = {scale:.3e}, bound {rel * scale + 1e-9:.3e}")
        assert err <= rel * scale + 1e-9, (n, err, scale)


@pytest.mark.parametrize("name", ["small-odd", "odd-width"])
def test_update_gradients_vs_float64_autograd(gpu, oracle, name):
    """topk_feed_update(lr = 0, no weight decay, so that an untouched row of Wemb stays an exact zero), keep 0.9, against float64 autograd
    over the restated graph with the same dropout masks, the device's ids -- asserted equal to the restatement's first -- as constants."""
    mdl, video, cap, mask, vid, sid = _model(oracle, name, decay=0.0)
    mdl.set_step(0)
    p, d, v, gt, hm, hv, hs = tc.case(oracle, name)
    dseed = mdl.dropout_seed + 104729 * mdl.global_step
    r = tc.unroll(oracle, p, d, v, gt, hm, hv, hs, keep=0.9, drop_seed=dseed, loss_weight=mdl.loss_weight)
    tc.assert_visible(r)
    ref_loss, ref_g, ref_dl = tc.autograd(p, v, gt, hm, r, 0.9, mdl.loss_weight, 0.0)
    st = mdl.topk_feed_update(video, cap, mask, lr=0.0, clip_norm=10.0)
    f = mdl.last_topk_feed
    views = gpu.topk_feed_scratch_views(mdl.dims, cap.shape[0], tc.K, f["scratch"])
    assert np.array_equal(views["ids"].cpu().numpy(), r["ids"])
    assert np.array_equal(st.generated.cpu().numpy(), r["generated"]) and float(st.mask_sum) == r["mask_sum"]
    print(f"loss {float(st.loss)!r} reference {ref_loss!r}")
    assert abs(float(st.loss) - ref_loss) < 1e-4 * max(1.0, abs(ref_loss))
    got = {n: mdl.store.g[n].cpu().numpy() for n in mdl.store.names}
    _grad_check(got, ref_g, 2e-4)
    # dlogits after the call: sum(mask) times autograd's d loss / d logits, the mix's share included
    _grad_check({"dlogits": f["dlogits"].cpu().numpy() / r["mask_sum"]}, {"dlogits": ref_dl}, 2e-4)
    _, _, dl_det = tc.autograd(p, v, gt, hm, r, 0.9, mdl.loss_weight, 0.0, detach_weights=True)
    assert np.abs(dl_det - ref_dl).max() > 2e-3 * np.abs(ref_dl).max()               # (the softmax part alone is far outside the bound)
    # a row of Wemb that was only ever selected, at a (step, row) some later step weighs: non-zero on both sides; a row nobody read: exact zero
    live = (r["mask"][:, ::-1].cumsum(1)[:, ::-1] > 0).T                               # [Tc, N]
    sel = set(np.unique(r["ids"][1:][live[1:]]).tolist()) - set(np.unique(r["truth"]).tolist()) - {1}
    assert sel
    for row in sorted(sel):
        assert np.abs(ref_g["Wemb"][row]).max() > 0 and np.abs(got["Wemb"][row]).max() > 0, row
    untouched = sorted(set(range(d.n_words)) - set(np.unique(r["ids"]).tolist()))
    assert untouched and not got["Wemb"][untouched].any() and not ref_g["Wemb"][untouched].any()
    gn = sum((g ** 2).sum() for g in ref_g.values())
    assert abs(float(st.grad_sumsq) - gn) <= 1e-3 * gn
    assert gpu.chain_timeouts() == 0


def test_bf16_precision_is_refused(gpu, oracle):
    mdl, video, cap, mask, vid, sid = _model(oracle, "small-odd")
    saved = mdl.grad_precision
    mdl.grad_precision = "bf16"
    try:
        with pytest.raises(ValueError):
            mdl.topk_feed_update(video, cap, mask, lr=0.0)
    finally:
        mdl.grad_precision = saved
    for bad in (dict(k=0), dict(k=9), dict(clip="per_row"), dict(optimizer="momentum")):
        with pytest.raises(ValueError):
            mdl.topk_feed_update(video, cap, mask, lr=0.0, **bad)


# ---------------------------------------------------------------------------------------------------------------- 4. residency
@pytest.mark.parametrize("name", ["small-odd", "many-rows"])
def test_outputs_workspace_and_scratch_stay_inside_their_buffers(gpu, oracle, name):
    """Every output in guard bands; the training workspace and the scratch at exactly their declared sizes, both dirtied first; forward
    and backward then give the restatement's values and the default buffers' gradients.  A scratch 256 bytes short is refused by both
    entries before any launch."""
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    mdl, video, cap, mask, vid, sid = _model(oracle, name)
    N, Tc = cap.shape
    V = mdl.dims.n_words
    B = video.shape[0]
    k = tc.K
    r = _ref(oracle, name, 0.9)
    tc.assert_visible(r)
    out = dict(generated=Guarded(N, Tc, dtype=torch.int32, lead=65, name="generated"), coef_tm=Guarded(1, Tc * N, lead=66, name="coef_tm"),
               target_tm=Guarded(1, Tc * N, dtype=torch.int32, lead=65, name="target_tm"), logits=Guarded(Tc * N, V, lead=68, name="logits"),
               mask_sum=Guarded(1, 1, lead=65, name="mask_sum"), mask_sum_copy=Guarded(1, 1, lead=69, name="mask_sum_copy"))
    capg = Guarded.of(cap.cpu().numpy(), lead=65, name="caption", fill=2)
    maskg = Guarded.of(mask.cpu().numpy(), lead=67, name="mask")
    vidg = Guarded.of(vid.cpu().numpy(), lead=65, name="video_id", fill=0)
    sidg = Guarded.of(sid.cpu().numpy(), lead=65, name="sample_id", fill=0)
    ws_bytes = L.s2vt_train_workspace_bytes(ctypes.byref(mdl.dims), B, N)
    sc_bytes = L.s2vt_topk_feed_scratch_bytes(ctypes.byref(mdl.dims), N, k)
    ws, scr = GuardedWorkspace(ws_bytes, name="workspace"), GuardedWorkspace(sc_bytes, name="scratch")
    ws.window.fill_(0xA5); scr.window.fill_(0xFF)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = _stream()

    def fwd(scratch_bytes):
        return L.s2vt_topk_feed_fwd(ctypes.byref(mdl.dims), ctypes.byref(mdl.store.params), vp(video), B, N, capg.ptr, maskg.ptr, 1.0, 0.9, tc.DROP_SEED,
                                    vidg.ptr, sidg.ptr, k, out["logits"].ptr, out["generated"].ptr, out["coef_tm"].ptr, out["target_tm"].ptr,
                                    out["mask_sum"].ptr, out["mask_sum_copy"].ptr, ws.ptr, ws_bytes, scr.ptr, scratch_bytes, stream)

    def bwd(dlogits, scratch_bytes):
        return L.s2vt_topk_feed_bptt_bwd(ctypes.byref(mdl.dims), ctypes.byref(mdl.store.params), ctypes.byref(mdl.store.grads), vp(video), B, N,
                                         dlogits.ptr, 0.9, tc.DROP_SEED, vidg.ptr, sidg.ptr, k, ws.ptr, ws_bytes, scr.ptr, scratch_bytes, stream)
    assert fwd(sc_bytes - 256) == -3                                 # S2VT_E_WORKSPACE, nothing launched
    assert bool((scr.window == 0xFF).all()) and bool((ws.window == 0xA5).all())
    assert fwd(sc_bytes) == 0
    assert np.array_equal(out["generated"].numpy(), r["generated"])
    for key in ("coef_tm", "target_tm"):
        assert np.array_equal(out[key].numpy().ravel(), r[key]), key
    assert np.array_equal(out["logits"].numpy(), r["logits"])
    assert out["mask_sum"].numpy().item() == r["mask_sum"] == out["mask_sum_copy"].numpy().item()
    dl = torch.as_tensor(r["logits"]).cuda()
    coef, tgt = torch.as_tensor(r["coef_tm"]).cuda(), torch.as_tensor(r["target_tm"]).cuda()
    gpu.softmax_nll_fwd_bwd(dl, tgt, coef, 0.0)
    dlg = Guarded.of(dl.cpu().numpy(), lead=68, name="dlogits")
    assert bwd(dlg, sc_bytes - 256) == -3
    assert np.array_equal(dlg.numpy(), dl.cpu().numpy())
    gpu.zero_(mdl.store.grad)
    assert bwd(dlg, sc_bytes) == 0
    guarded = {n: mdl.store.g[n].cpu().numpy().copy() for n in mdl.store.names}
    guarded_dl = dlg.numpy().copy()
    for g in list(out.values()) + [capg, maskg, vidg, sidg, ws, scr, dlg]:
        g.assert_intact()
    assert np.abs(guarded_dl - dl.cpu().numpy()).max() > 0           # the mix's share has been added
    # the same pass on the cached default buffers
    f = _fwd(gpu, mdl, video, cap, mask, vid, sid, 0.9)
    gpu.zero_(mdl.store.grad)
    dl2 = dl.clone()
    gpu.topk_feed_bptt_bwd(mdl.dims, mdl.store.params, mdl.store.grads, video, N, dl2, f["ws"], f["scratch"], k, 0.9, tc.DROP_SEED, vid, sid)
    plain = {n: mdl.store.g[n].cpu().numpy().copy() for n in mdl.store.names}
    assert max(np.abs(g).max() for g in plain.values()) > 0
    _grad_check(guarded, plain, 2e-4)
    _grad_check({"dlogits": guarded_dl}, {"dlogits": dl2.cpu().numpy()}, 2e-4)
    assert gpu.chain_timeouts() == 0


# ---------------------------------------------------------------------------------------------------------------- 5. the generator
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("name", ["small-odd", "odd-width"])
def test_generator_equals_the_restatement(gpu, oracle, name, mode):
    """build_generator (:221-275): ids and logits under the script's rule (weights from the unshifted softmax) and under the training rule
    (raw logits); B = 5 / 6 and B = 1, the single video equal to its row of the batch."""
    import torch
    mdl, video, *_ = _model(oracle, name)
    p, d, v, *_ = tc.case(oracle, name)
    ref_ids, ref_logits = tc.generate(oracle, p, d, v, weights_mode=mode)
    ids, logits = gpu.topk_feed_decode(mdl.dims, mdl.store.params, video, tc.K, mode, True, return_logits=True)
    assert np.array_equal(ids.cpu().numpy(), ref_ids) and np.array_equal(logits.cpu().numpy(), ref_logits)
    one = gpu.topk_feed_decode(mdl.dims, mdl.store.params, video[2:3].contiguous(), tc.K, mode, True)
    assert np.array_equal(one.cpu().numpy()[0], ref_ids[2])
    assert torch.equal(mdl.generate_topk_feed(video, weights_mode=mode), ids)
    assert gpu.chain_timeouts() == 0


def test_generator_without_the_softmax_and_in_a_guarded_workspace(gpu, oracle):
    """unshifted_softmax = 0 with the training rule: the emitted word is the first of the top-k ids.  The workspace at exactly its declared
    size, dirtied, in guard bands; 256 bytes short is refused."""
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    mdl, video, *_ = _model(oracle, "small-odd")
    p, d, v, *_ = tc.case(oracle, "small-odd")
    ref_ids, ref_logits = tc.generate(oracle, p, d, v, weights_mode=0, unshifted_softmax=False)
    B, Tc, V = video.shape[0], mdl.dims.n_caption_lstm_step, mdl.dims.n_words
    nb = L.s2vt_topk_feed_decode_workspace_bytes(ctypes.byref(mdl.dims), B, tc.K)
    ws = GuardedWorkspace(nb, name="workspace")
    ws.window.fill_(0xA5)
    ids = Guarded(B, Tc, dtype=torch.int32, lead=65, name="ids")
    logits = Guarded(Tc * B, V, lead=68, name="logits")
    call = lambda nbytes: L.s2vt_topk_feed_decode(ctypes.byref(mdl.dims), ctypes.byref(mdl.store.params), ctypes.c_void_p(video.data_ptr()), B, tc.K, 0, 0,
                                                  ids.ptr, logits.ptr, ws.ptr, nbytes, _stream())
    assert call(nb - 256) == -3
    assert bool((ws.window == 0xA5).all())
    assert call(nb) == 0
    assert np.array_equal(ids.numpy(), ref_ids) and np.array_equal(logits.numpy(), ref_logits)
    for g in (ws, ids, logits):
        g.assert_intact()
    assert gpu.chain_timeouts() == 0


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_residual_model_is_refused(gpu):
    import torch
    import s2vt_amd
    from s2vt_amd import model as M
    mdl = M.Video_Caption_Generator(64, 131, 24, 32, 5, 0, 3, 9, multisample=1, residual=True)
    video = torch.zeros(5, 3, 64, device="cuda")
    cap = torch.full((5, 9), 2, dtype=torch.int32, device="cuda")
    mask = torch.ones(5, 9, device="cuda")
    with pytest.raises(ValueError):
        mdl.topk_feed_update(video, cap, mask, lr=0.0)
    with pytest.raises(ValueError):
        mdl.build_topk_feed_model()
    with pytest.raises(ValueError):
        mdl.generate_topk_feed(video)
    L = s2vt_amd.lib()
    assert L.s2vt_topk_feed_scratch_bytes(ctypes.byref(mdl.dims), 5, 5) == 0
    assert L.s2vt_topk_feed_decode_workspace_bytes(ctypes.byref(mdl.dims), 5, 5) == 0
    assert gpu.chain_timeouts() == 0
