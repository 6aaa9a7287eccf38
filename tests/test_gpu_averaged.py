"""Averaged-embedding training (average_generate_words_tf_s2vt.py:88-165,358-371): s2vt_averaged_fwd / ops.averaged_fwd,
s2vt_averaged_bptt_bwd / ops.averaged_bptt_bwd, s2vt_embed_scatter_add2 / ops.embed_scatter_add2, Video_Caption_Generator.averaged_update.

The reference values come from tests/averaged_cases.py: a restatement of the unroll from the C oracle's pieces, on cases in which a pick
differs from the ground truth it is averaged with and a picked word occurs in no caption (every parity test asserts that first, on the
restatement).  Ids, coefficients and logits are compared with array_equal; gradients with float64 autograd under the bound of
tests/test_gpu_train.py::test_gradients_vs_float64_autograd."""
import ctypes

import numpy as np
import pytest

import averaged_cases as ac
from guardband import Guarded, GuardedWorkspace

pytestmark = pytest.mark.gpu

_models = {}
_refs = {}

# the small-dimension shape above the row count at which the backward's products turn to split-bf16 (ops.split_grad_active: N > 256):
# tests/test_gpu_split_fused.py's dimensions, 4 samples of 66 videos = 264 rows
SPLIT_DIMS = dict(dim_image=128, n_words=260, word_dim=32, lstm_dim=64, n_video_lstm_step=5, n_caption_lstm_step=8)
SPLIT_B, SPLIT_REP = 66, 4


def _model(oracle, name, keep=0.9, decay=None):
    """A model holding the case's parameters, and the device inputs: built once per (shape, keep, decay)."""
    key = (name, keep, decay)
    if key not in _models:
        import torch
        from s2vt_amd import model as M
        if name == "split":
            dims, B = SPLIT_DIMS, SPLIT_B
            p, d, video, gt, mask, vid, sid = ac.tiled_case(oracle, SPLIT_DIMS, SPLIT_B, SPLIT_REP)
        else:
            dims, B = ac.SHAPES[name]
            p, d, video, gt, mask, vid, sid = ac.case(oracle, name)
        mdl = M.Video_Caption_Generator(dims["dim_image"], dims["n_words"], dims["word_dim"], dims["lstm_dim"], B, 0, dims["n_video_lstm_step"],
                                        dims["n_caption_lstm_step"], seed=3, multisample=1, dropout_rate=keep)
        if decay is not None:
            mdl.decay_value = decay
        mdl.store.load(p)
        dev = lambda a: torch.as_tensor(a).cuda()
        _models[key] = (mdl, dev(video), dev(gt), dev(mask), dev(vid), dev(sid))
    return _models[key]


def _ref(oracle, name, keep, loss_weight=1.0):
    """The restatement's result of a case: computed once, shared, never written to."""
    key = (name, keep, loss_weight)
    if key not in _refs:
        p, d, video, gt, mask, vid, sid = ac.case(oracle, name)
        _refs[key] = ac.averaged_unroll(oracle, p, d, video, gt, mask, vid, sid, keep=keep, loss_weight=loss_weight)
    return _refs[key]


def _fwd(gpu, mdl, video, cap, mask, vid, sid, keep, loss_weight=1.0, **kw):
    return gpu.averaged_fwd(mdl.dims, mdl.store.params, video, cap, mask, cap.shape[0], loss_weight, keep, ac.DROP_SEED, vid, sid, **kw)


def _assert_forward(f, r):
    for k in ("generated", "coef_tm", "target_tm"):
        assert np.array_equal(f[k].cpu().numpy(), r[k]), k
    assert np.array_equal(f["logits"].cpu().numpy(), r["logits"])
    assert float(f["mask_sum"]) == r["mask_sum"]


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("keep", ac.KEEPS)
@pytest.mark.parametrize("name", list(ac.SHAPES))
def test_forward_equals_the_restatement(gpu, oracle, name, keep):
    mdl, video, cap, mask, vid, sid = _model(oracle, name)
    r = _ref(oracle, name, keep)
    ac.assert_visible(r)
    _assert_forward(_fwd(gpu, mdl, video, cap, mask, vid, sid, keep), r)
    assert gpu.chain_timeouts() == 0


def test_scratch_holds_the_means_and_the_id_pairs(gpu, oracle):
    """What the backward reads again, behind the packed picks and the pick launches' sample ids: Xbar [Tc N, E], then the two id arrays."""
    import torch
    mdl, video, cap, mask, vid, sid = _model(oracle, "small-odd")
    r = _ref(oracle, "small-odd", 0.9)
    ac.assert_visible(r)
    f = _fwd(gpu, mdl, video, cap, mask, vid, sid, 0.9)
    N, Tc = cap.shape
    E = mdl.dims.word_dim
    up = lambda b: (b + 255) // 256 * 256
    off = up(Tc * N * 16 * 8) + up(N * 4)
    s = f["scratch"]
    xbar = s[off:off + Tc * N * E * 4].view(torch.float32).view(Tc, N, E).cpu().numpy()
    off += up(Tc * N * E * 4)
    ida = s[off:off + Tc * N * 4].view(torch.int32).view(Tc, N).cpu().numpy()
    off += up(Tc * N * 4)
    idb = s[off:off + Tc * N * 4].view(torch.int32).view(Tc, N).cpu().numpy()
    assert off + up(Tc * N * 4) == s2vt_scratch_bytes(mdl, N)
    assert np.array_equal(xbar, r["xbar"]) and np.array_equal(ida, r["ida"]) and np.array_equal(idb, r["idb"])


def s2vt_scratch_bytes(mdl, N):
    import s2vt_amd
    return s2vt_amd.lib().s2vt_averaged_scratch_bytes(ctypes.byref(mdl.dims), N)


def test_loss_weight_scales_the_coefficients(gpu, oracle):
    mdl, video, cap, mask, vid, sid = _model(oracle, "small-odd")
    r = _ref(oracle, "small-odd", 0.9, loss_weight=0.3)
    f = _fwd(gpu, mdl, video, cap, mask, vid, sid, 0.9, loss_weight=0.3)
    assert np.array_equal(f["coef_tm"].cpu().numpy(), r["coef_tm"])
    assert set(np.unique(r["coef_tm"])) == {np.float32(0.0), np.float32(0.3)}


# ---------------------------------------------------------------------------------------------------------------- 2. the fixed point
@pytest.mark.parametrize("name", ["small-odd", "many-rows", "chain-range", "odd-width"])
def test_own_greedy_caption_is_the_teacher_forced_pass(gpu, oracle, name):
    """keep = 1, caption = the model's own greedy ids: every pick equals the ground truth it is averaged with, every mean is a plain row of
    Wemb bit for bit, and the logits are s2vt_teacher_forced_fwd's for that caption."""
    import torch
    mdl, video, cap, mask, vid, sid = _model(oracle, name)
    _, greedy = gpu.sample(mdl.dims, mdl.store.params, video, 1, 5, with_greedy=True)
    greedy = greedy.contiguous()
    N = greedy.shape[0]
    f = _fwd(gpu, mdl, video, greedy, mask, vid, sid, 1.0)
    assert torch.equal(f["generated"], greedy)
    logits_tf, _ = gpu.teacher_forced_fwd(mdl.dims, mdl.store.params, video, greedy, N, 1.0, ac.DROP_SEED, vid, sid)
    assert torch.equal(f["logits"], logits_tf)
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


def _check_update_against_autograd(gpu, oracle, name, rel, precision="fp32"):
    """averaged_update(lr = 0, no weight decay, so that an untouched row of Wemb stays an exact zero) against float64 autograd over the
    restated graph with the same dropout masks, the device's picks -- asserted equal to the restatement's first -- as constants."""
    mdl, video, cap, mask, vid, sid = _model(oracle, name, decay=0.0)
    mdl.set_step(0)
    if name == "split":
        p, d, v, gt, hm, hv, hs = ac.tiled_case(oracle, SPLIT_DIMS, SPLIT_B, SPLIT_REP)
        v = np.tile(v, (SPLIT_REP, 1, 1))
    else:
        p, d, v, gt, hm, hv, hs = ac.case(oracle, name)
    dseed = mdl.dropout_seed + 104729 * mdl.global_step
    r = ac.averaged_unroll(oracle, p, d, v, gt, hm, hv, hs, keep=0.9, drop_seed=dseed, loss_weight=mdl.loss_weight)
    ac.assert_visible(r)
    ref_loss, ref_g = ac.autograd(p, v, gt, hm, r, 0.9, mdl.loss_weight, 0.0)
    saved = mdl.grad_precision
    mdl.grad_precision = precision
    try:
        st = mdl.averaged_update(video, cap, mask, lr=0.0, clip_norm=10.0)
    finally:
        mdl.grad_precision = saved
    assert np.array_equal(st.generated.cpu().numpy(), r["generated"]) and float(st.mask_sum) == r["mask_sum"]
    print(f"loss {float(st.loss)!r} reference {ref_loss!r}")
    assert abs(float(st.loss) - ref_loss) < 1e-4 * max(1.0, abs(ref_loss))
    got = {n: mdl.store.g[n].cpu().numpy() for n in mdl.store.names}
    _grad_check(got, ref_g, rel)
    # rows of Wemb that only the second scatter reaches: non-zero on both sides; a row nobody read: an exact zero
    rows = ac.only_picked_rows(r)
    assert rows
    for k in rows:
        assert np.abs(ref_g["Wemb"][k]).max() > 0 and np.abs(got["Wemb"][k]).max() > 0, k
    untouched = sorted(set(range(d.n_words)) - set(np.unique(r["ida"]).tolist()) - set(np.unique(r["idb"]).tolist()))
    assert untouched and not got["Wemb"][untouched].any() and not ref_g["Wemb"][untouched].any()
    gn = sum((g ** 2).sum() for g in ref_g.values())
    assert abs(float(st.grad_sumsq) - gn) <= 1e-3 * gn
    assert gpu.chain_timeouts() == 0
    return mdl


@pytest.mark.parametrize("name", ["small-odd", "odd-width"])
def test_update_gradients_vs_float64_autograd(gpu, oracle, name):
    """N <= 256 rows: the fp32 MFMA products."""
    assert not gpu.split_grad_active(ac.SHAPES[name][1])
    _check_update_against_autograd(gpu, oracle, name, 2e-4)


def test_update_gradients_vs_float64_autograd_split_products(gpu, oracle):
    """264 rows: the default split-bf16 products (skipped over to the fp32 bound when S2VT_SPLIT_GRADS=0 keeps them off).  Bound: 5e-5 of the
    tensor's largest entry, what tests/test_gpu_split_fused.py::test_fused_update_matches_unfused allows the same products between their two
    operand layouts -- tighter than the fp32 body's 2e-4, which these three-product sums stay well inside."""
    on = gpu.split_grad_active(SPLIT_B * SPLIT_REP)
    _check_update_against_autograd(gpu, oracle, "split", 5e-5 if on else 2e-4)


def test_fp32_products_at_the_split_row_count(gpu, oracle):
    """ops.averaged_bptt_bwd(products="fp32") at 264 rows: s2vt_averaged_bptt_bwd's precision 0, the fp32 MFMA set, agrees with the default
    set of that row count within the fp32 bound."""
    import torch
    mdl, video, cap, mask, vid, sid = _model(oracle, "split", decay=0.0)
    N = cap.shape[0]
    f = _fwd(gpu, mdl, video, cap, mask, vid, sid, 0.9)
    dlogits = f["logits"].clone()
    gpu.softmax_nll_fwd_bwd(dlogits, f["target_tm"], f["coef_tm"], 0.0)
    grads = []
    for products in ("fp32", None):
        gpu.zero_(mdl.store.grad)
        gpu.averaged_bptt_bwd(mdl.dims, mdl.store.params, mdl.store.grads, video, N, dlogits.clone(), f["ws"], f["scratch"], 0.9, ac.DROP_SEED, vid, sid,
                              products=products)
        grads.append({n: mdl.store.g[n].cpu().numpy().copy() for n in mdl.store.names})
    assert max(np.abs(g).max() for g in grads[0].values()) > 0
    _grad_check(grads[1], grads[0], 2e-4)


def test_bf16_precision_passes_its_bound(gpu, oracle):
    """S2VT_GRAD_PRECISION=bf16 / grad_precision = "bf16": the same substitution of the embedding operand in the bf16 product set, under
    tests/test_gpu_bf16_grads.py's GRAD_TOL (1e-2 of the tensor's largest entry)."""
    _check_update_against_autograd(gpu, oracle, "small-odd", 1e-2, precision="bf16")


# ---------------------------------------------------------------------------------------------------------------- 4. the two-index scatter
@pytest.mark.parametrize("R,E,ld,V", [(0, 8, 8, 5), (1, 1, 1, 3), (7, 24, 24, 11), (9, 25, 40, 6), (150, 20, 84, 37), (300, 65, 65, 4)])
def test_embed_scatter_add2_in_guard_bands(gpu, R, E, ld, V):
    """dW[a[r]] += s dE[r] and dW[b[r]] += s dE[r] against float64: equal ids (both additions land), repeated ids, R = 0, row strides
    wider than E.  fp32 atomic sums of at most 2 R terms: 1e-6 of the largest |term| sum per element."""
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    rng = np.random.default_rng(R * 131 + E)
    Rr = max(R, 1)
    dE = rng.standard_normal((Rr, ld)).astype(np.float32)
    a = rng.integers(0, V, Rr).astype(np.int32)
    b = rng.integers(0, V, Rr).astype(np.int32)
    b[::3] = a[::3]                                                  # equal pairs
    if R > 2:
        a[1] = a[0]; b[2] = a[0]                                     # repeats across rows
    W0 = rng.standard_normal((V, E)).astype(np.float32)
    scale = 0.5
    ref = W0.astype(np.float64)
    mag = np.abs(W0).astype(np.float64)
    for r in range(R):
        for k in (a[r], b[r]):
            ref[k] += scale * dE[r, :E].astype(np.float64)
            mag[k] += scale * np.abs(dE[r, :E])
    dEg = Guarded.of(dE, lead=65, name="dE")
    ag, bg = Guarded.of(a, lead=65, name="idx_a", fill=0), Guarded.of(b, lead=67, name="idx_b", fill=0)
    Wg = Guarded.of(W0, lead=66, name="dWemb")
    rc = L.s2vt_embed_scatter_add2(dEg.ptr, ld, ag.ptr, bg.ptr, scale, R, E, Wg.ptr, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    got = Wg.numpy().astype(np.float64)
    assert np.all(np.abs(got - ref) <= 1e-6 * mag)
    if R == 0:
        assert np.array_equal(Wg.numpy(), W0)
    else:
        assert np.abs(got - W0).max() > 0
    for g in (dEg, ag, bg, Wg):
        g.assert_intact()
    assert np.array_equal(dEg.numpy(), dE)


def test_embed_scatter_add2_wrapper_on_a_strided_view(gpu):
    import torch
    rng = np.random.default_rng(5)
    full = torch.as_tensor(rng.standard_normal((12, 30)).astype(np.float32)).cuda()
    dE = full[:, 6:26]                                               # a row-strided view, as the embed slice of dX2 is
    a = torch.as_tensor(rng.integers(0, 7, 12).astype(np.int32)).cuda()
    W = torch.zeros(7, 20, device="cuda")
    gpu.embed_scatter_add2(dE, a, a, W, scale=0.5)                   # both halves into the same row: the plain scatter-add
    ref = torch.zeros(7, 20, dtype=torch.float64, device="cuda").index_add_(0, a.long(), dE.double())
    assert float((W.double() - ref).abs().max()) <= 1e-6 * float(dE.abs().sum())


# ---------------------------------------------------------------------------------------------------------------- 5. workspace and scratch
@pytest.mark.parametrize("name", ["small-odd", "many-rows"])
def test_outputs_workspace_and_scratch_stay_inside_their_buffers(gpu, oracle, name):
    """Every output in guard bands; the training workspace and the scratch at exactly their declared sizes, both dirtied first (nothing
    may rely on what a buffer held); forward and backward then give the restatement's values and the default buffers' gradients.  A
    scratch 256 bytes short is refused by both entries before any launch."""
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    mdl, video, cap, mask, vid, sid = _model(oracle, name)
    N, Tc = cap.shape
    V = mdl.dims.n_words
    B = video.shape[0]
    r = _ref(oracle, name, 0.9)
    ac.assert_visible(r)
    out = dict(generated=Guarded(N, Tc, dtype=torch.int32, lead=65, name="generated"), coef_tm=Guarded(1, Tc * N, lead=66, name="coef_tm"),
               target_tm=Guarded(1, Tc * N, dtype=torch.int32, lead=65, name="target_tm"), logits=Guarded(Tc * N, V, lead=68, name="logits"),
               mask_sum=Guarded(1, 1, lead=65, name="mask_sum"), mask_sum_copy=Guarded(1, 1, lead=69, name="mask_sum_copy"))
    capg = Guarded.of(cap.cpu().numpy(), lead=65, name="caption", fill=2)
    maskg = Guarded.of(mask.cpu().numpy(), lead=67, name="mask")
    vidg = Guarded.of(vid.cpu().numpy(), lead=65, name="video_id", fill=0)
    sidg = Guarded.of(sid.cpu().numpy(), lead=65, name="sample_id", fill=0)
    ws_bytes = L.s2vt_train_workspace_bytes(ctypes.byref(mdl.dims), B, N)
    sc_bytes = L.s2vt_averaged_scratch_bytes(ctypes.byref(mdl.dims), N)
    ws, scr = GuardedWorkspace(ws_bytes, name="workspace"), GuardedWorkspace(sc_bytes, name="scratch")
    ws.window.fill_(0xA5); scr.window.fill_(0xFF)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd(scratch_bytes):
        return L.s2vt_averaged_fwd(ctypes.byref(mdl.dims), ctypes.byref(mdl.store.params), vp(video), B, N, capg.ptr, maskg.ptr, 1.0, 0.9, ac.DROP_SEED,
                                   vidg.ptr, sidg.ptr, out["logits"].ptr, out["generated"].ptr, out["coef_tm"].ptr, out["target_tm"].ptr,
                                   out["mask_sum"].ptr, out["mask_sum_copy"].ptr, ws.ptr, ws_bytes, scr.ptr, scratch_bytes, stream)

    def bwd(dlogits, scratch_bytes):
        return L.s2vt_averaged_bptt_bwd(ctypes.byref(mdl.dims), ctypes.byref(mdl.store.params), ctypes.byref(mdl.store.grads), vp(video), B, N,
                                        vp(dlogits), 0.9, ac.DROP_SEED, vidg.ptr, sidg.ptr, ws.ptr, ws_bytes, scr.ptr, scratch_bytes, 0, None, 0, stream)
    assert fwd(sc_bytes - 256) == -3                                 # S2VT_E_WORKSPACE, nothing launched
    assert bool((scr.window == 0xFF).all()) and bool((ws.window == 0xA5).all())
    assert fwd(sc_bytes) == 0
    assert np.array_equal(out["generated"].numpy(), r["generated"])
    for k in ("coef_tm", "target_tm"):
        assert np.array_equal(out[k].numpy().ravel(), r[k]), k
    assert np.array_equal(out["logits"].numpy(), r["logits"])
    assert out["mask_sum"].numpy().item() == r["mask_sum"] == out["mask_sum_copy"].numpy().item()
    dlogits = torch.as_tensor(r["logits"]).cuda()
    coef, tgt = torch.as_tensor(r["coef_tm"]).cuda(), torch.as_tensor(r["target_tm"]).cuda()
    gpu.softmax_nll_fwd_bwd(dlogits, tgt, coef, 0.0)
    assert bwd(dlogits, sc_bytes - 256) == -3
    gpu.zero_(mdl.store.grad)
    assert bwd(dlogits.clone(), sc_bytes) == 0
    guarded = {n: mdl.store.g[n].cpu().numpy().copy() for n in mdl.store.names}
    for g in list(out.values()) + [capg, maskg, vidg, sidg, ws, scr]:
        g.assert_intact()
    # the same pass on the cached default buffers
    f = _fwd(gpu, mdl, video, cap, mask, vid, sid, 0.9)
    gpu.zero_(mdl.store.grad)
    gpu.averaged_bptt_bwd(mdl.dims, mdl.store.params, mdl.store.grads, video, N, dlogits.clone(), f["ws"], f["scratch"], 0.9, ac.DROP_SEED, vid, sid,
                          products="fp32")
    plain = {n: mdl.store.g[n].cpu().numpy().copy() for n in mdl.store.names}
    assert max(np.abs(g).max() for g in plain.values()) > 0
    _grad_check(guarded, plain, 2e-4)
    assert gpu.chain_timeouts() == 0


# ---------------------------------------------------------------------------------------------------------------- 6. the update
def test_per_variable_clip_and_sgd_three_steps(gpu, oracle):
    """train() of :368-371: tf.clip_by_norm(grad, 10) per variable, then GradientDescentOptimizer -- against a float64 replay on the
    gradients the device left in the bucket, three steps, rtol 2e-5 / atol 2e-6 (test_gpu_scheduled.py::test_sgd_three_steps_in_guard_bands').
    The loss weight is set so that 10 lies between the two largest per-variable norms: the clip acts on one variable alone."""
    import torch
    from s2vt_amd import model as M
    dims, B = ac.SHAPES["small-odd"]
    p, d, v, gt, hm, hv, hs = ac.case(oracle, "small-odd")
    mdl = M.Video_Caption_Generator(dims["dim_image"], dims["n_words"], dims["word_dim"], dims["lstm_dim"], B, 0, dims["n_video_lstm_step"],
                                    dims["n_caption_lstm_step"], seed=3, multisample=1, dropout_rate=0.9)
    mdl.store.load(p)
    video, cap, mask = torch.as_tensor(v).cuda(), torch.as_tensor(gt).cuda(), torch.as_tensor(hm).cuda()
    names = mdl.store.names
    probe = mdl.averaged_update(video, cap, mask, lr=0.0)
    assert mdl.global_step == 1
    norms = sorted(float(probe.var_sumsq[n]) ** 0.5 for n in names)
    assert norms[-1] > norms[-2] > 0
    mdl.loss_weight = 10.0 / (norms[-1] * norms[-2]) ** 0.5          # (weight decay's share of the norms is negligible at 5e-5)
    m0, v0, t0 = mdl.store.m.clone(), mdl.store.v.clone(), mdl.adam_t
    lr = 0.01
    for it in range(3):
        before = {n: mdl.store.p[n].cpu().numpy().astype(np.float64) for n in names}
        st = mdl.averaged_update(video, cap, mask, lr=lr, clip_norm=10.0, clip="per_variable", optimizer="sgd")
        clipped = []
        total = 0.0
        for n in names:
            g = mdl.store.g[n].cpu().numpy().astype(np.float64)
            sumsq = float((g ** 2).sum())
            total += sumsq
            assert abs(float(st.var_sumsq[n]) - sumsq) <= 1e-5 * sumsq + 1e-30, n
            nrm = sumsq ** 0.5
            if nrm > 10.0:
                clipped.append(n)
            want = before[n] - lr * g * (10.0 / max(nrm, 10.0))
            got = mdl.store.p[n].cpu().numpy()
            assert np.allclose(got, want, rtol=2e-5, atol=2e-6), n
            assert np.abs(got - before[n]).max() > 0, n
        print(f"step {it}: clipped {clipped}, loss {float(st.loss)!r}")
        assert len(clipped) == 1, clipped                            # the clip acts on that variable alone
        assert abs(float(st.grad_sumsq) - total) <= 1e-5 * total
        assert mdl.global_step == it + 2
    assert torch.equal(mdl.store.m, m0) and torch.equal(mdl.store.v, v0) and mdl.adam_t == t0
    assert gpu.chain_timeouts() == 0


def test_global_clip_and_adam_go_through_apply_gradients(gpu, oracle):
    """clip="global" + SGD: one norm over all variables; optimizer="adam": Adam's moments and count move."""
    import torch
    mdl, video, cap, mask, vid, sid = _model(oracle, "small-odd")
    mdl.set_step(0)
    before = mdl.store.theta.clone()
    m0, t0 = mdl.store.m.clone(), mdl.adam_t
    try:
        st = mdl.averaged_update(video, cap, mask, lr=0.5, clip_norm=1e-3, clip="global", optimizer="sgd")
        assert st.var_sumsq is None
        g = mdl.store.grad[:mdl.store.numel].double()
        nrm = float(st.grad_sumsq) ** 0.5
        assert nrm > 1e-3                                            # the global clip acts
        want = before.double() - 0.5 * g * (1e-3 / nrm)
        assert np.allclose(mdl.store.theta.cpu().numpy(), want.cpu().numpy(), rtol=2e-5, atol=2e-6)
        assert torch.equal(mdl.store.m, m0) and mdl.adam_t == t0
        mdl.averaged_update(video, cap, mask, lr=1e-4, optimizer="adam")
        assert mdl.adam_t == t0 + 1 and not torch.equal(mdl.store.m, m0)
        with pytest.raises(ValueError):
            mdl.averaged_update(video, cap, mask, lr=0.0, clip="per_row")
        with pytest.raises(ValueError):
            mdl.averaged_update(video, cap, mask, lr=0.0, optimizer="momentum")
        with pytest.raises(ValueError):
            mdl.averaged_update(video, cap[:, :-1].contiguous(), mask, lr=0.0)
    finally:
        mdl.store.theta.copy_(before)
        mdl.store.m.copy_(m0); mdl.store.v.zero_()
        mdl.set_step(0)
        mdl.adam_t = t0


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_residual_model_is_refused(gpu):
    import torch
    from s2vt_amd import model as M
    mdl = M.Video_Caption_Generator(64, 131, 24, 32, 5, 0, 3, 9, multisample=1, residual=True)
    video = torch.zeros(5, 3, 64, device="cuda")
    cap = torch.full((5, 9), 2, dtype=torch.int32, device="cuda")
    mask = torch.ones(5, 9, device="cuda")
    with pytest.raises(ValueError):
        mdl.averaged_update(video, cap, mask, lr=0.0)
    with pytest.raises(ValueError):
        mdl.build_averaged_model()
    import s2vt_amd
    assert s2vt_amd.lib().s2vt_averaged_scratch_bytes(ctypes.byref(mdl.dims), 5) == 0
