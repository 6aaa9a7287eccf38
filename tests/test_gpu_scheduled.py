"""Scheduled-sampling training (generate_words_tf_s2vt.py:101-211,412-418): s2vt_scheduled_fwd / ops.scheduled_fwd,
Video_Caption_Generator.scheduled_update, s2vt_sgd_guarded / ops.sgd.

The reference values come from tests/scheduled_cases.py: a restatement of the unroll from the C oracle's pieces, on shapes whose <eos>
bias was chosen on the CPU so that the coin, the fed word and the running mask of quirk SQ1 all show in the result (every parity test
asserts that first, on the restatement).  Ids, masks and logits are compared with array_equal; gradients with the tolerances of
tests/test_gpu_train.py::test_gradients_vs_float64_autograd."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import scheduled_cases as sc
from guardband import Guarded

pytestmark = pytest.mark.gpu

_models = {}
_refs = {}


def _model(oracle, name, keep=0.9):
    """A model holding the case's parameters (bias included), and the device video: built once per (shape, keep)."""
    key = (name, keep)
    if key not in _models:
        import torch
        from s2vt_amd import model as M
        dims, B = sc.SHAPES[name]
        p, d, video, gt, vid, sid = sc.case(oracle, name)
        mdl = M.Video_Caption_Generator(dims["dim_image"], dims["n_words"], dims["word_dim"], dims["lstm_dim"], B, 0, dims["n_video_lstm_step"],
                                        dims["n_caption_lstm_step"], seed=sc.PARAM_SEED, multisample=1, dropout_rate=keep)
        mdl.store.load(p)
        _models[key] = (mdl, torch.as_tensor(video).cuda(), torch.as_tensor(gt).cuda(), torch.as_tensor(vid).cuda(), torch.as_tensor(sid).cuda())
    return _models[key]


def _ref(oracle, name, prob, seed, keep, loss_weight=1.0):
    """The restatement's result of a case: computed once, shared, never written to."""
    key = (name, prob, seed, keep, loss_weight)
    if key not in _refs:
        p, d, video, gt, vid, sid = sc.case(oracle, name)
        _refs[key] = sc.scheduled_unroll(oracle, p, d, video, gt, sc.p_gt_of(prob), seed, vid, sid, keep=keep, loss_weight=loss_weight)
    return _refs[key]


def _fwd(gpu, mdl, video, cap, vid, sid, prob, seed, keep, loss_weight=1.0, ws=None):
    return gpu.scheduled_fwd(mdl.dims, mdl.store.params, video, cap, cap.shape[0], float(sc.p_gt_of(prob)), seed, loss_weight, keep, sc.DROP_SEED,
                             vid, sid, ws=ws)


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("keep", sc.KEEPS)
@pytest.mark.parametrize("prob", sc.PROBS)
@pytest.mark.parametrize("name", list(sc.SHAPES))
def test_forward_equals_the_restatement(gpu, oracle, name, prob, keep):
    mdl, video, cap, vid, sid = _model(oracle, name)
    for seed in sc.SEEDS:
        r = _ref(oracle, name, prob, seed, keep)
        sc.assert_visible(r)
        f = _fwd(gpu, mdl, video, cap, vid, sid, prob, seed, keep)
        for k in ("generated", "fed", "mask", "coef_tm", "target_tm"):
            assert np.array_equal(f[k].cpu().numpy(), r[k]), k
        assert np.array_equal(f["logits"].cpu().numpy(), r["logits"])
        assert float(f["mask_sum"]) == r["mask_sum"]
    assert gpu.chain_timeouts() == 0


def test_loss_weight_scales_the_coefficients(gpu, oracle):
    mdl, video, cap, vid, sid = _model(oracle, "small-odd")
    r = _ref(oracle, "small-odd", 0.5, sc.SEEDS[0], 0.9, loss_weight=0.3)
    f = _fwd(gpu, mdl, video, cap, vid, sid, 0.5, sc.SEEDS[0], 0.9, loss_weight=0.3)
    assert np.array_equal(f["coef_tm"].cpu().numpy(), r["coef_tm"]) and np.array_equal(f["mask"].cpu().numpy(), r["mask"])
    assert set(np.unique(r["coef_tm"])) == {np.float32(0.0), np.float32(0.3)}


def test_coin_follows_the_sample_id(gpu, oracle):
    """Counter (0, video, sample, step): rows of another sample id draw other coins; the restatement with those ids agrees."""
    import torch
    mdl, video, cap, vid, sid = _model(oracle, "one-tile")
    p, d, v, gt, hv, hs = sc.case(oracle, "one-tile")
    hs2 = (np.arange(len(hs)) % 3 + 1).astype(np.int32)
    r = sc.scheduled_unroll(oracle, p, d, v, gt, sc.p_gt_of(0.5), sc.SEEDS[1], hv, hs2, keep=1.0)
    sc.assert_visible(r)
    f = gpu.scheduled_fwd(mdl.dims, mdl.store.params, video, cap, cap.shape[0], float(sc.p_gt_of(0.5)), sc.SEEDS[1], 1.0, 1.0, sc.DROP_SEED, vid,
                          torch.as_tensor(hs2).cuda())
    assert np.array_equal(f["fed"].cpu().numpy(), r["fed"]) and np.array_equal(f["generated"].cpu().numpy(), r["generated"])
    assert not np.array_equal(r["coin"], _ref(oracle, "one-tile", 0.5, sc.SEEDS[1], 1.0)["coin"])


# ---------------------------------------------------------------------------------------------------------------- 2. the mixed decode
@pytest.mark.parametrize("name", ["small-odd", "one-tile", "chain-range", "many-rows"])
def test_generated_equals_the_mixed_sampler(gpu, oracle, name):
    """keep = 1, sample id 0: the same coins, the same fed words, the same picks as mix_sample's already-verified decode."""
    mdl, video, cap, vid, sid = _model(oracle, name)
    for prob in sc.PROBS:
        seed = sc.SEEDS[1]
        sc.assert_visible(_ref(oracle, name, prob, seed, 1.0))
        f = _fwd(gpu, mdl, video, cap, vid, sid, prob, seed, 1.0)
        mix, _ = mdl.mix_sample(video, cap, prob, False, seed=seed)
        assert np.array_equal(f["generated"].cpu().numpy(), mix.cpu().numpy())
    assert gpu.chain_timeouts() == 0


# ---------------------------------------------------------------------------------------------------------------- 3. the workspace contract
def _grad_check(got, want, what=""):
    """tests/test_gpu_train.py::test_gradients_vs_float64_autograd's per-tensor bound: 2e-4 of the largest reference entry + 1e-9."""
    for n in want:
        g, w = np.asarray(got[n], np.float64), np.asarray(want[n], np.float64)
        scale = np.abs(w).max() + 1e-12
        err = np.abs(g - w).max()
        print(f"{what}{n}: max |diff| = {err:.3e}, largest reference entry = {scale:.3e}")
        assert err <= 2e-4 * scale + 1e-9, (n, err, scale)


@pytest.mark.parametrize("keep", sc.KEEPS)
@pytest.mark.parametrize("name", ["small-odd", "one-tile", "chain-range"])
def test_workspace_is_the_teacher_forced_one_for_the_fed_words(gpu, oracle, name, keep):
    import torch
    mdl, video, cap, vid, sid = _model(oracle, name)
    N = cap.shape[0]
    sc.assert_visible(_ref(oracle, name, 0.5, sc.SEEDS[0], keep))
    nb = gpu.train_workspace(mdl.dims, video.shape[0], N, video.device).numel()
    ws_a, ws_b = (torch.empty(nb, dtype=torch.uint8, device="cuda") for _ in range(2))
    f = _fwd(gpu, mdl, video, cap, vid, sid, 0.5, sc.SEEDS[0], keep, ws=ws_a)
    fed = f["fed"]
    # a caption whose previous-word sequence is `fed`: column t holds the word fed at step t + 1 (the last column feeds nothing)
    cap_fed = torch.cat([fed[:, 1:], cap[:, -1:]], 1).contiguous()
    logits_tf, _ = gpu.teacher_forced_fwd(mdl.dims, mdl.store.params, video, cap_fed, N, keep, sc.DROP_SEED, vid, sid, ws=ws_b)
    assert torch.equal(logits_tf, f["logits"])
    dlogits = f["logits"].clone()
    gpu.softmax_nll_fwd_bwd(dlogits, f["target_tm"], f["coef_tm"], 0.0)
    grads = []
    for ws in (ws_a, ws_b):
        gpu.zero_(mdl.store.grad)
        gpu.bptt_bwd(mdl.dims, mdl.store.params, mdl.store.grads, video, N, dlogits.clone(), ws, keep, sc.DROP_SEED, vid, sid)
        grads.append({n: mdl.store.g[n].cpu().numpy().copy() for n in mdl.store.names})
    assert max(np.abs(g).max() for g in grads[1].values()) > 0
    _grad_check(grads[0], grads[1])
    assert gpu.chain_timeouts() == 0


# ---------------------------------------------------------------------------------------------------------------- 4. gradients
def _autograd(oracle, name, r, keep, loss_weight, decay):
    import torch
    from oracle import s2vt_torch as T
    p, d, video, gt, vid, sid = sc.case(oracle, name)
    pt = T.to_torch(p, torch.float64, True)
    fed = torch.as_tensor(r["fed"]).long()
    logits = T.unroll(pt, torch.as_tensor(video).double(), lambda t, _: fed[:, t], gt.shape[1], r["drop"], keep)        # [N, Tc, V]
    lp = torch.log_softmax(logits, -1)
    ce = -lp.gather(2, torch.as_tensor(gt).long().unsqueeze(-1)).squeeze(-1)                                            # [N, Tc]
    mask = torch.as_tensor(r["mask"]).double()
    wd = sum(0.5 * (v ** 2).sum() for k, v in pt.items() if k not in ("lstm1_b", "lstm2_b"))
    loss = loss_weight * (ce * mask).sum() / mask.sum() + decay * wd                                                   # :198-210
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in pt.items()}


def _check_update_against_autograd(gpu, oracle, name):
    from s2vt_amd import model as M
    keep, prob, seed = 0.9, 0.5, sc.SEEDS[0]
    mdl, video, cap, vid, sid = _model(oracle, name)
    mdl.set_step(0)
    p, d, v, gt, hv, hs = sc.case(oracle, name)
    dseed = mdl.dropout_seed + 104729 * mdl.global_step
    r = sc.scheduled_unroll(oracle, p, d, v, gt, sc.p_gt_of(prob), seed, hv, hs, keep=keep, drop_seed=dseed)
    sc.assert_visible(r)
    ref_loss, ref_g = _autograd(oracle, name, r, keep, mdl.loss_weight, mdl.decay_value)
    st = mdl.scheduled_update(video, cap, lr=0.0, true_word_prob=prob, clip_norm=10.0, coin_seed=seed)
    assert np.array_equal(st.fed.cpu().numpy(), r["fed"]) and np.array_equal(st.mask.cpu().numpy(), r["mask"])
    assert np.array_equal(st.generated.cpu().numpy(), r["generated"]) and float(st.mask_sum) == r["mask_sum"]
    wd = sum(0.5 * float((mdl.store.p[n].double() ** 2).sum()) for n in mdl.store.names if n not in M.UNDECAYED)
    loss = float(st.loss) + mdl.decay_value * wd
    print(f"loss {loss!r} reference {ref_loss!r}")
    assert abs(loss - ref_loss) < 1e-4 * max(1.0, abs(ref_loss))
    _grad_check({n: mdl.store.g[n].cpu().numpy() for n in mdl.store.names}, ref_g)
    gn = sum((g ** 2).sum() for g in ref_g.values())
    print(f"grad_sumsq {float(st.grad_sumsq)!r} reference {gn!r}")
    assert abs(float(st.grad_sumsq) - gn) <= 1e-3 * gn
    assert gpu.chain_timeouts() == 0
    return mdl


@pytest.mark.parametrize("name", ["small-odd", "one-tile"])
def test_update_gradients_vs_float64_autograd(gpu, oracle, name):
    """scheduled_update(lr = 0) against float64 autograd over the restated graph fed the words that were fed, with the same dropout masks
    and the loss of :198-210.  Run with the process's gradient precision; when that is the split form at this row count, once more with
    S2VT_SPLIT_GRADS=0 in a fresh child process (the switch is read once per process)."""
    mdl = _check_update_against_autograd(gpu, oracle, name)
    if gpu.split_grad_active(sc.SHAPES[name][1]) and os.environ.get("S2VT_SPLIT_GRADS") != "0":
        env = dict(os.environ, S2VT_SPLIT_GRADS="0")
        me = f"{os.path.abspath(__file__)}::test_update_gradients_vs_float64_autograd[{name}]"
        out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", me], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------------------- 5. p_gt = 1
@pytest.mark.parametrize("name", ["small-odd", "one-tile"])
def test_always_truth_is_the_cross_entropy_update(gpu, oracle, name):
    """p_gt = 1 feeds the caption: logits, loss and gradients are xe_update(q1=False, smoothing=0)'s on the same caption under the same
    device-made mask."""
    import torch
    from s2vt_amd import model as M
    dims, B = sc.SHAPES[name]
    p, d, v, gt, hv, hs = sc.case(oracle, name)
    mk = lambda: M.Video_Caption_Generator(dims["dim_image"], dims["n_words"], dims["word_dim"], dims["lstm_dim"], B, 0, dims["n_video_lstm_step"],
                                           dims["n_caption_lstm_step"], seed=sc.PARAM_SEED, multisample=1, dropout_rate=0.9)
    a, b = mk(), mk()
    a.store.load(p); b.store.load(p)
    video, cap = torch.as_tensor(v).cuda(), torch.as_tensor(gt).cuda()
    dseed = a.dropout_seed + 104729 * a.global_step
    r = sc.scheduled_unroll(oracle, p, d, v, gt, np.float32(1.0), 5, hv, hs, keep=0.9, drop_seed=dseed)
    assert (r["mask"] == 0).any() and (r["mask"] == 1).any()                       # the mask is not trivial
    a._keep_scheduled_logits = True
    sa = a.scheduled_update(video, cap, lr=0.0, true_word_prob=1.00001, clip_norm=10.0, coin_seed=5)
    assert np.array_equal(sa.fed.cpu().numpy()[:, 1:], gt[:, :-1]) and np.array_equal(sa.mask.cpu().numpy(), r["mask"])
    vid, sid = a._row_ids(B, 1, 0)
    logits_tf, _ = gpu.teacher_forced_fwd(b.dims, b.store.params, video, cap, B, 0.9, dseed, vid, sid)
    assert torch.equal(a.last_scheduled["probs"], logits_tf)
    assert np.array_equal(logits_tf.cpu().numpy(), r["logits"])
    sb = b.xe_update(video, cap, sa.mask, lr=0.0, clip_norm=10.0, q1=False, smoothing=0.0)
    print(f"loss scheduled {float(sa.loss)!r} xe {float(sb.loss)!r}")
    assert abs(float(sa.loss) - float(sb.loss)) < 1e-4 * max(1.0, abs(float(sb.loss)))
    _grad_check({n: a.store.g[n].cpu().numpy() for n in a.store.names}, {n: b.store.g[n].cpu().numpy() for n in b.store.names})
    assert abs(float(sa.grad_sumsq) - float(sb.grad_sumsq)) <= 1e-3 * float(sb.grad_sumsq)
    assert gpu.chain_timeouts() == 0


# ---------------------------------------------------------------------------------------------------------------- 6. zero mask
def test_zero_mask_forward(gpu, oracle):
    """A bias so large that every row picks <eos> at step 0: the mask and the coefficients are all zeros, sum(mask) = 0 (the reference's
    0/0 is the caller's to see), and the fed words still follow the coins."""
    import torch
    mdl, video, cap, vid, sid = _model(oracle, "small-odd")
    p, d, v, gt, hv, hs = sc.case(oracle, "small-odd")
    big = {k: a.copy() for k, a in p.items()}
    big["embed_word_b"][0] += np.float32(50.0)
    r = sc.scheduled_unroll(oracle, big, d, v, gt, sc.p_gt_of(0.5), sc.SEEDS[0], hv, hs, keep=0.9)
    assert (r["generated"] == 0).all() and r["mask_sum"] == 0 and r["coin"][:, 1:].any() and not r["coin"][:, 1:].all()
    saved = mdl.store.p["embed_word_b"].clone()
    try:
        mdl.store.load({"embed_word_b": big["embed_word_b"]})
        f = _fwd(gpu, mdl, video, cap, vid, sid, 0.5, sc.SEEDS[0], 0.9)
        assert float(f["mask"].abs().max()) == 0 and float(f["coef_tm"].abs().max()) == 0 and float(f["mask_sum"]) == 0
        assert np.array_equal(f["fed"].cpu().numpy(), r["fed"]) and np.array_equal(f["generated"].cpu().numpy(), r["generated"])
        assert np.array_equal(f["fed"].cpu().numpy()[:, 1:] != 0, r["coin"][:, 1:])     # truth (>= 2) where the coin says so, <eos> elsewhere
    finally:
        mdl.store.p["embed_word_b"].copy_(saved)
    assert gpu.chain_timeouts() == 0


# ---------------------------------------------------------------------------------------------------------------- 7. SGD
@pytest.mark.parametrize("lead", [64, 65])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_sgd_three_steps_in_guard_bands(gpu, n, lead):
    """theta -= lr * g * clip / max(sqrt(sumsq), clip) against float64, three steps: not clipped, clipped, clipping off (clip_norm = 0).
    lead 65: neither buffer is 16-byte aligned (the scalar path)."""
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    rng = np.random.default_rng(n)
    theta0 = rng.standard_normal(n).astype(np.float32)
    th = Guarded.of(theta0, lead=lead, name="theta")
    ref = theta0.astype(np.float64)
    applied = torch.zeros(1, dtype=torch.int32, device="cuda")
    lr = 0.05
    for step, (amp, clip) in enumerate([(0.01, 10.0), (100.0, 10.0), (100.0, 0.0)], start=1):
        g = (rng.standard_normal(n) * amp).astype(np.float32)
        sumsq = float((g.astype(np.float64) ** 2).sum())
        nrm = np.sqrt(sumsq)
        if step == 2:
            assert nrm > clip
        s = clip / max(nrm, clip) if clip > 0 else 1.0
        ref = ref - lr * g.astype(np.float64) * s
        gd = Guarded.of(g, lead=lead, name="g")
        sq = torch.full((1,), sumsq, dtype=torch.float32, device="cuda")
        rc = L.s2vt_sgd_guarded(th.ptr, gd.ptr, n, ctypes.c_void_p(sq.data_ptr()), clip, lr, step, ctypes.c_void_p(applied.data_ptr()),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        assert np.allclose(th.numpy().ravel(), ref, rtol=2e-5, atol=2e-6)
        assert np.array_equal(gd.numpy().ravel(), g)                                   # the gradient is read only
        th.assert_intact(); gd.assert_intact()
        assert int(applied.item()) == step
    assert np.abs(th.numpy().ravel() - theta0).max() > 0


def test_sgd_optimizer_leaves_adam_alone(gpu, oracle):
    """apply_gradients(optimizer="sgd") through scheduled_update: the variables move by -lr * clipped gradient, m / v / adam_t stay."""
    import torch
    mdl, video, cap, vid, sid = _model(oracle, "small-odd")
    mdl.set_step(0)
    before = mdl.store.theta.clone()
    m0, v0, t0 = mdl.store.m.clone(), mdl.store.v.clone(), mdl.adam_t
    try:
        st = mdl.scheduled_update(video, cap, lr=0.5, true_word_prob=0.5, optimizer="sgd", coin_seed=sc.SEEDS[0])
        g = mdl.store.grad[:mdl.store.numel].double()
        nrm = float(st.grad_sumsq) ** 0.5
        want = before.double() - 0.5 * g * (10.0 / max(nrm, 10.0))
        assert np.allclose(mdl.store.theta.cpu().numpy(), want.cpu().numpy(), rtol=2e-5, atol=2e-6)
        assert float((mdl.store.theta - before).abs().max()) > 0
        assert torch.equal(mdl.store.m, m0) and torch.equal(mdl.store.v, v0) and mdl.adam_t == t0 and mdl.global_step == 1
        with pytest.raises(ValueError):
            mdl.apply_gradients(None, 0.0, 10.0, optimizer="momentum")
    finally:
        mdl.store.theta.copy_(before)
        mdl.set_step(0)


# ---------------------------------------------------------------------------------------------------------------- 8. guard bands
@pytest.mark.parametrize("name", ["small-odd", "many-rows"])
def test_outputs_stay_inside_their_buffers(gpu, oracle, name):
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    mdl, video, cap, vid, sid = _model(oracle, name)
    N, Tc = cap.shape
    V = mdl.dims.n_words
    r = _ref(oracle, name, 0.5, sc.SEEDS[1], 0.9)
    sc.assert_visible(r)
    out = dict(generated=Guarded(N, Tc, dtype=torch.int32, lead=65, name="generated"), fed=Guarded(N, Tc, dtype=torch.int32, lead=67, name="fed"),
               mask=Guarded(N, Tc, lead=65, name="mask"), coef_tm=Guarded(1, Tc * N, lead=66, name="coef_tm"),
               target_tm=Guarded(1, Tc * N, dtype=torch.int32, lead=65, name="target_tm"), logits=Guarded(Tc * N, V, lead=68, name="logits"),
               mask_sum=Guarded(1, 1, lead=65, name="mask_sum"), mask_sum_copy=Guarded(1, 1, lead=69, name="mask_sum_copy"))
    capg = Guarded.of(cap.cpu().numpy(), lead=65, name="caption", fill=2)
    vidg = Guarded.of(vid.cpu().numpy(), lead=65, name="video_id", fill=0)
    sidg = Guarded.of(sid.cpu().numpy(), lead=65, name="sample_id", fill=0)
    ws = gpu.train_workspace(mdl.dims, video.shape[0], N, video.device)
    scratch = gpu.workspace(L.s2vt_scheduled_scratch_bytes(ctypes.byref(mdl.dims), N), video.device, "scheduled")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.s2vt_scheduled_fwd(ctypes.byref(mdl.dims), ctypes.byref(mdl.store.params), vp(video), video.shape[0], N, capg.ptr, float(sc.p_gt_of(0.5)),
                              sc.SEEDS[1], 1.0, 0.9, sc.DROP_SEED, vidg.ptr, sidg.ptr, out["logits"].ptr, out["generated"].ptr, out["fed"].ptr,
                              out["mask"].ptr, out["coef_tm"].ptr, out["target_tm"].ptr, out["mask_sum"].ptr, out["mask_sum_copy"].ptr, vp(ws),
                              ws.numel(), vp(scratch), scratch.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    for k in ("generated", "fed", "mask"):
        assert np.array_equal(out[k].numpy(), r[k]), k
    for k in ("coef_tm", "target_tm"):
        assert np.array_equal(out[k].numpy().ravel(), r[k]), k
    assert np.array_equal(out["logits"].numpy(), r["logits"])
    assert out["mask_sum"].numpy().item() == r["mask_sum"] == out["mask_sum_copy"].numpy().item()
    for g in list(out.values()) + [capg, vidg, sidg]:
        g.assert_intact()
    assert gpu.chain_timeouts() == 0
