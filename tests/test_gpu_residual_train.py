"""The residual model's training half on the GPU (S2VT_MODEL_RESIDUAL): the teacher-forced logits bit for bit against the CPU
restatement of tests/residual_cases.py, and the backward -- dWout = s^T dlogits, ds into LSTM2 as before AND into LSTM1's dropped output
of the decode steps -- against float64 autograd of the restated graph, in the three precision modes, in phases, with live rows.

Bounds: max |g - ref| per tensor within 2e-4 of that tensor's largest reference entry with the fp32 and the
split-bf16 products, 1e-2 with bf16 operands; the loss within 1e-3."""
import numpy as np
import pytest

import residual_cases as RC

pytestmark = pytest.mark.gpu

KEEP = 0.9
TOL = {"fp32": 2e-4, "split": 2e-4, "bf16": 1e-2}


def _dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _rows(name, rep, B=None):
    """Captions with ragged ends (a first <eos> inside the caption), sample-major row ids."""
    dims, B0 = RC.SHAPES[name]
    B = B0 if B is None else B
    N, Tc, V = B * rep, dims["n_caption_lstm_step"], dims["n_words"]
    rng = np.random.default_rng(7 + N)
    cap = rng.integers(2, V, (N, Tc)).astype(np.int32)
    if Tc > 3:
        ln = rng.integers(2, Tc - 1, N)
        for n in range(N):
            cap[n, ln[n]:] = 0
        cap[0, :] = rng.integers(2, V, Tc)                                       # one row that never ends
    vid = np.tile(np.arange(B, dtype=np.int32) + 5, rep); sid = np.repeat(np.arange(rep, dtype=np.int32), B)
    return cap, vid, sid, N


def _case(oracle, name, B=None):
    p, d, video = RC.case(oracle, name)
    if B is not None and B != video.shape[0]:
        rng = np.random.default_rng(B)
        video = np.abs(rng.standard_normal((B,) + video.shape[1:]) * 0.5).astype(np.float32)
    return p, d, video


def _gpu_case(gpu, p, d, residual=True):
    dims = gpu.make_dims(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step, residual=residual)
    dp = {k: _dev(v) for k, v in p.items()}
    return dims, dp, gpu.make_params(dp)


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name,rep", [("small-odd", 1), ("small-odd", 3), ("one-tile", 3), ("many-rows", 1), ("chain-range", 1), ("chain-range", 3),
                                      ("one-step", 3)])
def test_teacher_forced_logits_equal_the_restatement(gpu, oracle, name, rep):
    """All steps, a truncated unroll (_steps) and the live rows only (_live), keep 0.9.  chain-range: 16 / 48 rows at H = 992, the
    persistent recurrences."""
    from s2vt_amd import hostglue
    p, d, video = _case(oracle, name)
    cap, vid, sid, N = _rows(name, rep)
    Tc, V = d.n_caption_lstm_step, d.n_words
    drop = oracle.dropout_masks(RC.DROP_SEED, vid, sid, KEEP, d.lstm_dim, d.n_video_lstm_step, Tc)
    ref = RC.residual_teacher_forced(oracle, p, d, np.tile(video, (rep, 1, 1)), cap, drop, KEEP)              # [N, Tc, V]
    plain = RC.residual_teacher_forced(oracle, p, d, np.tile(video, (rep, 1, 1)), cap, drop, KEEP, residual=False)
    assert not np.array_equal(ref, plain)
    ref_tm = ref.transpose(1, 0, 2).reshape(Tc * N, V)
    dims, dp, params = _gpu_case(gpu, p, d)                                      # (dp is held: the struct has raw pointers)
    args = (dims, params, _dev(video), _dev(cap), N, KEEP, RC.DROP_SEED, _dev(vid), _dev(sid))
    logits, ws = gpu.teacher_forced_fwd(*args)
    assert np.array_equal(logits.cpu().numpy(), ref_tm)
    if Tc > 3:
        steps = Tc - 2
        logits, ws = gpu.teacher_forced_fwd(*args, steps=steps)
        assert np.array_equal(logits.cpu().numpy(), ref_tm[:steps * N])
        mask = hostglue.masks_from_ids(cap)
        live = np.flatnonzero(mask.T.reshape(-1) != 0).astype(np.int32)
        assert 0 < len(live) < Tc * N
        assert (d.lstm_dim | d.word_dim) % 4 == 0                                # (the live form moves packed rows as 16-byte pieces: every shape here)
        logits, ws = gpu.teacher_forced_fwd(*args, live=_dev(live))
        assert np.array_equal(logits.cpu().numpy(), ref_tm[live])
    # the _reuse form: LSTM1's trajectory out of the workspace of a sampler pass on the same videos (a residual sampler's workspace: its
    # extra block lies behind the regions re-carved here)
    dv = args[2]
    gpu.sample(dims, params, dv, 2, seed=11)
    sws, srows = gpu.sample.last_state[0], gpu.sample.last_state[1]
    logits, ws = gpu.teacher_forced_fwd(dims, params, dv, *args[3:], sampler_state=(sws, srows))
    assert np.array_equal(logits.cpu().numpy(), ref_tm)


# ------------------------------------------------------------------------------------------------------------------ gradients
def _model(p, d, B, rep, residual=True, precision="fp32"):
    from s2vt_amd import model as M
    mdl = M.Video_Caption_Generator(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, B, 0, d.n_video_lstm_step, d.n_caption_lstm_step,
                                    dropout_rate=KEEP, multisample=rep, residual=residual)
    mdl.store.load(p)
    mdl.grad_precision = "bf16" if precision == "bf16" else "fp32"
    return mdl


def _ref_grads(oracle, p, d, video_rows, cap, vid, sid, dseed, loss_fn, residual=True, detach_o1=False):
    import torch
    from oracle import s2vt_torch as T
    drop = oracle.dropout_masks(dseed, vid, sid, KEEP, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step)
    pt = T.to_torch(p, torch.float64, True)
    logits = RC.torch_teacher_forced(pt, video_rows, cap, drop, KEEP, residual=residual, detach_o1=detach_o1)
    loss = loss_fn(pt, logits)
    loss.backward()
    return float(loss), {k: v.grad.numpy() for k, v in pt.items()}


def _check(mdl, ref_g, tol):
    worst = {}
    for n in mdl.store.names:
        g = mdl.store.g[n].cpu().numpy().astype(np.float64)
        scale = np.abs(ref_g[n]).max() + 1e-12
        worst[n] = np.abs(g - ref_g[n]).max() / scale
    print("max |g - ref| / max |ref|:", {k: f"{v:.2e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= tol}
    assert not bad, (tol, bad)


# (case, B, rep, mode): fp32 = the fp32-MFMA body (N <= 256); split = the split-bf16 products (N = 260 > 256); bf16 = bf16 operands
GRAD_CASES = [("small-odd", 5, 2, "fp32"), ("one-tile", 16, 3, "fp32"), ("one-tile", 16, 3, "bf16"), ("many-rows", 52, 5, "split"),
              ("many-rows", 52, 5, "bf16")]


@pytest.mark.parametrize("name,B,rep,mode", GRAD_CASES)
def test_reinforce_gradients_vs_float64_autograd(gpu, oracle, name, B, rep, mode):
    import s2vt_amd
    from oracle import s2vt_torch as T
    p, d, video = _case(oracle, name, B)
    cap, vid, sid, N = _rows(name, rep, B)
    assert gpu.split_grad_active(N) == (mode == "split") or mode == "bf16"
    mask = s2vt_amd.hostglue.masks_from_ids(cap)
    rng = np.random.default_rng(5)
    r = rng.random(N).astype(np.float32) * 2; b = np.tile(rng.random(B).astype(np.float32) * 2, rep)
    mdl = _model(p, d, B, rep, precision=mode)
    dseed = mdl.dropout_seed + 104729 * mdl.global_step
    rows = np.tile(video, (rep, 1, 1))
    fn = lambda pt, lg: T.pg_loss(lg, cap, mask, r, b)
    ref_loss, ref_g = _ref_grads(oracle, p, d, rows, cap, vid, sid, dseed, fn)
    st = mdl.reinforce_update(video, cap, mask, r, b, lr=0.0, clip_norm=5.0, video_base=5)
    assert abs(float(st.loss) - ref_loss) <= 1e-3 * max(1.0, abs(ref_loss))
    _check(mdl, ref_g, TOL[mode])
    # the ds -> o1 term is there, and the bound sees it: lstm1_W's gradient is neither the plain model's nor that of a backward without
    # the term (float64 autograd with the o1 addend detached), each by far more than the bound
    g = mdl.store.g["lstm1_W"].cpu().numpy().astype(np.float64)
    scale = np.abs(ref_g["lstm1_W"]).max()
    _, plain_g = _ref_grads(oracle, p, d, rows, cap, vid, sid, dseed, fn, residual=False)
    _, cut_g = _ref_grads(oracle, p, d, rows, cap, vid, sid, dseed, fn, detach_o1=True)
    assert np.abs(g - plain_g["lstm1_W"]).max() > 10 * TOL[mode] * scale
    assert np.abs(g - cut_g["lstm1_W"]).max() > 10 * TOL[mode] * scale


@pytest.mark.parametrize("name,B,mode", [("small-odd", 5, "fp32"), ("one-tile", 16, "fp32"), ("one-tile", 16, "bf16")])
def test_xe_gradients_vs_float64_autograd(gpu, oracle, name, B, mode):
    import s2vt_amd
    from oracle import s2vt_torch as T
    from s2vt_amd import model as M
    p, d, video = _case(oracle, name, B)
    cap, _, _, N = _rows(name, 1, B)
    vid = np.arange(N, dtype=np.int32) + 5; sid = np.zeros(N, np.int32)
    mask = s2vt_amd.hostglue.masks_from_ids(cap)
    mdl = _model(p, d, B, 1, precision=mode)
    dseed = mdl.dropout_seed + 104729 * mdl.global_step
    ref_loss, ref_g = _ref_grads(oracle, p, d, video, cap, vid, sid, dseed, lambda pt, lg: T.xe_loss(pt, lg, cap, mask, q1=True))
    st = mdl.xe_update(video, cap, mask, lr=0.0, clip_norm=10.0, q1=True, video_base=5)
    wd = sum(0.5 * float((mdl.store.p[n].double() ** 2).sum()) for n in mdl.store.names if n not in M.UNDECAYED)
    loss = float(st.loss) + mdl.decay_value * wd
    assert abs(loss - ref_loss) <= 1e-3 * max(1.0, abs(ref_loss))
    _check(mdl, ref_g, TOL[mode])


def test_mixed_update_on_the_multitask_class_vs_float64_autograd(gpu, oracle):
    """multitask.Video_Caption_Generator(residual=True).mixed_update: -(1 - lambda) PG / sum(mask) + lambda XE(ground truth)
    (reinforce_multitask_e2e_attribute_s2vt.py:850) as ONE teacher-forced pass of sampled + ground-truth rows, both summed residually."""
    import s2vt_amd
    from oracle import s2vt_torch as T
    from s2vt_amd import multitask
    name, B, lam = "one-tile", 16, 0.5
    p, d, video = _case(oracle, name, B)
    cap, _, _, _ = _rows(name, 1, B)
    gcap = np.roll(cap, 3, axis=0).copy()
    mask, gmask = s2vt_amd.hostglue.masks_from_ids(cap), s2vt_amd.hostglue.masks_from_ids(gcap)
    rng = np.random.default_rng(9)
    r = (rng.random(B) * 2).astype(np.float32); b = (rng.random(B) * 2).astype(np.float32)
    mdl = multitask.Video_Caption_Generator(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, B, 0, d.n_video_lstm_step, d.n_caption_lstm_step,
                                            dropout_rate=KEEP, label_dim=0, residual=True)
    assert mdl.residual and mdl.dims.reserved == 1
    mdl.store.load(p)
    vid = np.arange(B, dtype=np.int32); dseed = mdl.dropout_seed + 104729 * mdl.global_step
    Tv, Tc, H = d.n_video_lstm_step, d.n_caption_lstm_step, d.lstm_dim
    drop1 = oracle.dropout_masks(dseed, vid, np.zeros(B, np.int32), KEEP, H, Tv, Tc)
    drop2 = oracle.dropout_masks(dseed, vid, np.ones(B, np.int32), KEEP, H, Tv, Tc)      # the ground-truth rows are "sample" 1 of the same pass
    import torch
    pt = T.to_torch(p, torch.float64, True)
    lg1 = RC.torch_teacher_forced(pt, video, cap, drop1, KEEP)
    lg2 = RC.torch_teacher_forced(pt, video, gcap, drop2, KEEP)
    ref = (1 - lam) * T.pg_loss(lg1, cap, mask, r, b) + lam * T.xe_loss(pt, lg2, gcap, gmask, q1=True)
    ref.backward()
    mdl.mixed_update(video, cap, mask, r, b, gcap, gmask, lr=0.0, lambda_loss=lam)
    _check(mdl, {k: v.grad.numpy() for k, v in pt.items()}, TOL["fp32"])


def test_e2e_reinforce_step_through_a_cnn_vs_float64_autograd(gpu, oracle):
    """e2e.EndToEnd on a residual model (the stand-in CNN of tests/test_gpu_e2e.py): the sampler, the REINFORCE update and the gradient
    w.r.t. the features (s2vt_bptt_dvideo, which carries ds through LSTM1 as well) into the CNN's parameters."""
    import copy
    import torch
    import s2vt_amd
    from oracle import s2vt_torch as T
    from s2vt_amd import e2e
    from test_gpu_e2e import _tiny_cnn
    p, d, _ = _case(oracle, "small-odd")
    B, K = 4, 2
    rng = np.random.default_rng(8)
    Tv, Tc, H, D = d.n_video_lstm_step, d.n_caption_lstm_step, d.lstm_dim, d.dim_image
    frames = rng.uniform(-1, 1, (B, Tv, 3, 17, 17)).astype(np.float32)
    mdl = _model(p, d, B, K)
    cnn = _tiny_cnn(D, seed=1)
    ref_cnn = copy.deepcopy(cnn).double()
    plain_cnn = copy.deepcopy(ref_cnn)
    tr = e2e.EndToEnd(mdl, cnn, feature_keep=1.0)
    rb = {}

    def reward_fn(samples, greedy):
        rb["r"] = rng.random(samples.shape[0]).astype(np.float32); rb["b"] = rng.random(greedy.shape[0]).astype(np.float32)
        return rb["r"], rb["b"]
    st = tr.reinforce_step(torch.as_tensor(frames), reward_fn, lr=0.0, K=K, sample_seed=11)
    samples = st.samples.cpu().numpy()
    feats64 = ref_cnn(torch.as_tensor(frames).double().reshape(B * Tv, 3, 17, 17)).reshape(B, Tv, D)
    mask = s2vt_amd.hostglue.masks_from_ids(samples)
    vid = np.tile(np.arange(B, dtype=np.int32), K); sid = np.repeat(np.arange(K, dtype=np.int32), B)
    drop = oracle.dropout_masks(mdl.dropout_seed, vid, sid, KEEP, H, Tv, Tc)              # the step ran at global_step 0
    pt = T.to_torch(p, torch.float64, True)
    lg = RC.torch_teacher_forced(pt, feats64.repeat(K, 1, 1), samples, drop, KEEP)
    T.pg_loss(lg, samples, mask, rb["r"], np.tile(rb["b"], K)).backward()
    ref_flat = np.concatenate([q.grad.numpy().ravel() for q in ref_cnn.parameters()])
    got = tr.grad.cpu().numpy()
    assert np.abs(got - ref_flat).max() <= 3e-4 * np.abs(ref_flat).max() + 1e-10          # (the bound tests/test_gpu_e2e.py holds the plain model to)
    assert torch.equal(tr.generate(torch.as_tensor(frames)), st.greedy)
    # ... and it is the residual model's gradient: the plain graph on the same ids gives the CNN another one, by far more than the bound
    pf = plain_cnn(torch.as_tensor(frames).double().reshape(B * Tv, 3, 17, 17)).reshape(B, Tv, D)
    T.pg_loss(RC.torch_teacher_forced(T.to_torch(p, torch.float64, False), pf.repeat(K, 1, 1), samples, drop, KEEP, residual=False), samples, mask,
              rb["r"], np.tile(rb["b"], K)).backward()
    plain_flat = np.concatenate([q.grad.numpy().ravel() for q in plain_cnn.parameters()])
    assert np.abs(got - plain_flat).max() > 10 * 3e-4 * np.abs(ref_flat).max()


# ------------------------------------------------------------------------------------------------------------------ phases, determinism, live rows
def _lowlevel(gpu, oracle, name, B, rep, precision, with_live):
    """One forward + softmax + backward through the ops layer; returns run(phases) -> gradient tensors, and the tolerance's scale."""
    import torch
    from s2vt_amd import hostglue
    p, d, video = _case(oracle, name, B)
    cap, vid, sid, N = _rows(name, rep, B)
    Tc = d.n_caption_lstm_step
    dims, dp, params = _gpu_case(gpu, p, d)
    mask = hostglue.masks_from_ids(cap)
    steps, live, ix = Tc, None, slice(None)
    if with_live:
        steps = int(np.flatnonzero(mask.any(0))[-1]) + 1
        live = _dev(np.flatnonzero(mask[:, :steps].T.reshape(-1) != 0).astype(np.int32))
        assert 0 < live.numel() < steps * N
        ix = live.long()
    rng = np.random.default_rng(2)
    coef_full = (rng.standard_normal((Tc, N)).astype(np.float32) * mask.T).reshape(-1)        # zero at the masked positions, as every objective's
    coef = _dev(coef_full)[:steps * N][ix].contiguous()
    tgt = _dev(cap).t().contiguous().view(-1)[:steps * N][ix].contiguous()

    def run(phases):
        logits, ws = gpu.teacher_forced_fwd(dims, params, _dev(video), _dev(cap), N, KEEP, 99, _dev(vid), _dev(sid), steps=steps, live=live)
        dlogits = logits
        if precision == "fp32" and gpu.split_grad_active(N):
            _, _, in_planes = gpu.softmax_nll_fwd_bwd_split(logits, tgt, coef, 0.0, dims, B, N)
            dlogits = None if in_planes else logits
        else:
            gpu.softmax_nll_fwd_bwd(logits, tgt, coef, 0.0)
        g = {k: torch.zeros_like(v) for k, v in dp.items()}
        for ph in phases:
            gpu.bptt_bwd(dims, params, gpu.make_params(g), _dev(video), N, dlogits, ws, KEEP, 99, _dev(vid), _dev(sid), phase=ph, steps=steps,
                         live=live, precision=precision)
        g["d_video"] = gpu.bptt_dvideo(dims, params, B, N, ws).clone()      # the gradient w.r.t. the frame features: what phase 4 left of LSTM1's side
        torch.cuda.synchronize()
        return g
    return run


FP32_RERUN_TOL = 1e-5


def _same(a, b, what, mode):
    """bf16 and split-bf16 products: fixed order, no atomics -- equal bits, except Wemb (the embedding scatter-add uses fp32 atomics in every
    mode; 1e-6 of its largest entry, as tests/test_gpu_bf16_grads.py has it).  The fp32-MFMA body (N <= 256 rows) reduces every weight
    gradient with fp32 atomics (gemm_tn.h: order-free), the plain model's too, so two passes cannot agree to the bit;
    they agree within 1e-5 of each tensor's largest entry, the bound tests/test_gpu_train.py holds the plain model's phases to.
    "d_video" (s2vt_bptt_dvideo: dZ1 through two fixed-order products) has no atomics on its way in any mode, and everything the
    residual adds lies on that way -- ds joins the dropout reduction in front of LSTM1's backward recurrence -- so it is compared bit for
    bit in every mode."""
    import torch
    for k in a:
        ref = a[k].cpu().numpy()
        if k == "d_video":
            assert float(a[k].abs().max()) > 0 and torch.equal(a[k], b[k]), (what, k)
        elif mode == "fp32":
            assert np.abs(b[k].cpu().numpy() - ref).max() <= FP32_RERUN_TOL * np.abs(ref).max(), (what, k)
        elif k == "Wemb":
            assert np.abs(b[k].cpu().numpy() - ref).max() <= 1e-6 * np.abs(ref).max(), (what, k)
        else:
            assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("name,B,rep,precision", [("one-tile", 16, 3, "fp32"), ("one-tile", 16, 3, "bf16"), ("many-rows", 52, 5, "fp32")])
@pytest.mark.parametrize("with_live", [False, True])
def test_phases_and_a_second_run_give_the_bits_of_the_whole_pass(gpu, oracle, name, B, rep, precision, with_live):
    """Phase 4 on its own reads ds (the gradient w.r.t. the summed output) where phase 1 left it: nothing in between may touch it."""
    mode = "bf16" if precision == "bf16" else ("split" if gpu.split_grad_active(B * rep) else "fp32")
    run = _lowlevel(gpu, oracle, name, B, rep, precision, with_live)
    whole = run([0])
    assert float(whole["lstm1_W"].abs().max()) > 0
    _same(whole, run([0]), "second run", mode)
    _same(whole, run([1, 3, 4]), "phases 1, 3, 4", mode)
    _same(whole, run([1, 2]), "phases 1, 2", mode)


@pytest.mark.parametrize("name,B,rep,precision", [("one-tile", 16, 3, "fp32"), ("one-tile", 16, 3, "bf16"), ("many-rows", 52, 5, "fp32")])
def test_live_rows_agree_with_all_rows(gpu, oracle, name, B, rep, precision):
    mode = "bf16" if precision == "bf16" else ("split" if gpu.split_grad_active(B * rep) else "fp32")
    dense = _lowlevel(gpu, oracle, name, B, rep, precision, False)([0])
    live = _lowlevel(gpu, oracle, name, B, rep, precision, True)([0])
    for k in dense:
        a, b = dense[k].cpu().numpy().astype(np.float64), live[k].cpu().numpy().astype(np.float64)
        assert np.abs(a - b).max() <= TOL[mode] * np.abs(a).max() + 1e-12, k


def test_reuse_sampler_state_gives_the_same_update(gpu, oracle):
    """reinforce_update with the sampler pass's LSTM1 trajectory (s2vt_teacher_forced_fwd_reuse re-carves the residual sampler's
    workspace, whose extra block lies behind the regions it reads) against recomputing it."""
    import torch
    import s2vt_amd
    name, B, rep = "one-tile", 16, 3
    p, d, video = _case(oracle, name, B)
    outs = []
    for reuse in (False, True):
        mdl = _model(p, d, B, rep)
        dv = _dev(video)
        s, _ = mdl.sample(dv, rep, True, seed=11)
        cap = s.cpu().numpy().astype(np.int32)
        mask = s2vt_amd.hostglue.masks_from_ids(cap)
        r = np.linspace(0.1, 1.9, B * rep).astype(np.float32); b = np.tile(np.linspace(0.5, 1.0, B).astype(np.float32), rep)
        mdl.reinforce_update(dv, s, _dev(mask), r, b, lr=0.0, clip_norm=5.0, reuse_sampler_state=reuse)
        torch.cuda.synchronize()
        outs.append({n: mdl.store.g[n].clone() for n in mdl.store.names})
    (rs, _), _ = RC.decodes(oracle, name, 11, rep)
    assert np.array_equal(cap, rs)
    _same(outs[0], outs[1], "reuse_sampler_state", "fp32")          # (48 rows: the fp32-MFMA body; the logits of this form: bit for bit in the forward test)
