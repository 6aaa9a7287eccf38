"""The opt-in bf16 mode of the backward's gradient contractions (s2vt_bptt_bwd_bf16): the casts bit for bit against
torch, gemm_bf16_nt against float64 on the same bf16 values, the whole backward against float64 autograd of oracle/s2vt_torch.py
with the product's dropout masks at the rl / xe / multitask shapes (loss and NLL bit-identical to the fp32 mode), its phases and live
rows, and a short training run."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TC, TV, D, E, H, V = 20, 5, 1536, 500, 1000, 12000
# max |g - ref| / max |ref| per gradient tensor in bf16 mode: measured at most 4.4e-3 over the three shapes, about 2x it
GRAD_TOL = 1e-2


def _dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _special(rng, shape):
    import torch
    x = (rng.standard_normal(shape) * 3).astype(np.float32)
    flat = x.reshape(-1)
    sp = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 3.4e38, -3.4e38, 1.00390625, 1.01171875, -1.00390625],
                  np.float32)
    n = min(sp.size, flat.size)
    flat[:n] = sp[:n]
    flat[-n:] = sp[:n]
    return torch.as_tensor(x)


def _bits(t):
    import torch
    return t.cpu().view(torch.int16).numpy()


def _same_bf16(got, want):
    """Bit for bit, except that a NaN only has to stay a NaN (the kernel writes the quiet NaN 0x7fc0; torch's CPU cast writes
    its own pattern)."""
    import torch
    g, w = got.cpu(), want.cpu()
    nan = torch.isnan(w)
    return bool(torch.equal(torch.isnan(g), nan)) and np.array_equal(_bits(g)[~nan.numpy()], _bits(w)[~nan.numpy()])


@pytest.mark.parametrize("R,C,ld,gather", [(1, 1, 1, False), (17, 37, 37, False), (130, 1000, 1000, False), (64, 500, 503, True),
                                          (33, 12000, 12000, True), (200, 64, 64, False)])
def test_cast_rows_bit_exact(gpu, R, C, ld, gather):
    import torch
    rng = np.random.default_rng(R * 7 + C)
    rows = R + 9 if gather else R
    src = _special(rng, (rows, ld))
    idx = torch.as_tensor(rng.integers(0, rows, R).astype(np.int32)) if gather else None
    out = gpu.cast_bf16(src.cuda()[:, :C] if ld != C else src.cuda(), rowidx=None if idx is None else idx.cuda())
    sel = (src[idx.long()] if gather else src)[:, :C]
    Kp = (C + 63) // 64 * 64
    assert out.shape == (R, Kp)
    want = sel.to(torch.bfloat16)
    assert _same_bf16(out[:, :C], want)
    assert not _bits(out[:, C:]).any()


@pytest.mark.parametrize("R,C,ld,gather", [(1, 1, 1, False), (17, 37, 39, False), (130, 1000, 1000, True), (777, 500, 500, True),
                                          (6400, 64, 64, False), (300, 4000, 4000, False)])
def test_cast_transpose_bit_exact_with_colsum(gpu, R, C, ld, gather):
    import torch
    rng = np.random.default_rng(R + 3 * C)
    rows = R + 5 if gather else R
    src = _special(rng, (rows, ld))
    finite = src.clone()
    finite[~torch.isfinite(finite) | (finite.abs() > 1e30)] = 0.5     # (column sums: no overflow)
    idx = torch.as_tensor(rng.integers(0, rows, R).astype(np.int32)) if gather else None
    for x, with_sum in ((src, False), (finite, True)):
        dx = x.cuda()
        view = dx[:, :C]
        cs0 = torch.as_tensor(rng.standard_normal(C).astype(np.float32))
        cs = cs0.cuda() if with_sum else None
        Rp = (R + 63) // 64 * 64 + (64 if R % 2 else 0)                 # a pad of more than the round-up too
        tr, rows_bf = gpu.cast_bf16(view, rowidx=None if idx is None else idx.cuda(), transpose=True, pad_rows=Rp, colsum=cs, row_copy=True)
        sel = (x[idx.long()] if gather else x)[:, :C]
        want = sel.to(torch.bfloat16)
        assert tr.shape == (C, Rp)
        assert _same_bf16(tr[:, :R], want.t())
        assert not _bits(tr[:, R:]).any()
        assert _same_bf16(rows_bf[:, :C], want)
        assert not _bits(rows_bf[:, C:]).any()
        if with_sum:
            ref = cs0.double() + sel.double().sum(0)
            got = cs.cpu().double()
            assert float((got - ref).abs().max()) <= 1e-6 * float(sel.double().abs().sum(0).max() + cs0.abs().max()), (R, C)


@pytest.mark.parametrize("M,N,K", [(1, 1, 64), (17, 130, 100), (130, 17, 4000), (1000, 1000, 1600), (17, 1000, 12000), (1000, 130, 12000),
                                   (130, 1000, 6400), (1, 1000, 12000)])
@pytest.mark.parametrize("mfma", [16, 32])
def test_gemm_bf16_nt_vs_float64(gpu, M, N, K, mfma):
    import torch
    g = torch.Generator(device="cuda").manual_seed(M * 31 + N + K)
    Kp = (K + 63) // 64 * 64
    A = torch.zeros(M, Kp, device="cuda", dtype=torch.bfloat16)
    B = torch.zeros(N, Kp, device="cuda", dtype=torch.bfloat16)
    A[:, :K] = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
    B[:, :K] = torch.randn(N, K, device="cuda", generator=g).to(torch.bfloat16)
    ref = A.double() @ B.double().t()
    scale = float(ref.abs().max()) + 1e-30
    ldc = N + 5
    C0 = torch.randn(M, ldc, device="cuda", generator=g)
    out = C0.clone()
    gpu.gemm_bf16_nt(A, B, out=out[:, :N], mfma=mfma)
    assert float((out[:, :N].double() - ref).abs().max()) <= 1e-4 * scale
    assert torch.equal(out[:, N:], C0[:, N:])                           # the ldc gap is not touched
    first = out.clone()
    gpu.gemm_bf16_nt(A, B, out=out[:, :N], mfma=mfma)
    assert torch.equal(out, first)                                      # deterministic: two launches, the same bits
    acc = C0.clone()
    gpu.gemm_bf16_nt(A, B, out=acc[:, :N], accumulate=True, mfma=mfma)
    assert float((acc[:, :N].double() - (ref + C0[:, :N].double())).abs().max()) <= 1e-4 * (scale + float(C0.abs().max()))
    assert torch.equal(acc[:, N:], C0[:, N:])


# ---------------------------------------------------------------------------------------------------- the whole backward
def _model(B, K, seed, label_dim=0):
    import torch
    from s2vt_amd import model as M
    mdl = M.Video_Caption_Generator(D, V, E, H, B, 0, TV, TC, seed=seed, dropout_rate=0.9, multisample=K)
    rng = np.random.default_rng(seed)
    for n in ("lstm1_b", "lstm2_b", "encode_image_b", "embed_word_b"):         # non-zero biases: every term of the graph is live
        mdl.store.p[n].copy_(torch.as_tensor(rng.uniform(-.1, .1, mdl.store.shapes[n]).astype(np.float32)))
    video = np.abs(rng.standard_normal((B, TV, D)) * 0.5).astype(np.float32)
    return mdl, video


def _ref_grads(mdl, video_rows, cap, vid, sid, keep, loss_fn, oracle):
    """float64 autograd of the restated graph (oracle/s2vt_torch.py) with the product's dropout masks."""
    import torch
    from oracle import s2vt_torch as T
    p = {n: mdl.store.p[n].cpu().numpy() for n in mdl.store.names}
    dseed = mdl.dropout_seed + 104729 * mdl.global_step
    drop = oracle.dropout_masks(dseed, vid, sid, keep, H, TV, TC)
    pt = T.to_torch(p, torch.float64, True)
    logits = T.teacher_forced(pt, torch.as_tensor(video_rows).double(), cap, drop, keep)
    loss = loss_fn(T, pt, logits)
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in pt.items()}


def _run_both(mdl, update):
    """The same update (lr = 0) in fp32 and in bf16 mode: (fp32 stats, bf16 stats, bf16 gradients)."""
    out = {}
    for prec in ("fp32", "bf16"):
        mdl.grad_precision = prec
        step0 = mdl.global_step
        st = update()
        mdl.global_step = step0
        out[prec] = (st, {n: mdl.store.g[n].cpu().numpy().astype(np.float64) for n in mdl.store.names})
    mdl.grad_precision = "fp32"
    return out


def _check(name, out, ref_g):
    st32, _ = out["fp32"]
    st16, g16 = out["bf16"]
    assert float(st16.loss) == float(st32.loss), name                  # the forward is untouched: the same loss bits
    errs = {}
    for n, rg in ref_g.items():
        scale = np.abs(rg).max() + 1e-30
        errs[n] = float(np.abs(g16[n] - rg).max() / scale)
    print(f"\nbf16 gradient error ({name}), max|g - ref| / max|ref|:", {k: f"{v:.2e}" for k, v in errs.items()})
    for n, e in errs.items():
        assert e <= GRAD_TOL, (name, n, e)


def test_bf16_backward_rl_shape(gpu, oracle):
    """BASELINE configs[2]: REINFORCE update at B = 64, K = 5 (320 rows), |V| = 12000."""
    from s2vt_amd import hostglue
    B, K = 64, 5
    mdl, video = _model(B, K, 31)
    dv = _dev(video)
    s, _ = mdl.sample(dv, K, True, seed=2024)
    cap = s.cpu().numpy().astype(np.int32)
    mask = hostglue.masks_from_ids(cap)
    rng = np.random.default_rng(3)
    r = (rng.random(K * B) * 2).astype(np.float32)
    b = np.tile((rng.random(B) * 2).astype(np.float32), K)
    vid = np.tile(np.arange(B, dtype=np.int32), K); sid = np.repeat(np.arange(K, dtype=np.int32), B)
    _, ref_g = _ref_grads(mdl, np.tile(video, (K, 1, 1)), cap, vid, sid, 0.9, lambda T, pt, lg: T.pg_loss(lg, cap, mask, r, b), oracle)
    out = _run_both(mdl, lambda: mdl.reinforce_update(dv, s, _dev(mask), r, b, lr=0.0, clip_norm=5.0, reuse_sampler_state=False))
    _check("rl", out, ref_g)


def test_bf16_backward_xe_shape(gpu, oracle):
    """BASELINE configs[1]: XE update at B = 64 (Q1, label smoothing, weight decay; lr = 0)."""
    from s2vt_amd import hostglue, model as M
    B = 64
    mdl, video = _model(B, 1, 37)
    rng = np.random.default_rng(5)
    ln = 1 + np.minimum(rng.poisson(6, B), TC - 2)
    cap = rng.integers(2, V, (B, TC)).astype(np.int32)
    for i in range(B):
        cap[i, ln[i]:] = 0
    mask = hostglue.masks_from_ids(cap)
    vid = np.arange(B, dtype=np.int32); sid = np.zeros(B, np.int32)
    _, ref_g = _ref_grads(mdl, video, cap, vid, sid, 0.9, lambda T, pt, lg: T.xe_loss(pt, lg, cap, mask, q1=True), oracle)
    out = _run_both(mdl, lambda: mdl.xe_update(_dev(video), cap, mask, lr=0.0, clip_norm=10.0, q1=True))
    _check("xe", out, ref_g)


def test_bf16_backward_multitask_shape(gpu, oracle):
    """BASELINE configs[3] per-GPU shape: B = 32, K = 1 -- 32 rows, the <= 256-row branch of the backward."""
    from s2vt_amd import hostglue
    B, K = 32, 1
    mdl, video = _model(B, K, 41)
    dv = _dev(video)
    s, _ = mdl.sample(dv, K, True, seed=77)
    cap = s.cpu().numpy().astype(np.int32)
    mask = hostglue.masks_from_ids(cap)
    rng = np.random.default_rng(9)
    r = (rng.random(K * B) * 2).astype(np.float32)
    b = (rng.random(B) * 2).astype(np.float32)
    vid = np.arange(B, dtype=np.int32); sid = np.zeros(B, np.int32)
    _, ref_g = _ref_grads(mdl, video, cap, vid, sid, 0.9, lambda T, pt, lg: T.pg_loss(lg, cap, mask, r, b), oracle)
    out = _run_both(mdl, lambda: mdl.reinforce_update(dv, s, _dev(mask), r, b, lr=0.0, clip_norm=5.0, reuse_sampler_state=False))
    _check("multitask", out, ref_g)


# ---------------------------------------------------------------------------------------------------- phases, live rows
def _small(oracle, B=4, rep=3, seed=3):
    d = oracle.Dims(dim_image=128, n_words=260, word_dim=32, lstm_dim=64, n_video_lstm_step=5, n_caption_lstm_step=8, label_dim=0)
    p = oracle.init_params(d, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for k in ("lstm1_b", "lstm2_b", "encode_image_b", "embed_word_b"):
        p[k] = rng.uniform(-.1, .1, p[k].shape).astype(np.float32)
    N = B * rep
    video = np.abs(rng.standard_normal((B, d.n_video_lstm_step, d.dim_image)) * 0.5).astype(np.float32)
    cap = rng.integers(2, d.n_words, (N, d.n_caption_lstm_step)).astype(np.int32)
    ln = rng.integers(2, d.n_caption_lstm_step - 1, N)
    for n in range(N):
        cap[n, ln[n]:] = 0
    vid = np.tile(np.arange(B, dtype=np.int32) + 5, rep); sid = np.repeat(np.arange(rep, dtype=np.int32), B)
    return d, p, video, cap, vid, sid, N


@pytest.mark.parametrize("with_live", [False, True])
def test_bf16_phases_give_the_bits_of_the_whole_pass(gpu, oracle, with_live):
    """with_live: the live-row list of the captions' masks -- the transposed products over the packed live rows, and a lone phase 4
    that reads the packed dZ2 rows phase 3 left in the workspace."""
    import torch
    from s2vt_amd import hostglue
    d, p, video, cap, vid, sid, N = _small(oracle)
    dims = gpu.make_dims(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step)
    dp_ = {k: _dev(v) for k, v in p.items()}
    params = gpu.make_params(dp_)
    steps, live, ix = d.n_caption_lstm_step, None, slice(None)
    if with_live:
        mask = hostglue.masks_from_ids(cap)
        steps = int(np.flatnonzero(mask.any(0))[-1]) + 1
        live = _dev(np.flatnonzero(mask[:, :steps].T.reshape(-1) != 0).astype(np.int32))      # (as model.live_rows lists them)
        assert 0 < live.numel() < 0.9 * steps * N
        ix = live.long()
    coef = _dev(np.random.default_rng(2).standard_normal(N * d.n_caption_lstm_step).astype(np.float32))[:steps * N][ix].contiguous()
    tgt = _dev(cap).t().contiguous().view(-1)[:steps * N][ix].contiguous()

    def run(phases):
        logits, ws = gpu.teacher_forced_fwd(dims, params, _dev(video), _dev(cap), N, 0.9, 99, _dev(vid), _dev(sid), steps=steps, live=live)
        gpu.softmax_nll_fwd_bwd(logits, tgt, coef, 0.0)
        g = {k: torch.zeros_like(v) for k, v in dp_.items()}
        for ph in phases:
            gpu.bptt_bwd(dims, params, gpu.make_params(g), _dev(video), N, logits, ws, 0.9, 99, _dev(vid), _dev(sid), phase=ph, steps=steps, live=live,
                         precision="bf16")
        torch.cuda.synchronize()
        return g
    whole = run([0])
    for phases in ([1, 3, 4], [1, 2]):
        parts = run(phases)
        for k in whole:
            if k == "Wemb":                 # (the embedding scatter-add is the fp32 path's, with atomics in either mode: order-free)
                ref = whole[k].cpu().numpy()
                assert np.abs(parts[k].cpu().numpy() - ref).max() <= 1e-6 * np.abs(ref).max(), k
            else:
                assert torch.equal(parts[k], whole[k]), (phases, k)


def test_bf16_live_rows_match_all_rows(gpu, oracle):
    import torch
    from s2vt_amd import hostglue
    d, p, video, cap, vid, sid, N = _small(oracle, seed=5)
    mask = hostglue.masks_from_ids(cap)
    steps = int(np.flatnonzero(mask.any(0))[-1]) + 1
    live = np.flatnonzero(mask[:, :steps].T.reshape(-1) != 0).astype(np.int32)
    assert 0 < live.size < 0.9 * steps * N
    dims = gpu.make_dims(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step)
    dp_ = {k: _dev(v) for k, v in p.items()}
    params = gpu.make_params(dp_)
    coef = (mask * np.random.default_rng(7).standard_normal(N)[:, None]).T.astype(np.float32).reshape(-1)[:steps * N]
    tgt = _dev(cap).t().contiguous().view(-1)[:steps * N]

    def run(lv):
        logits, ws = gpu.teacher_forced_fwd(dims, params, _dev(video), _dev(cap), N, 0.9, 99, _dev(vid), _dev(sid), steps=steps, live=lv)
        ix = slice(None) if lv is None else lv.long()
        gpu.softmax_nll_fwd_bwd(logits, tgt[ix].contiguous(), _dev(coef)[ix].contiguous(), 0.0)
        g = {k: torch.zeros_like(v) for k, v in dp_.items()}
        gpu.bptt_bwd(dims, params, gpu.make_params(g), _dev(video), N, logits, ws, 0.9, 99, _dev(vid), _dev(sid), steps=steps, live=lv,
                     precision="bf16")
        return g
    full = run(None)
    part = run(_dev(live))
    for k in full:
        ref = full[k].cpu().numpy()
        assert np.abs(part[k].cpu().numpy() - ref).max() <= 1e-4 * (np.abs(ref).max() + 1e-12), k


# ---------------------------------------------------------------------------------------------------- training
# |loss_bf16 - loss_fp32| / loss_fp32 over the run: measured at most 1.23e-3, about 2x it
LOSS_MARGIN = 2.5e-3


def test_bf16_xe_training_tracks_fp32(gpu):
    import torch
    from s2vt_amd import hostglue, model as M
    Bs, Dd, Vv, Ee, Hh, Tv, Tc = 16, 256, 1000, 64, 128, 5, 10
    rng = np.random.default_rng(11)
    video = np.abs(rng.standard_normal((Bs, Tv, Dd)) * 0.5).astype(np.float32)
    cap = rng.integers(2, Vv, (Bs, Tc)).astype(np.int32)
    ln = rng.integers(3, Tc, Bs)
    for i in range(Bs):
        cap[i, ln[i]:] = 0
    mask = hostglue.masks_from_ids(cap)
    losses = {}
    for prec in ("fp32", "bf16"):
        mdl = M.Video_Caption_Generator(Dd, Vv, Ee, Hh, Bs, 0, Tv, Tc, seed=5, dropout_rate=0.9)
        mdl.grad_precision = prec
        dv = _dev(video)
        losses[prec] = [float(mdl.xe_update(dv, cap, mask, lr=2e-3, clip_norm=10.0, q1=True).loss) for _ in range(36)]
    l32, l16 = np.array(losses["fp32"]), np.array(losses["bf16"])
    print("\nxe loss fp32 / bf16 (first, last):", l32[0], l32[-1], l16[0], l16[-1], " max rel gap:", float(np.max(np.abs(l16 - l32) / l32)))
    assert l16[0] == l32[0]                                             # the same forward before any update
    assert l16[-1] < 0.7 * l16[0]
    assert np.all(np.abs(l16 - l32) <= LOSS_MARGIN * l32)
