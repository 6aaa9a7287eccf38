"""The fused form of the split-bf16 backward: dlogits planes straight from the softmax (bit for bit the split of the
fp32 dlogits, nll / lp / logits untouched), gemm_bf16x3_tn against float64, against itself (two runs) and against gemm_bf16x3_nt
on explicitly transposed planes (same K steps: equal bits), its bias row, and whole updates -- the rl shape through the model, a
live-row case and a vocabulary the fused softmax does not take -- with S2VT_SPLIT_FUSED=0 / 1 in child processes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_bf16_grads import _dev
from test_gpu_split_grads import _split_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- softmax planes
@pytest.mark.parametrize("R,V", [(64, 12000), (6400, 12000), (128, 9972), (37, 4096)])
@pytest.mark.parametrize("row_smoothing", [False, True])
def test_softmax_planes_are_the_split_of_fp32_dlogits(gpu, R, V, row_smoothing):
    import torch
    B, N, Tc = 64, 320, 20                                     # 320 unrolled rows: the split mode; R <= Tc * N
    assert gpu.split_grad_active(N)
    dims = gpu.make_dims(128, V, 32, 64, 5, Tc)
    g = torch.Generator(device="cuda").manual_seed(R + V)
    logits = torch.randn(R, V, device="cuda", generator=g) * 3.0
    target = torch.randint(0, V, (R,), device="cuda", generator=g, dtype=torch.int32)
    coef = torch.randn(R, device="cuda", generator=g)
    coef[::7] = 0.0                                            # masked positions
    smoothing = (torch.rand(R, device="cuda", generator=g) * 0.1).contiguous() if row_smoothing else 0.05
    want = logits.clone()
    nll0, lp0 = gpu.softmax_nll_fwd_bwd(want, target, coef, smoothing)          # want <- fp32 dlogits
    kept = logits.clone()
    nll, lp, in_planes = gpu.softmax_nll_fwd_bwd_split(logits, target, coef, smoothing, dims, B, N)
    assert in_planes
    hi, lo = gpu.split_grad_dlogits_planes(dims, B, N, R, logits.device)
    Kv = (V + 63) // 64 * 64
    assert hi.shape == (R, Kv) and lo.shape == (R, Kv)
    wh, wl = _split_ref(want)
    assert torch.equal(hi[:, :V].view(torch.int16), wh.view(torch.int16)) and torch.equal(lo[:, :V].view(torch.int16), wl.view(torch.int16))
    assert not hi[:, V:].view(torch.int16).any() and not lo[:, V:].view(torch.int16).any()
    assert torch.equal(nll.view(torch.int32), nll0.view(torch.int32)) and torch.equal(lp.view(torch.int32), lp0.view(torch.int32))
    assert torch.equal(logits, kept)


def test_softmax_split_falls_back_where_the_register_kernel_does_not_fit(gpu):
    import torch
    B, N, Tc, R, V = 64, 320, 20, 33, 262                       # V % 4 != 0
    dims = gpu.make_dims(128, V, 32, 64, 5, Tc)
    g = torch.Generator(device="cuda").manual_seed(5)
    logits = torch.randn(R, V, device="cuda", generator=g)
    target = torch.randint(0, V, (R,), device="cuda", generator=g, dtype=torch.int32)
    coef = torch.randn(R, device="cuda", generator=g)
    want = logits.clone()
    nll0, lp0 = gpu.softmax_nll_fwd_bwd(want, target, coef, 0.05)
    nll, lp, in_planes = gpu.softmax_nll_fwd_bwd_split(logits, target, coef, 0.05, dims, B, N)
    assert not in_planes
    assert torch.equal(logits, want) and torch.equal(nll, nll0) and torch.equal(lp, lp0)


# ---------------------------------------------------------------------------------------------------- the K-major product
def _tn_planes(x, ld, junk):
    """x [K, W] fp32 -> split planes [K, ld] inside buffers of K + 64 rows whose other rows, and columns >= W, hold `junk`."""
    import torch
    K, W = x.shape
    out = []
    for p in _split_ref(x):
        buf = torch.full((K + 64, ld), junk, device="cuda", dtype=torch.bfloat16)
        buf[:K, :W] = p
        out.append(buf[:K])
    return out


# the shapes of test_gemm_bf16x3_vs_float64, + ragged M and N with K that is no multiple of 64 (of 32; odd)
@pytest.mark.parametrize("M,N,K", [(1, 1, 64), (17, 130, 100), (130, 17, 4000), (1000, 1000, 1600), (17, 1000, 12000),
                                   (1000, 500, 6400), (300, 500, 4000), (129, 257, 320), (500, 4000, 4160), (320, 500, 4000),
                                   (1000, 4000, 500), (1000, 4000, 1601), (500, 1000, 37)])
@pytest.mark.parametrize("split_k", [True, False])
def test_gemm_bf16x3_tn_vs_float64_and_nt(gpu, M, N, K, split_k):
    import torch
    g = torch.Generator(device="cuda").manual_seed(M * 17 + N + K)
    a = torch.randn(K, M, device="cuda", generator=g)
    b = torch.randn(K, N, device="cuda", generator=g)
    lda, ldb = (M + 7) // 8 * 8 + 8, (N + 7) // 8 * 8
    # rows >= K and columns >= M / N hold NaN: they must never reach a stored output
    Ah, Al = _tn_planes(a, lda, float("nan"))
    Bh, Bl = _tn_planes(b, ldb, float("nan"))
    ah, al = _split_ref(a)
    bh, bl = _split_ref(b)
    ref = ah.double().t() @ bh.double() + ah.double().t() @ bl.double() + al.double().t() @ bh.double()
    scale = float(ref.abs().max()) + 1e-30
    tol = 1e-6 * max(1.0, (K / 1000) ** 0.5)
    ldc = N + 3
    C0 = torch.randn(M, ldc, device="cuda", generator=g)
    out = C0.clone()
    gpu.gemm_bf16x3_tn(Ah, Al, Bh, Bl, M, N, out=out[:, :N], split_k=split_k)
    err = float((out[:, :N].double() - ref).abs().max())
    print(f"\ntn {M}x{N}x{K} split_k={split_k}: max err {err:.3e}, bound {tol * scale:.3e}")
    assert err <= tol * scale
    assert torch.equal(out[:, N:], C0[:, N:])
    first = out.clone()
    gpu.gemm_bf16x3_tn(Ah, Al, Bh, Bl, M, N, out=out[:, :N], split_k=split_k)
    assert torch.equal(out, first)                                      # deterministic
    acc = C0.clone()
    gpu.gemm_bf16x3_tn(Ah, Al, Bh, Bl, M, N, out=acc[:, :N], accumulate=True, split_k=split_k)
    want = ref + C0[:, :N].double()
    assert float((acc[:, :N].double() - want).abs().max()) <= tol * (scale + float(C0.abs().max()))
    # the same K steps in the same order: the bits of the NT form on explicitly transposed planes
    Kp = (K + 63) // 64 * 64
    tr = [torch.zeros(p.shape[1], Kp, device="cuda", dtype=torch.bfloat16) for p in (ah, al, bh, bl)]
    for t, p in zip(tr, (ah, al, bh, bl)):
        t[:, :K] = p.t()
    nt = gpu.gemm_bf16x3_nt(*tr, split_k=split_k)
    assert torch.equal(nt, first[:, :N])


@pytest.mark.parametrize("M,N,K", [(1000, 4000, 1600), (64, 260, 1601), (1000, 12000, 640), (127, 130, 100)])
@pytest.mark.parametrize("split_k", [True, False])
def test_gemm_bf16x3_tn_bias_row(gpu, M, N, K, split_k):
    """Column M of A = ones: row M of the product, the column sums of B's hi + lo, is added to bias; C is what it is without."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    a = torch.randn(K, M, device="cuda", generator=g)
    b = torch.randn(K, N, device="cuda", generator=g)
    lda, ldb = (M + 1 + 63) // 64 * 64, (N + 63) // 64 * 64
    Ah, Al = _tn_planes(a, lda, 0.0)
    Bh, Bl = _tn_planes(b, ldb, 0.0)
    Ah[:, M] = 1.0
    bh, bl = _split_ref(b)
    plain = gpu.gemm_bf16x3_tn(Ah, Al, Bh, Bl, M, N, split_k=split_k)
    bias0 = torch.randn(N, device="cuda", generator=g)
    for accumulate in (False, True):
        bias = bias0.clone()
        C0 = torch.randn(M, N, device="cuda", generator=g)
        out = C0.clone()
        gpu.gemm_bf16x3_tn(Ah, Al, Bh, Bl, M, N, out=out, accumulate=accumulate, split_k=split_k, bias=bias)
        ref = bias0.double() + (bh.double() + bl.double()).sum(0)
        # one more row of the same product: the product test's bound, on the scale of the largest column sum
        scale = float((bh.double() + bl.double()).sum(0).abs().max()) + float(bias0.abs().max())
        assert float((bias.double() - ref).abs().max()) <= 1e-6 * scale * max(1.0, (K / 1000) ** 0.5)
        if not accumulate:
            assert torch.equal(out, plain)
        second = bias0.clone()
        gpu.gemm_bf16x3_tn(Ah, Al, Bh, Bl, M, N, out=C0.clone(), accumulate=accumulate, split_k=split_k, bias=second)
        assert torch.equal(second, bias)


# ---------------------------------------------------------------------------------------------------- whole updates
def _lowlevel_update(V, with_live, phases=(0,)):
    """A backward at 320 unrolled rows on small dims through the ops layer, as model._forward_loss / backward() drive it."""
    import torch
    from s2vt_amd import hostglue, ops
    from oracle import s2vt_oracle as orc
    B, rep = 64, 5
    d = orc.Dims(dim_image=128, n_words=V, word_dim=32, lstm_dim=64, n_video_lstm_step=5, n_caption_lstm_step=8, label_dim=0)
    p = orc.init_params(d, seed=3)
    rng = np.random.default_rng(4)
    for k in ("lstm1_b", "lstm2_b", "encode_image_b", "embed_word_b"):
        p[k] = rng.uniform(-.1, .1, p[k].shape).astype(np.float32)
    N = B * rep
    video = np.abs(rng.standard_normal((B, d.n_video_lstm_step, d.dim_image)) * 0.5).astype(np.float32)
    cap = rng.integers(2, d.n_words, (N, d.n_caption_lstm_step)).astype(np.int32)
    ln = rng.integers(2, d.n_caption_lstm_step - 1, N)
    for n in range(N):
        cap[n, ln[n]:] = 0
    vid = np.tile(np.arange(B, dtype=np.int32) + 5, rep); sid = np.repeat(np.arange(rep, dtype=np.int32), B)
    mask = hostglue.masks_from_ids(cap)
    steps = int(np.flatnonzero(mask.any(0))[-1]) + 1 if with_live else d.n_caption_lstm_step
    live = _dev(np.flatnonzero(mask[:, :steps].T.reshape(-1) != 0).astype(np.int32)) if with_live else None
    dims = ops.make_dims(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step)
    dp_ = {k: _dev(v) for k, v in p.items()}
    params = ops.make_params(dp_)
    coef = _dev((mask * rng.standard_normal(N)[:, None]).T.astype(np.float32).reshape(-1)[:steps * N])
    tgt = _dev(cap).t().contiguous().view(-1)[:steps * N]
    logits, ws = ops.teacher_forced_fwd(dims, params, _dev(video), _dev(cap), N, 0.9, 99, _dev(vid), _dev(sid), steps=steps, live=live)
    ix = slice(None) if live is None else live.long()
    tgt, coef = tgt[ix].contiguous(), coef[ix].contiguous()
    dlogits = logits
    if ops.split_grad_active(N):
        nll, _, in_planes = ops.softmax_nll_fwd_bwd_split(logits, tgt, coef, 0.0, dims, B, N)
        dlogits = None if in_planes else logits
    else:
        nll, _ = ops.softmax_nll_fwd_bwd(logits, tgt, coef, 0.0)
    g = {k: torch.zeros_like(v) for k, v in dp_.items()}
    for ph in phases:
        ops.bptt_bwd(dims, params, ops.make_params(g), _dev(video), N, dlogits, ws, 0.9, 99, _dev(vid), _dev(sid), phase=ph, steps=steps, live=live)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in g.items()}
    out["loss"] = nll.cpu().numpy()
    out["planes"] = np.int32(dlogits is None)
    return out


@pytest.mark.parametrize("with_live", [False, True])
def test_fused_phases_give_the_bits_of_the_whole_pass(gpu, with_live):
    """The data-parallel caller's phases 1 / 3 / 4 (and 1 / 2), every one with dlogits = None after one split softmax: the split
    products' gradients bit for bit those of the whole pass (the rest goes through fp32 atomics: order-free)."""
    whole = _lowlevel_update(260, with_live)
    assert int(whole["planes"]) == 1
    for phases in ((1, 3, 4), (1, 2)):
        parts = _lowlevel_update(260, with_live, phases)
        assert whole["loss"].tobytes() == parts["loss"].tobytes()
        for k in whole:
            if k in ("embed_word_W", "embed_word_b", "lstm2_W", "lstm2_b"):
                assert np.array_equal(parts[k], whole[k]), (phases, k)
            elif k not in ("loss", "planes"):
                assert np.abs(parts[k] - whole[k]).max() <= 1e-6 * (np.abs(whole[k]).max() + 1e-30), (phases, k)


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from test_gpu_split_grads import _rl_update
from test_gpu_split_fused import _lowlevel_update
mdl, video, cap, mask, r, b, run = _rl_update()
st = run()
g = {n: mdl.store.g[n].cpu().numpy() for n in mdl.store.names}
np.savez(sys.argv[2] + "_rl.npz", loss=np.float32(float(st.loss)), planes=np.int32(type(mdl._ctx[2]).__name__ == "_PlanesDlogits"), **g)
np.savez(sys.argv[2] + "_live.npz", **_lowlevel_update(260, True))
np.savez(sys.argv[2] + "_fallback.npz", **_lowlevel_update(262, False))
"""


@pytest.fixture(scope="module")
def fused_and_unfused(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("fused")
    for knob in ("0", "1"):
        subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(d / f"k{knob}")], check=True, env=dict(os.environ, S2VT_SPLIT_FUSED=knob), timeout=600)
    return {(knob, case): np.load(str(d / f"k{knob}_{case}.npz")) for knob in ("0", "1") for case in ("rl", "live", "fallback")}


# weight gradients whose products keep the unfused path's K steps (encode rows a multiple of 64 in all three cases): equal bits
_BIT_EQUAL = ("embed_word_W", "lstm2_W")


@pytest.mark.parametrize("case,planes", [("rl", 1), ("live", 1), ("fallback", 0)])
def test_fused_update_matches_unfused(fused_and_unfused, case, planes):
    """S2VT_SPLIT_FUSED=1 against 0 (the transposed casts and NT products): the loss bits; every gradient within 5e-5 of its tensor's
    maximum (test_split_knob_off_is_fp32_body's bound); the K-major weight gradients bit for bit.  The bias gradients embed_word_b and
    lstm2_b differ in rounding (sums of hi + lo inside the product against fp32 column sums); what follows LSTM2 is order-free."""
    u, f = fused_and_unfused[("0", case)], fused_and_unfused[("1", case)]
    assert int(u["planes"]) == 0 and int(f["planes"]) == planes
    assert u["loss"].tobytes() == f["loss"].tobytes()
    for n in u.files:
        if n in ("loss", "planes"):
            continue
        a, b = u[n].astype(np.float64), f[n].astype(np.float64)
        err = np.abs(a - b).max() / (np.abs(a).max() + 1e-30)
        print(f"\n{case} {n}: max|fused - unfused| / max|unfused| = {err:.2e}")
        assert err <= 5e-5, n
        if n in _BIT_EQUAL:
            assert np.array_equal(u[n], f[n]), n
