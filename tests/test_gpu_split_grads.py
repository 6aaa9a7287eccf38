"""The default fp32 mode's split-bf16 gradient products (s2vt_bptt_bwd_split): the split casts bit for bit against
torch, gemm_bf16x3_nt against float64 on the same bf16 values (ragged shapes, both accumulate settings, split-K), and the whole
REINFORCE backward at the rl shape against float64 autograd of oracle/s2vt_torch.py, with the loss bit-identical to the fp32-MFMA
body (S2VT_SPLIT_GRADS=0) and two runs giving the same bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_bf16_grads import D, E, H, TC, TV, V, _dev, _model, _ref_grads, _same_bf16, _special, _bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# max |g - ref| / max |ref| per gradient tensor with the split products
GRAD_TOL = 5e-5


def _split_ref(x):
    import torch
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


@pytest.mark.parametrize("R,C,ld,gather", [(1, 1, 1, False), (17, 37, 37, False), (130, 1000, 1000, False), (64, 500, 503, True),
                                          (33, 12000, 12000, True)])
def test_cast_rows_split_bit_exact(gpu, R, C, ld, gather):
    import torch
    rng = np.random.default_rng(R * 11 + C)
    rows = R + 9 if gather else R
    src = _special(rng, (rows, ld))
    idx = torch.as_tensor(rng.integers(0, rows, R).astype(np.int32)) if gather else None
    hi, lo = gpu.cast_bf16_split(src.cuda()[:, :C] if ld != C else src.cuda(), rowidx=None if idx is None else idx.cuda())
    sel = (src[idx.long()] if gather else src)[:, :C]
    wh, wl = _split_ref(sel)
    assert _same_bf16(hi[:, :C], wh) and _same_bf16(lo[:, :C], wl)
    assert not _bits(hi[:, C:]).any() and not _bits(lo[:, C:]).any()


@pytest.mark.parametrize("R,C,ld,gather", [(1, 1, 1, False), (17, 37, 39, False), (130, 1000, 1000, True), (777, 500, 500, True),
                                          (300, 4000, 4000, False)])
def test_cast_transpose_split_bit_exact_with_colsum(gpu, R, C, ld, gather):
    import torch
    rng = np.random.default_rng(R + 5 * C)
    rows = R + 5 if gather else R
    src = _special(rng, (rows, ld))
    finite = src.clone()
    finite[~torch.isfinite(finite) | (finite.abs() > 1e30)] = 0.5
    idx = torch.as_tensor(rng.integers(0, rows, R).astype(np.int32)) if gather else None
    for x, with_sum in ((src, False), (finite, True)):
        cs0 = torch.as_tensor(rng.standard_normal(C).astype(np.float32))
        cs = cs0.cuda() if with_sum else None
        Rp = (R + 63) // 64 * 64 + (64 if R % 2 else 0)
        (th, tl), (rh, rl) = gpu.cast_bf16_split(x.cuda()[:, :C], rowidx=None if idx is None else idx.cuda(), transpose=True, pad_rows=Rp,
                                                 colsum=cs, row_copy=True)
        sel = (x[idx.long()] if gather else x)[:, :C]
        wh, wl = _split_ref(sel)
        assert _same_bf16(th[:, :R], wh.t()) and _same_bf16(tl[:, :R], wl.t())
        assert not _bits(th[:, R:]).any() and not _bits(tl[:, R:]).any()
        assert _same_bf16(rh[:, :C], wh) and _same_bf16(rl[:, :C], wl)
        if with_sum:
            ref = cs0.double() + sel.double().sum(0)
            assert float((cs.cpu().double() - ref).abs().max()) <= 1e-6 * float(sel.double().abs().sum(0).max() + cs0.abs().max())


@pytest.mark.parametrize("M,N,K", [(1, 1, 64), (17, 130, 100), (130, 17, 4000), (1000, 1000, 1600), (17, 1000, 12000),
                                   (1000, 500, 6400), (300, 500, 4000), (129, 257, 320), (500, 4000, 4160), (320, 500, 4000)])
@pytest.mark.parametrize("split_k", [True, False])
def test_gemm_bf16x3_vs_float64(gpu, M, N, K, split_k):
    import torch
    g = torch.Generator(device="cuda").manual_seed(M * 17 + N + K)
    Kp = (K + 63) // 64 * 64
    a = torch.zeros(M, Kp, device="cuda")
    b = torch.zeros(N, Kp, device="cuda")
    a[:, :K] = torch.randn(M, K, device="cuda", generator=g)
    b[:, :K] = torch.randn(N, K, device="cuda", generator=g)
    Ah, Al = _split_ref(a)
    Bh, Bl = _split_ref(b)
    ref = Ah.double() @ Bh.double().t() + Ah.double() @ Bl.double().t() + Al.double() @ Bh.double().t()
    scale = float(ref.abs().max()) + 1e-30
    ldc = N + 3
    C0 = torch.randn(M, ldc, device="cuda", generator=g)
    out = C0.clone()
    gpu.gemm_bf16x3_nt(Ah, Al, Bh, Bl, out=out[:, :N], split_k=split_k)
    assert float((out[:, :N].double() - ref).abs().max()) <= 1e-6 * scale * max(1.0, (K / 1000) ** 0.5)
    assert torch.equal(out[:, N:], C0[:, N:])
    first = out.clone()
    gpu.gemm_bf16x3_nt(Ah, Al, Bh, Bl, out=out[:, :N], split_k=split_k)
    assert torch.equal(out, first)                                      # deterministic
    acc = C0.clone()
    gpu.gemm_bf16x3_nt(Ah, Al, Bh, Bl, out=acc[:, :N], accumulate=True, split_k=split_k)
    want = ref + C0[:, :N].double()
    assert float((acc[:, :N].double() - want).abs().max()) <= 1e-6 * (scale + float(C0.abs().max())) * max(1.0, (K / 1000) ** 0.5)
    # the split product is far closer to the fp32 product than bf16 alone
    full = a.double() @ b.double().t()
    assert float((out[:, :N].double() - full).abs().max()) <= 2e-5 * (float(full.abs().max()) + 1e-30)


def _rl_update(B=64, K=5, seed=31):
    from s2vt_amd import hostglue
    mdl, video = _model(B, K, seed)
    dv = _dev(video)
    s, _ = mdl.sample(dv, K, True, seed=2024)
    cap = s.cpu().numpy().astype(np.int32)
    mask = hostglue.masks_from_ids(cap)
    rng = np.random.default_rng(3)
    r = (rng.random(K * B) * 2).astype(np.float32)
    b = np.tile((rng.random(B) * 2).astype(np.float32), K)
    run = lambda: mdl.reinforce_update(dv, s, _dev(mask), r, b, lr=0.0, clip_norm=5.0, reuse_sampler_state=False)
    return mdl, video, cap, mask, r, b, run


def test_split_backward_rl_shape(gpu, oracle):
    """BASELINE configs[2] (320 rows: the split products): every gradient within GRAD_TOL of float64 autograd, the split products'
    gradients bit-identical over two runs."""
    B, K = 64, 5
    mdl, video, cap, mask, r, b, run = _rl_update(B, K)
    vid = np.tile(np.arange(B, dtype=np.int32), K); sid = np.repeat(np.arange(K, dtype=np.int32), B)
    _, ref_g = _ref_grads(mdl, np.tile(video, (K, 1, 1)), cap, vid, sid, 0.9, lambda T, pt, lg: T.pg_loss(lg, cap, mask, r, b), oracle)
    grads = []
    for _ in range(2):
        step0 = mdl.global_step
        st = run()
        mdl.global_step = step0
        grads.append({n: mdl.store.g[n].cpu().numpy().astype(np.float64) for n in mdl.store.names})
    errs = {n: float(np.abs(grads[0][n] - rg).max() / (np.abs(rg).max() + 1e-30)) for n, rg in ref_g.items()}
    print("\nsplit gradient error (rl), max|g - ref| / max|ref|:", {k: f"{v:.2e}" for k, v in errs.items()}, "loss", float(st.loss))
    for n, e in errs.items():
        assert e <= GRAD_TOL, (n, e)
    # the split products (vocab projection, LSTM2) give the same bits twice; Wemb's scatter-add and LSTM1's fp32-MFMA weight
    # gradients (split-K with fp32 atomics) are order-free, as in s2vt_bptt_bwd_live
    for n in grads[0]:
        if n not in ("embed_word_W", "embed_word_b", "lstm2_W", "lstm2_b"):
            assert np.abs(grads[0][n] - grads[1][n]).max() <= 1e-6 * (np.abs(grads[0][n]).max() + 1e-30)
        else:
            assert np.array_equal(grads[0][n], grads[1][n]), n


_CHILD = r"""
import sys, json
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from test_gpu_split_grads import _rl_update
mdl, video, cap, mask, r, b, run = _rl_update()
st = run()
g = {n: mdl.store.g[n].cpu().numpy() for n in mdl.store.names}
np.savez(sys.argv[2], loss=np.float32(float(st.loss)), **g)
"""


def test_split_knob_off_is_fp32_body(gpu, tmp_path):
    """S2VT_SPLIT_GRADS=0 (child process): the fp32-MFMA body; the loss bits are the same either way, the gradients close."""
    outs = {}
    for knob in ("0", "1"):
        env = dict(os.environ, S2VT_SPLIT_GRADS=knob)
        f = str(tmp_path / f"g{knob}.npz")
        subprocess.run([sys.executable, "-c", _CHILD, ROOT, f], check=True, env=env, timeout=600)
        outs[knob] = np.load(f)
    assert outs["0"]["loss"].tobytes() == outs["1"]["loss"].tobytes()
    for n in outs["0"].files:
        if n == "loss":
            continue
        a, b = outs["0"][n].astype(np.float64), outs["1"][n].astype(np.float64)
        assert np.abs(a - b).max() <= 5e-5 * (np.abs(a).max() + 1e-30), n
