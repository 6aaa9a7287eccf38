"""s2vt_attention_fwd / s2vt_attention_bwd at the frame counts where the kernels change course -- 1, 8 / 9 (the regulariser's first
eight frames), 32 / 33 (the LDS chunk), 64 (kAttnMaxTv) -- with every pointer 16-byte aligned (float4 path) and with every pointer
offset by one float (the scalar path at H % 4 == 0), inside guard bands (tests/guardband.py).  Forward: bit-exact against the C
oracle, so the two paths are bit-equal to each other; backward: float64 autograd, into a dw that does not start from zero."""
import numpy as np
import pytest

from guardband import Guarded

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 4), (8, 2, 16), (9, 2, 20), (32, 3, 64), (33, 3, 64), (64, 2, 36), (64, 1, 1000)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _alpha_from_scores(oracle, scores):
    """The kernel's own softmax restated on its scores: exp by the contract's sequence, the sum in ascending t, one fp32 division --
    pins `scores` to the bit-exact alpha."""
    x = oracle.det_exp(scores)                                       # [Tv, B]
    den = np.zeros(scores.shape[1], np.float32)
    for t in range(scores.shape[0]):
        den = den + x[t]
    den = np.where(den == 0, den + np.float32(1.0), den)
    assert np.isfinite(den).all()
    return x / den[None]


def _forward(gpu, L, hWa, P, Vt, w, lead):
    Tv, B, H = P.shape
    g = dict(hWa=Guarded.of(hWa, lead=lead, name="hWa"), P=Guarded.of(P.reshape(Tv * B, H), lead=lead, name="P"),
             Vt=Guarded.of(Vt.reshape(Tv * B, H), lead=lead, name="Vt"), w=Guarded.of(w, lead=lead, name="w"),
             scores=Guarded(Tv, B, lead=lead, name="scores"), alpha=Guarded(Tv, B, lead=lead, name="alpha"), ctx=Guarded(B, H, lead=lead, name="ctx"))
    assert all(x.aligned16 == (lead % 4 == 0) for x in g.values())
    rc = L.s2vt_attention_fwd(g["hWa"].ptr, g["P"].ptr, g["Vt"].ptr, g["w"].ptr, g["scores"].ptr, g["alpha"].ptr, g["ctx"].ptr, Tv, B, H,
                              gpu._stream())
    assert rc == 0
    return g


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("Tv,B,H", CASES)
def test_attention_step_paths_bit_exact_and_backward(gpu, oracle, Tv, B, H, misaligned):
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    lead = 65 if misaligned else 64
    rng = np.random.default_rng(Tv * 1000 + B * 7 + H)
    hWa = rng.standard_normal((B, H)).astype(np.float32); P = rng.standard_normal((Tv, B, H)).astype(np.float32)
    Vt = rng.standard_normal((Tv, B, H)).astype(np.float32); w = rng.uniform(-.1, .1, H).astype(np.float32)
    alpha, ctx = oracle.attention_step(hWa, P, Vt, w)
    g = _forward(gpu, L, hWa, P, Vt, w, lead)
    assert np.array_equal(_bits(g["alpha"].numpy()), _bits(alpha)) and np.array_equal(_bits(g["ctx"].numpy()), _bits(ctx))
    # backward vs float64 autograd, the bound of test_gpu_attn_attr.py
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    th, tP, tV, tw = t(hWa), t(P), t(Vt), t(w)
    e = (torch.tanh(th + tP) * tw).sum(-1)
    assert np.array_equal(_bits(_alpha_from_scores(oracle, g["scores"].numpy())), _bits(alpha))
    scores_err = float(np.abs(g["scores"].numpy() - e.detach().numpy()).max())
    a = torch.exp(e) / torch.exp(e).sum(0)
    c = (a.unsqueeze(-1) * tV).sum(0)
    dctx = rng.standard_normal((B, H)).astype(np.float32)
    (c * torch.tensor(dctx, dtype=torch.float64)).sum().backward()
    ref = {"dhWa": th.grad.numpy(), "dP": tP.grad.numpy().reshape(Tv * B, H), "dVt": tV.grad.numpy().reshape(Tv * B, H), "dw": tw.grad.numpy()[None]}
    # dw accumulates: it starts from non-zero values of the gradient's own size (of 2^-10 where the gradient is zero, Tv = 1), so
    # the fp32 rounding of the B additions into it, 2^-24 of |dw0 + increment| each, stays orders below the 2e-4 bound
    dw0 = (rng.uniform(0.5, 1.0, H) * rng.choice([-1.0, 1.0], H) * max(float(np.abs(ref["dw"]).max()), 2.0 ** -10)).astype(np.float32)
    gal, gdc = Guarded.of(alpha, lead=lead, name="alpha(in)"), Guarded.of(dctx, lead=lead, name="dctx")
    out = dict(de=Guarded(1, Tv * B, lead=lead, name="de_scratch"), dhWa=Guarded(B, H, lead=lead, name="dhWa"),
               dP=Guarded(Tv * B, H, lead=lead, name="dP"), dVt=Guarded(Tv * B, H, lead=lead, name="dVt"), dw=Guarded.of(dw0, lead=lead, name="dw"))
    rc = L.s2vt_attention_bwd(g["hWa"].ptr, g["P"].ptr, g["Vt"].ptr, g["w"].ptr, gal.ptr, gdc.ptr, out["de"].ptr, out["dhWa"].ptr, out["dP"].ptr,
                              out["dVt"].ptr, out["dw"].ptr, Tv, B, H, gpu._stream())
    assert rc == 0
    got = {k: out[k].numpy().astype(np.float64) for k in ("dhWa", "dP", "dVt", "dw")}
    got["dw"] = got["dw"] - dw0.astype(np.float64)[None]             # the increment
    line = []
    for k, r in ref.items():
        err, bound = float(np.abs(got[k] - r).max()), 2e-4 * float(np.abs(r).max()) + 1e-7
        line.append(f"{k} {err:.2e}/{bound:.2e}")
        assert err <= bound, (k, err, bound)
    print(f"\nattention Tv={Tv} B={B} H={H} misaligned={misaligned}: scores err {scores_err:.2e}; max err / bound: " + ", ".join(line))
    for x in list(g.values()) + [gal, gdc] + list(out.values()):
        x.assert_intact()


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("Tv,B,H", CASES)
def test_attention_forward_saturated_stays_bit_exact(gpu, oracle, Tv, B, H, misaligned):
    """P x 20 clamps every tanh, w uniform in [-1, 1] takes the scores to tens: exp without a max shift spans its range."""
    import s2vt_amd
    L = s2vt_amd.lib()
    rng = np.random.default_rng(Tv * 1000 + B * 7 + H + 1)
    hWa = rng.standard_normal((B, H)).astype(np.float32); P = (rng.standard_normal((Tv, B, H)) * 20).astype(np.float32)
    Vt = rng.standard_normal((Tv, B, H)).astype(np.float32); w = rng.uniform(-1, 1, H).astype(np.float32)
    alpha, ctx = oracle.attention_step(hWa, P, Vt, w)
    g = _forward(gpu, L, hWa, P, Vt, w, 65 if misaligned else 64)
    assert np.array_equal(_bits(g["alpha"].numpy()), _bits(alpha)) and np.array_equal(_bits(g["ctx"].numpy()), _bits(ctx))
    assert np.isfinite(g["scores"].numpy()).all()
    assert np.array_equal(_bits(_alpha_from_scores(oracle, g["scores"].numpy())), _bits(alpha))
    if H >= 36:
        assert np.abs(g["scores"].numpy()).max() > 5.0
    for x in g.values():
        x.assert_intact()


@pytest.mark.parametrize("Tv", [0, 65])
def test_attention_fwd_refuses_frame_counts_outside_1_to_64(gpu, Tv):
    """Checked on the host before any launch (attn.hip, s2vt_attention_fwd's first line): an error, and nothing is written."""
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    B, H = 2, 8
    z = lambda r, c, n: Guarded.of(np.zeros((r, c), np.float32), name=n)
    hWa, P, Vt, w = z(B, H, "hWa"), z(65 * B, H, "P"), z(65 * B, H, "Vt"), z(1, H, "w")
    scores, alpha, ctx = z(65, B, "scores"), z(65, B, "alpha"), z(B, H, "ctx")
    assert L.s2vt_attention_fwd(hWa.ptr, P.ptr, Vt.ptr, w.ptr, scores.ptr, alpha.ptr, ctx.ptr, Tv, B, H, gpu._stream()) == -1
    torch.cuda.synchronize()
    for x in (scores, alpha, ctx):
        assert not x.bits().any()
    for x in (hWa, P, Vt, w, scores, alpha, ctx):
        x.assert_intact()


@pytest.mark.parametrize("Tv,hinge", [(8, 0.95), (9, 0.95), (9, 0.5)])
def test_first_eight_frames_sum_at_eight_and_nine_frames(gpu, oracle, Tv, hinge):
    """The regulariser's sum(alpha[0:8]) -- written by the forward kernel only inside the whole model -- where it is all frames
    (Tv = 8: the softmax sums to 1, the hinge stays closed below m = 0.95) and all but the last (Tv = 9): the loss scalar against the
    oracle's restatement on its own, bit-identical alphas, as test_gpu_attention_model.py::test_attention_regulariser_value_vs_oracle."""
    from test_gpu_attention_model import _setup
    d, p, m, video, cap, rng = _setup(oracle, 40, 97, 36, Tv, 5, 6, 9, dict(m=hinge))
    mask = (rng.random((6, 5)) < 0.7).astype(np.float32); mask[:, 0] = 1
    ref_l, ref_a, _ = oracle.attention_forward(p, d, video, cap)
    reg = oracle.attention_regulariser(ref_a, mask, m.beta, m.m).sum()
    assert (reg == 0) if Tv == 8 else (reg > 0 or hinge == 0.5)
    ref = oracle.attention_xe_loss(ref_l, ref_a, cap, mask, m.beta, m.m)
    got = float(m.loss(video, cap, mask, keep=1.0))
    print(f"\nregulariser Tv={Tv} m={hinge}: loss {got:.7f}, oracle {ref:.7f}, regulariser part {float(reg):.5f}")
    assert abs(got - ref) <= 1e-5 * abs(ref)
