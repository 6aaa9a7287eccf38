"""s2vt_attention_fwd_rows / s2vt_attention_bwd_rows -- the attention step and its backward for N = samples * n_video sample-major
rows that share n_video image blocks -- inside guard bands (tests/guardband.py).

Forward: alpha and ctx array_equal s2vt_attention_fwd on P / Vt tiled `samples` times (the same chains).  Backward: dhWa per row and
dP / dVt per video against float64 autograd of the formulas in attn.hip's header (the sum over the video's rows falls out of sharing the
block), each array within 2e-4 of its own max; against s2vt_attention_bwd on the tiled inputs summed over the samples; dP / dVt of two
runs bit-equal (every element has one owner, no atomics); with acc a second call adds to the first."""
import numpy as np
import pytest

from guardband import Guarded

pytestmark = pytest.mark.gpu

SHAPES = [(5, 3, 2, 32), (12, 2, 3, 36), (33, 1, 4, 20)]       # (Tv, n_video, samples, H)


def _inputs(Tv, nv, S, H):
    rng = np.random.default_rng(Tv * 1000 + nv * 100 + S * 10 + H)
    N = nv * S
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(hWa=f(N, H), P=f(Tv, nv, H), Vt=f(Tv, nv, H), w=rng.uniform(-.1, .1, H).astype(np.float32), dctx=f(N, H)), rng


def _tiled(x, S):
    """[Tv, nv, H] -> [Tv, S * nv, H]: block s * nv + j = block j."""
    return np.ascontiguousarray(np.tile(x, (1, S, 1)))


def _fwd_rows(gpu, L, x, Tv, nv, S, H, lead=64):
    N = nv * S
    g = dict(hWa=Guarded.of(x["hWa"], lead=lead, name="hWa"), P=Guarded.of(x["P"].reshape(Tv * nv, H), lead=lead, name="P"),
             Vt=Guarded.of(x["Vt"].reshape(Tv * nv, H), lead=lead, name="Vt"), w=Guarded.of(x["w"], lead=lead, name="w"),
             scores=Guarded(Tv, N, lead=lead, name="scores"), alpha=Guarded(Tv, N, lead=lead, name="alpha"), ctx=Guarded(N, H, lead=lead, name="ctx"))
    import torch
    rv = Guarded(1, N, dtype=torch.int32, lead=lead, name="row_video", fill=0)
    rc = L.s2vt_attention_fwd_rows(g["hWa"].ptr, g["P"].ptr, g["Vt"].ptr, g["w"].ptr, g["scores"].ptr, g["alpha"].ptr, g["ctx"].ptr, rv.ptr,
                                   Tv, nv, S, H, gpu._stream())
    assert rc == 0
    g["row_video"] = rv
    return g


@pytest.mark.parametrize("lead", [64, 65])
@pytest.mark.parametrize("Tv,nv,S,H", SHAPES)
def test_attention_fwd_rows_equals_plain_on_tiled_blocks(gpu, Tv, nv, S, H, lead):
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    x, _ = _inputs(Tv, nv, S, H)
    g = _fwd_rows(gpu, L, x, Tv, nv, S, H, lead)
    t = lambda a: torch.as_tensor(a).cuda()
    sc, al, ctx = gpu.attention_fwd(t(x["hWa"]), t(_tiled(x["P"], S)), t(_tiled(x["Vt"], S)), t(x["w"]))
    assert np.array_equal(g["alpha"].numpy().view(np.uint32), al.cpu().numpy().view(np.uint32))
    assert np.array_equal(g["ctx"].numpy().view(np.uint32), ctx.cpu().numpy().view(np.uint32))
    assert np.array_equal(g["scores"].numpy().view(np.uint32), sc.cpu().numpy().view(np.uint32))
    assert np.array_equal(g["row_video"].numpy().reshape(-1), np.arange(nv * S) % nv)
    for v in g.values():
        v.assert_intact()


def _reference(x, alpha, Tv, nv, S, H):
    """float64 autograd through score -> softmax -> context with the rows READING the shared blocks: the gradient of a block is the sum
    over its rows."""
    import torch
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    th, tP, tV, tw = t(x["hWa"]), t(x["P"]), t(x["Vt"]), t(x["w"])
    Pr, Vr = tP.repeat(1, S, 1), tV.repeat(1, S, 1)                       # row s * nv + j reads block j
    e = (torch.tanh(th + Pr) * tw).sum(-1)
    a = torch.exp(e) / torch.exp(e).sum(0)
    c = (a.unsqueeze(-1) * Vr).sum(0)
    (c * torch.tensor(x["dctx"], dtype=torch.float64)).sum().backward()
    assert np.abs(a.detach().numpy() - alpha).max() < 1e-5
    return {"dhWa": th.grad.numpy(), "dP": tP.grad.numpy().reshape(Tv * nv, H), "dVt": tV.grad.numpy().reshape(Tv * nv, H), "dw": tw.grad.numpy()[None]}


@pytest.mark.parametrize("lead", [64, 65])
@pytest.mark.parametrize("Tv,nv,S,H", SHAPES)
def test_attention_bwd_rows_sums_owner_rule_and_accumulation(gpu, Tv, nv, S, H, lead):
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    N = nv * S
    x, rng = _inputs(Tv, nv, S, H)
    g = _fwd_rows(gpu, L, x, Tv, nv, S, H, lead)
    alpha = g["alpha"].numpy()
    ref = _reference(x, alpha, Tv, nv, S, H)
    gal, gdc = Guarded.of(alpha, lead=lead, name="alpha(in)"), Guarded.of(x["dctx"], lead=lead, name="dctx")
    out = dict(de=Guarded(1, N * Tv, lead=lead, name="de_scratch"), dhWa=Guarded(N, H, lead=lead, name="dhWa"), dP=Guarded(Tv * nv, H, lead=lead, name="dP"),
               dVt=Guarded(Tv * nv, H, lead=lead, name="dVt"), dw=Guarded.of(np.zeros(H, np.float32), lead=lead, name="dw"))

    def run(acc):
        rc = L.s2vt_attention_bwd_rows(g["hWa"].ptr, g["P"].ptr, g["Vt"].ptr, g["w"].ptr, gal.ptr, gdc.ptr, out["de"].ptr, out["dhWa"].ptr,
                                       out["dP"].ptr, out["dVt"].ptr, out["dw"].ptr, Tv, nv, S, H, acc, gpu._stream())
        assert rc == 0
        return {k: out[k].numpy().copy() for k in ("dhWa", "dP", "dVt", "dw")}
    first = run(0)
    line = []
    for k, r in ref.items():
        err, bound = float(np.abs(first[k].astype(np.float64) - r).max()), 2e-4 * float(np.abs(r).max())
        line.append(f"{k} {err:.2e}/{bound:.2e}")
        assert err <= bound, (k, err, bound)
    print(f"\nattention rows Tv={Tv} n_video={nv} S={S} H={H} lead={lead}: max err / bound: " + ", ".join(line))
    # the plain kernel on the tiled inputs, summed over the samples (its own order-free fp32 sums: the same bound against it)
    t = lambda a: torch.as_tensor(a).cuda()
    dw2 = torch.zeros(H, device="cuda")
    dh2, dP2, dV2 = gpu.attention_bwd(t(x["hWa"]), t(_tiled(x["P"], S)), t(_tiled(x["Vt"], S)), t(x["w"]), t(alpha), t(x["dctx"]), dw2)
    fold = lambda a: a.cpu().numpy().astype(np.float64).reshape(Tv, S, nv, H).sum(1).reshape(Tv * nv, H)
    for k, other in (("dhWa", dh2.cpu().numpy().astype(np.float64)), ("dP", fold(dP2)), ("dVt", fold(dV2)), ("dw", dw2.cpu().numpy().astype(np.float64)[None])):
        assert np.abs(first[k] - other).max() <= 2e-4 * np.abs(other).max(), k
    # the ownership rule: a second run (dw starts again from zero) gives equal BITS in dP / dVt / dhWa
    out["dw"].fill(np.zeros(H, np.float32))
    second = run(0)
    for k in ("dP", "dVt", "dhWa"):
        assert np.array_equal(first[k].view(np.uint32), second[k].view(np.uint32)), k
    # acc: a further call adds to what is there
    third = run(1)
    for k in ("dP", "dVt"):
        assert np.array_equal(third[k], second[k] + second[k]), k
    assert np.array_equal(third["dhWa"].view(np.uint32), second["dhWa"].view(np.uint32))          # dhWa is per call, never accumulated
    assert np.abs(third["dw"].astype(np.float64) - 2 * ref["dw"]).max() <= 2e-4 * 2 * np.abs(ref["dw"]).max()
    for v in list(g.values()) + [gal, gdc] + list(out.values()):
        v.assert_intact()
