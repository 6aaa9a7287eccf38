"""The backward recurrence above 256 rows on split-bf16 operands (csrc/chain_bwd.hip, lstm_bwd_chain4_split_kernel: dz @ Whh^T as
Ahi Bhi + Ahi Blo + Alo Bhi on v_mfma_f32_16x16x32_bf16, hi = bf16(x), lo = bf16(x - hi)):
(1) against a float64 restatement of BasicLSTMCell's backward, bounded by a CPU emulation of the same arithmetic on the same data,
(2) its dispatch -- where the stand-alone entry refuses, and the two knobs that restore the fp32 recurrence inside s2vt_bptt_bwd_split,
(3) the dense form against the live-row form in the default mode."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_chain import _case, _dev, gpu_mask

pytestmark = pytest.mark.gpu

SPLIT_SHAPES = [  # M, E, H, T, first step with an upstream gradient
    (260, 16, 136, 4, 1),        # three unit groups, the last one partial, k tail zero, 5 row tiles per part
    (257, 8, 264, 3, 0),         # ragged last row tile, 5 row tiles per part
    (321, 8, 264, 4, 2),         # just past 320 rows: 6 row tiles per part, ragged last tile
    (384, 8, 1000, 3, 0),        # 6 row tiles per part, all full
    (300, 8, 1024, 3, 1),        # H = 1024: every k-step live
    (320, 500, 1000, 25, 5),     # the bench shape with its full unroll: the error compounds over the steps
]


def _split(x):
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def _float64_and_emulation(gpu, W, E, gates, C, dext, t0, keep, vid, sid):
    """Per step: dz of a float64 restatement (tf.gradients through tf_s2vt.py:113-153), and of an fp32 CPU emulation of the kernel's
    arithmetic -- both operands of dz @ Whh^T split with round-to-nearest-even, three products summed in fp32, the pointwise part in
    fp32 -- on the same gates, cell states, upstream gradient and masks."""
    import torch
    T, M, H4 = gates.shape
    H = H4 // 4
    g32 = gates.cpu(); C32 = C.cpu()
    g64 = g32.double(); C64 = C32.double()
    Wt32 = torch.as_tensor(W[E:]).t().contiguous()              # [4H, H]
    Wt64 = Wt32.double()
    bhi, blo = _split(Wt32)
    d32 = torch.as_tensor(dext)
    keep32 = torch.tensor(keep, dtype=torch.float32)
    ref, emu = [None] * T, [None] * T
    dc64 = torch.zeros(M, H, dtype=torch.float64); rec64 = torch.zeros(M, H, dtype=torch.float64)
    dc32 = torch.zeros(M, H); rec32 = torch.zeros(M, H)
    for t in range(T - 1, -1, -1):
        dh64, dh32 = rec64, rec32
        if t >= t0:
            d = d32[t - t0]
            if keep < 1:
                mask = torch.as_tensor(gpu_mask(gpu, 99, vid, sid, 512 + t, keep, H))
                dh64 = dh64 + d.double() / keep32.double() * mask
                dh32 = dh32 + (d / keep32) * mask.float()
            else:
                dh64 = dh64 + d.double(); dh32 = dh32 + d
        for (g, c_all, dh, dc, out, prec) in ((g64, C64, dh64, dc64, ref, 64), (g32, C32, dh32, dc32, emu, 32)):
            si, tj, sf, so = (g[t][:, q * H:(q + 1) * H] for q in range(4))
            tc = torch.tanh(c_all[t + 1])
            dcur = dh * so * (1 - tc * tc) + dc
            out[t] = torch.cat([dcur * tj * si * (1 - si), dcur * si * (1 - tj * tj), dcur * c_all[t] * sf * (1 - sf), dh * tc * so * (1 - so)], 1)
            if prec == 64:
                dc64 = dcur * sf
            else:
                dc32 = dcur * sf
        rec64 = ref[t] @ Wt64
        ahi, alo = _split(emu[t])
        rec32 = ahi @ bhi + ahi @ blo + alo @ bhi
    return torch.stack(ref), torch.stack(emu)


def _worst(x, ref):
    """worst per-step error over the step's largest entry"""
    scale = ref.abs().amax(dim=(1, 2)).clamp_min(1e-30)
    return float(((x.double() - ref).abs().amax(dim=(1, 2)) / scale).max())


@pytest.mark.parametrize("M,E,H,T,t0", SPLIT_SHAPES)
@pytest.mark.parametrize("keep", [1.0, 0.9])
def test_split_backward_recurrence_vs_float64(gpu, M, E, H, T, t0, keep):
    """dZ of the split recurrence against float64: its worst per-step error (over the step's largest entry) is at most 2 x that of the CPU
    emulation of its arithmetic on the same data -- the margin covers the fp32 accumulation order, which differs between the MFMA chain and
    the CPU's products (by itself worth 1.6e-6 at the bench shape, where the emulation is at 1.9e-5).  At the 25-step shape also at least
    0.1 x the emulation's: a run that took the fp32 kernel (1.6e-6 there) is not the split form.  Twice back to back, no timeout.
    Measured on MI355X, GPU error / emulation error at keep 1.0 | 0.9:
      (260,16,136,4,1) 1.02 | 1.01   (257,8,264,3,0) 1.01 | 0.97   (321,8,264,4,2) 1.02 | 1.04
      (384,8,1000,3,0) 1.11 | 1.16   (300,8,1024,3,1) 0.96 | 1.02   (320,500,1000,25,5) 1.04 | 1.06 (1.83e-5 and 1.70e-5 of the maximum)"""
    import torch
    W, b, h0, c0, cinit, vid, sid = _case(M, E, H, T, T, seed=M + H + 1)
    Wd = _dev(W)
    C, Hh, gates, _ = gpu.lstm_recurrence_fwd(Wd, E, _dev(b), _dev(h0), _dev(c0), T=T, cinit=_dev(cinit), cinit_steps=T, want_gates=True)
    rng = np.random.default_rng(M * 7 + H)
    dext = (rng.standard_normal((T - t0, M, H)) * 0.1).astype(np.float32)
    args = dict(dext=_dev(dext), dext_t0=t0, keep=keep, seed=99, video_id=_dev(vid), sample_id=_dev(sid), drop_code0=512)
    ref, emu = _float64_and_emulation(gpu, W, E, gates, C, dext, t0, keep, vid, sid)
    e_emu = _worst(emu, ref)
    for rep in range(2):
        got = gpu.lstm_recurrence_bwd(Wd, E, gates, C, persistent=1, precision="split", **args)
        assert gpu.chain_timeouts() == 0
        e_gpu = _worst(got.cpu(), ref)
        print(f"split recurrence M={M} H={H} T={T} keep={keep} rep={rep}: gpu {e_gpu:.3e} emulation {e_emu:.3e} ratio {e_gpu / e_emu:.3f}")
        assert torch.isfinite(got).all()
        assert e_gpu <= 2 * e_emu, (rep, e_gpu, e_emu)
        if T == 25:
            assert e_gpu >= 0.1 * e_emu, (rep, e_gpu, e_emu)


@pytest.mark.parametrize("M,E,H,T", [(64, 8, 64, 3), (256, 8, 1000, 3)])
def test_split_entry_refuses_shapes_it_does_not_serve(gpu, M, E, H, T):
    """Only the register-weights form (above 256 rows) has split kernels: the stand-alone entry says so instead of running fp32."""
    from s2vt_amd._lib import S2VTLibraryError
    W, b, h0, c0, cinit, vid, sid = _case(M, E, H, T, T, seed=1)
    Wd = _dev(W)
    C, Hh, gates, _ = gpu.lstm_recurrence_fwd(Wd, E, _dev(b), _dev(h0), _dev(c0), T=T, cinit=_dev(cinit), cinit_steps=T, want_gates=True)
    gpu.lstm_recurrence_bwd(Wd, E, gates, C, persistent=1)                                     # (the fp32 entry serves it)
    with pytest.raises(S2VTLibraryError, match=r"code -1\b"):
        gpu.lstm_recurrence_bwd(Wd, E, gates, C, persistent=1, precision="split")
    assert gpu.chain_timeouts() == 0


# ---- a teacher-forced pass at 320 rows whose LSTM2 recurrences take the register-weights forms (the setup of
# test_gpu_live_rows.py::test_live_rows_stop_inside_the_recurrences at B = 64, rep = 5, keep 0.9)
BIG = dict(dim_image=64, n_words=300, word_dim=32, lstm_dim=256, n_video_lstm_step=3, n_caption_lstm_step=9)


def _pass_320(ops, oracle_mod, live, phase=0):
    import torch
    from s2vt_amd import hostglue
    B, rep, keep = 64, 5, 0.9
    d = oracle_mod.Dims(label_dim=0, **BIG)
    p = oracle_mod.init_params(d, seed=11)
    rng = np.random.default_rng(12)
    for k in ("lstm1_b", "lstm2_b", "encode_image_b", "embed_word_b"):
        p[k] = rng.uniform(-.1, .1, p[k].shape).astype(np.float32)
    N, Tc = B * rep, d.n_caption_lstm_step
    video = np.abs(rng.standard_normal((B, d.n_video_lstm_step, d.dim_image)) * 0.5).astype(np.float32)
    cap = rng.integers(2, d.n_words, (N, Tc)).astype(np.int32)
    ln = np.minimum(rng.poisson(2.5, N), Tc - 2)
    ln[7] = Tc - 2
    for n in range(N):
        cap[n, ln[n]:] = 0
    vid = np.tile(np.arange(B, dtype=np.int32) + 5, rep); sid = np.repeat(np.arange(rep, dtype=np.int32), B)
    mask = hostglue.masks_from_ids(cap)
    steps = int(np.flatnonzero(mask.any(0))[-1]) + 1
    tm = mask[:, :steps].T.reshape(-1)
    lv = _dev(np.flatnonzero(tm != 0).astype(np.int32)) if live else None
    gd = ops.make_dims(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, d.n_video_lstm_step, Tc)
    dp_ = {k: _dev(v) for k, v in p.items()}
    params = ops.make_params(dp_)
    coef = (mask * rng.standard_normal(N)[:, None]).T.astype(np.float32).reshape(-1)[:steps * N]
    tgt = _dev(cap).t().contiguous().view(-1)[:steps * N]
    ops.prof_filter(-1, -1); ops.prof_enable(True)
    logits, ws = ops.teacher_forced_fwd(gd, params, _dev(video), _dev(cap), N, keep, 99, _dev(vid), _dev(sid), steps=steps, live=lv)
    ix = slice(None) if lv is None else lv.long()
    ops.softmax_nll_fwd_bwd(logits, tgt[ix].contiguous(), _dev(coef)[ix].contiguous(), 0.0)
    g = {k: torch.zeros_like(v) for k, v in dp_.items()}
    for ph in ((1, 3) if phase == 3 else (phase,)):              # (phase 3 reads dO2, which the vocabulary phase leaves)
        ops.bptt_bwd(gd, params, ops.make_params(g), _dev(video), N, logits, ws, keep, 99, _dev(vid), _dev(sid), steps=steps, live=lv, phase=ph)
    torch.cuda.synchronize()
    ops.prof_enable(False)
    names = sorted(r["name"] for r in ops.prof_collect() if r["kernel_class"] in (5, 6))
    assert ops.chain_timeouts() == 0
    if phase == 3:                                               # LSTM2's dZ history of the unrolled steps, as the recurrence left it
        g["dZ2"] = ops.train_workspace_dz2(gd, B, N, ws)[:d.n_video_lstm_step + steps].clone()
    return g, names


CHILD_KNOB = r"""
import os, sys
sys.path.insert(0, os.environ["S2VT_ROOT"]); sys.path.insert(0, os.path.join(os.environ["S2VT_ROOT"], "tests"))
import numpy as np, torch
import s2vt_amd
from s2vt_amd import ops
from oracle import s2vt_oracle
from test_gpu_bchain_split import _pass_320
g, names = _pass_320(ops, s2vt_oracle, live=False, phase=3)
assert any(n.startswith("bchain4") for n in names), names
np.savez(sys.argv[1], lstm2_W=g["lstm2_W"].cpu().numpy(), dZ2=g["dZ2"].cpu().numpy())
print("child ok")
"""


def test_knobs_restore_the_fp32_recurrence(gpu, tmp_path):
    """The vocabulary phase and LSTM2's phase of s2vt_bptt_bwd_split at N = 320 in child processes (the knobs are read once).  Compared
    bit for bit is LSTM2's dZ history in the workspace: it comes out of the recurrence alone, with no atomics behind it, whereas
    lstm2_W's gradient under S2VT_SPLIT_GRADS=0 comes out of fp32 products that sum their slabs with atomics (two runs of one
    configuration differ in its last bits).
    S2VT_BCHAIN_SPLIT=0 keeps the fp32 recurrence beside the split products: dZ2 differs from the default's, and lstm2_W's gradient
    differs from the default's by at most 1e-5 of its largest entry.
    S2VT_SPLIT_GRADS=0 restores the fp32 recurrence together with the fp32 products: its dZ2 is bit-equal to that of a run which also
    sets S2VT_BCHAIN_SPLIT=0 (the fp32 recurrence by the knob shown to work above) -- a split recurrence left running would differ.
    Measured on MI355X, split against fp32 recurrence: lstm2_W's gradient 1.07e-6, dZ2 1.34e-6 of the maximum."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for mode, env in (("default", {}), ("rec_fp32", {"S2VT_BCHAIN_SPLIT": "0"}), ("all_fp32", {"S2VT_SPLIT_GRADS": "0"}),
                      ("all_fp32_knob", {"S2VT_SPLIT_GRADS": "0", "S2VT_BCHAIN_SPLIT": "0"})):
        out = str(tmp_path / f"{mode}.npz")
        e = dict(os.environ, S2VT_ROOT=root, **env)
        r = subprocess.run([sys.executable, "-c", CHILD_KNOB, out], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "child ok" in r.stdout, f"{mode}: rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        res[mode] = dict(np.load(out))
    for mode in res:
        assert np.isfinite(res[mode]["dZ2"]).all() and np.isfinite(res[mode]["lstm2_W"]).all(), mode
    top = np.abs(res["rec_fp32"]["lstm2_W"]).max()
    diff = np.abs(res["default"]["lstm2_W"] - res["rec_fp32"]["lstm2_W"]).max()
    ztop = np.abs(res["rec_fp32"]["dZ2"]).max()
    zdiff = np.abs(res["default"]["dZ2"] - res["rec_fp32"]["dZ2"]).max()
    print(f"split against fp32 recurrence: lstm2_W gradient {diff / top:.3e}, dZ2 {zdiff / ztop:.3e} of the maximum")
    assert zdiff > 0 and diff > 0 and diff <= 1e-5 * top
    assert np.array_equal(res["all_fp32"]["dZ2"], res["all_fp32_knob"]["dZ2"])
    assert np.abs(res["all_fp32"]["lstm2_W"] - res["all_fp32_knob"]["lstm2_W"]).max() <= 1e-5 * top


def test_dense_against_live_rows_in_the_default_mode(gpu, oracle):
    """Both forms of the split recurrence take the same three products per element: only the order of the sums differs between the dense
    and the live-row pass, so every gradient agrees within 1e-5 of its largest entry; and the [live] rows ran."""
    g_f, names_f = _pass_320(gpu, oracle, live=False)
    g_p, names_p = _pass_320(gpu, oracle, live=True)
    assert not any("[live]" in n for n in names_f) and any(n.startswith("bchain4") for n in names_f), names_f
    assert sum("chain4" in n and "[live]" in n for n in names_p) == 2, names_p                 # forward and backward recurrence of LSTM2
    assert any(n.startswith("bchain4") and "[live]" in n for n in names_p), names_p
    for k in g_f:
        ref = g_f[k].cpu().numpy(); got = g_p[k].cpu().numpy()
        assert np.isfinite(got).all(), k
        assert np.abs(got - ref).max() <= 1e-5 * (np.abs(ref).max() + 1e-12) + 1e-9, k
