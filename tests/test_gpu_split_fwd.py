"""The split-bf16 forward of an update (s2vt_teacher_forced_fwd_split), each S2VT_SPLIT_FWD setting in a fresh child process
(the env is read once).  Stage 1: every history of the training workspace bit for bit that of the fp32 forward, the logits within the
per-row, per-column margin the pick screen proves for this product and arithmetic (csrc/pick_screen.hip), live-row logits the
dense call's rows bit for bit, the dlogits planes' region of the split workspace untouched, and the same bits under S2VT_SPLIT_FUSED=0
(row planes in AT, or in BT where that carve leaves AT short).  Stage 2: the decode partials read back from dZ2p in live mode, and LSTM2's
step-0 gates (all encode rows where Tv = 1), against the float64 sum of the three split products of the same operands; one whole REINFORCE
update against float64 autograd.  All stages: two runs give equal bits; stage 0 is the fp32 forward, down to the loss bits recorded from
the build before this entry.  The workspace contract of the new entry with the helpers of tests/workspace_contract.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_workspace_contract as WC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (D, V, E, H, Tv, Tc), B, rep: the smallest shapes that take the split mode (N = 320 and N = 264 rows); H % 64 != 0 in both, V and
# H + E no multiples of the tile, E = 500 puts the embedding columns of stage B's planes across several K steps
# "tv1": one encode step, so that EVERY encode row's partial is observable (below); "h64": bf16_pad(H + 1) = 2 H, where the carve of
# S2VT_SPLIT_FUSED=0 leaves AT too short for stage A's row planes and they go to BT
SHAPES = {"a": ((128, 300, 40, 136, 2, 3), 64, 5), "b": ((128, 1100, 500, 264, 2, 3), 33, 8), "tv1": ((128, 300, 40, 136, 1, 3), 64, 5),
          "h64": ((128, 300, 40, 64, 2, 3), 64, 5)}
# name -> (shape, residual, live: False | "third" (a third of the positions masked) | "all" (every position listed))
CASES = {"a": ("a", False, False), "b": ("b", False, False), "residual": ("a", True, False), "live": ("a", False, "third"),
         "live_b": ("b", False, "all"), "tv1": ("tv1", False, False), "h64": ("h64", False, False)}
HIST = ("H1", "C1", "H2", "C2", "G2", "O2")


def _pad(n, m):
    return (n + m - 1) // m * m


def train_regions(dims, B, N):
    """Byte (offset, count) of the leading regions of the training workspace, in the order carve_train takes them (each rounded up to 256)."""
    D, V, E, H, Tv, Tc = dims
    T = Tv + Tc
    order = [("emb", B * Tv * E), ("Xp1", B * Tv * 4 * H), ("prev", Tc * N), ("tgt", Tc * N), ("encidx", Tv * B), ("G1", T * B * 4 * H),
             ("C1", (T + 1) * B * H), ("H1", (T + 1) * B * H), ("O1", T * N * H), ("G2", T * N * 4 * H), ("C2", (T + 1) * N * H),
             ("H2", (T + 1) * N * H), ("O2", T * N * H), ("dO2", Tc * N * H), ("dO2p", Tc * N * H), ("dZ2p", Tc * N * 4 * H)]
    out, off = {}, 0
    for name, n in order:
        out[name] = (off, n * 4)
        off += _pad(n * 4, 256)
    return out


def l_region_bytes(dims, B, N):
    """Bytes of one plane set's L region in the split workspace (carve_bf16: the first take)."""
    D, V, E, H, Tv, Tc = dims
    Kv, K4 = _pad(V, 64), _pad(4 * H, 64)
    return _pad(2 * max(Tc * N * Kv, (Tv + Tc) * N * K4, Tv * B * K4), 256)


def make_case(name):
    from oracle import s2vt_oracle as orc
    shape, residual, live = CASES[name]
    dims, B, rep = SHAPES[shape]
    d = orc.Dims(dim_image=dims[0], n_words=dims[1], word_dim=dims[2], lstm_dim=dims[3], n_video_lstm_step=dims[4], n_caption_lstm_step=dims[5],
                 label_dim=0)
    p = orc.init_params(d, seed=3)
    rng = np.random.default_rng(4 + len(name))
    for k in ("lstm1_b", "lstm2_b", "encode_image_b", "embed_word_b"):
        p[k] = rng.uniform(-.1, .1, p[k].shape).astype(np.float32)
    N, Tc = B * rep, dims[5]
    video = np.abs(rng.standard_normal((B, dims[4], dims[0])) * 0.5).astype(np.float32)
    cap = rng.integers(2, dims[1], (N, Tc)).astype(np.int32)
    live_rows = None
    if live:                                                     # a third of the positions masked, closed towards earlier steps
        ln = rng.integers(1, Tc + 1, N)                          # lengths 1 .. Tc, equally likely: (Tc - 1) / (2 Tc) = a third at Tc = 3
        if live == "all":
            ln[:] = Tc
        mask = np.arange(Tc)[None, :] < ln[:, None]
        live_rows = np.flatnonzero(mask.T.reshape(-1)).astype(np.int32)
        assert live == "all" or 0.27 < 1 - len(live_rows) / (Tc * N) < 0.40
    vid = np.tile(np.arange(B, dtype=np.int32) + 5, rep)
    sid = np.repeat(np.arange(rep, dtype=np.int32), B)
    return dict(dims=dims, B=B, N=N, residual=residual, p=p, video=video, cap=cap, live=live_rows, vid=vid, sid=sid)


def run_case(name):
    """One case in this process: the fp32 forward, then the split entry twice on a split workspace filled with a byte pattern."""
    import torch
    from s2vt_amd import ops
    c = make_case(name)
    dims, B, N = c["dims"], c["B"], c["N"]
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    gd = ops.make_dims(*dims, residual=c["residual"])
    keep_alive = {k: dv(v) for k, v in c["p"].items() if v is not None}
    params = ops.make_params(keep_alive)
    video, cap, vid, sid = dv(c["video"]), dv(c["cap"]), dv(c["vid"]), dv(c["sid"])
    live = None if c["live"] is None else dv(c["live"])
    reg = train_regions(dims, B, N)
    out = {}

    def fwd(split, lv):
        ws = ops.train_workspace(gd, B, N, video.device)        # (the cached buffer the call below takes)
        ws.zero_()
        logits, ws = ops.teacher_forced_fwd(gd, params, video, cap, N, 0.9, 99, vid, sid, live=lv, split=split)
        torch.cuda.synchronize()
        return logits.cpu().numpy(), {h: ws[reg[h][0]:reg[h][0] + reg[h][1]].cpu().numpy().view(np.float32) for h in HIST + ("O1", "dZ2p", "prev")}

    out["logits_fp32"], h0 = fwd(False, live)
    for h, v in h0.items():
        out["fp32_" + h] = v
    sws = ops.split_grad_workspace(gd, B, N, video.device)
    sws.fill_(0xA5)
    out["logits_split"], h1 = fwd(True, live)
    for h, v in h1.items():
        out["split_" + h] = v
    lb = l_region_bytes(dims, B, N)
    lo_off = C.c_size_t()
    hi_off, ld = C.c_size_t(), C.c_int32()
    ops.check(ops.lib().s2vt_split_grad_dlogits_planes(C.byref(gd), B, N, C.byref(hi_off), C.byref(lo_off), C.byref(ld)), "planes")
    out["L_untouched"] = np.int32(bool((sws[hi_off.value:hi_off.value + lb] == 0xA5).all()) and bool((sws[lo_off.value:lo_off.value + lb] == 0xA5).all()))
    out["ws_written"] = np.int32(bool((sws != 0xA5).any()))
    again, h2 = fwd(True, live)
    out["same_twice"] = np.int32(again.tobytes() == out["logits_split"].tobytes() and all(h1[h].tobytes() == h2[h].tobytes() for h in h1))
    if live is not None:
        out["logits_split_dense"], _ = fwd(True, None)
    out["stage"] = np.int32(ops.split_fwd_active(N))
    return out


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_split_fwd as T
for name in (sys.argv[3].split(",") if len(sys.argv) > 3 else T.CASES):
    np.savez(sys.argv[2] + "_" + name + ".npz", **T.run_case(name))
"""

_CHILD_UPDATE = r"""
import sys, json
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from test_gpu_split_grads import _rl_update
from test_gpu_bf16_grads import _ref_grads
from oracle import s2vt_oracle as oracle
mdl, video, cap, mask, r, b, run = _rl_update()
out = {}
if sys.argv[3] == "ref":
    B, K = 64, 5
    vid = np.tile(np.arange(B, dtype=np.int32), K); sid = np.repeat(np.arange(K, dtype=np.int32), B)
    ref_loss, ref_g = _ref_grads(mdl, np.tile(video, (K, 1, 1)), cap, vid, sid, 0.9, lambda T, pt, lg: T.pg_loss(lg, cap, mask, r, b), oracle)
step0 = mdl.global_step
st = run()
mdl.global_step = step0
g1 = {n: mdl.store.g[n].cpu().numpy().copy() for n in mdl.store.names}
out["loss"] = np.float32(float(st.loss)).tobytes().hex()
out["mask_sum"] = np.float32(float(st.mask_sum)).tobytes().hex()
st2 = run()
out["loss_twice"] = np.float32(float(st2.loss)).tobytes().hex()
if sys.argv[3] == "ref":
    out["loss_value"], out["ref_loss"] = float(st.loss), ref_loss
    out["grad_err"] = {n: float(np.abs(g1[n].astype(np.float64) - ref_g[n]).max() / (np.abs(ref_g[n]).max() + 1e-30)) for n in ref_g}
print(json.dumps(out))
"""


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("S2VT_SPLIT_FWD", "S2VT_SPLIT_GRADS", "S2VT_SPLIT_FUSED")}
    env.update(kw)
    return env


@pytest.fixture(scope="module")
def staged(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("split_fwd")
    for stage in ("0", "1", "2"):
        subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(d / f"s{stage}")], check=True, env=_env(S2VT_SPLIT_FWD=stage), timeout=300)
    out = {(stage, name): np.load(str(d / f"s{stage}_{name}.npz")) for stage in ("0", "1", "2") for name in CASES}
    # stage A with the backward's unfused operand layout: the forward must not follow that knob
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(d / "u1"), "a,h64"], check=True, env=_env(S2VT_SPLIT_FWD="1", S2VT_SPLIT_FUSED="0"),
                   timeout=300)
    out.update({("1u", name): np.load(str(d / f"u1_{name}.npz")) for name in ("a", "h64")})
    return out


def _o2_rows(r, name):
    """The rows the logits product read: the decode part of O2 (the residual sum already in place), the live ones when listed."""
    c = make_case(name)
    D, V, E, H, Tv, Tc = c["dims"]
    o2 = r["fp32_O2"].reshape(Tv + Tc, c["N"], H)[Tv:].reshape(-1, H)
    return (o2 if c["live"] is None else o2[c["live"]]), c


def _screen_bound(h, W, bias, fp32_logits):
    """The pick screen's proof for this product (csrc/pick_screen.hip): |fp32 chain - split product| <= m = C |h_r| |W[:, v]|, C = 2^-10 per
    1024 terms, plus the roundings of (logit + bias) on either side, each within 2^-24 of a value no larger than |logit| + m: the screen's
    slack (|v| + m + 1) 2^-20 covers both."""
    K = h.shape[1]
    Cc = 2.0 ** -10 * ((K + 1023) // 1024)
    m = Cc * np.sqrt((h.astype(np.float64) ** 2).sum(1))[:, None] * np.sqrt((W.astype(np.float64) ** 2).sum(0))[None, :]
    return m + (np.abs(fp32_logits.astype(np.float64)) + m + 1.0) * 2.0 ** -20


@pytest.mark.parametrize("name", list(CASES))
def test_stage0_is_the_fp32_forward(staged, name):
    r = staged[("0", name)]
    assert int(r["stage"]) == 0 and int(r["same_twice"]) == 1
    assert r["logits_split"].tobytes() == r["logits_fp32"].tobytes()
    for h in HIST:
        assert r["split_" + h].tobytes() == r["fp32_" + h].tobytes(), h
    assert int(r["ws_written"]) == 0                                    # the fp32 products never touch the split workspace


@pytest.mark.parametrize("name", list(CASES))
def test_stage_a_histories_equal_and_logits_within_the_screen_margin(staged, name):
    r = staged[("1", name)]
    assert int(r["stage"]) == 1 and int(r["ws_written"]) == 1
    for h in HIST:
        assert r["split_" + h].tobytes() == r["fp32_" + h].tobytes(), h
    h, c = _o2_rows(r, name)
    bound = _screen_bound(h, c["p"]["embed_word_W"], c["p"]["embed_word_b"], r["logits_fp32"])
    err = np.abs(r["logits_split"].astype(np.float64) - r["logits_fp32"].astype(np.float64))
    assert err.shape == bound.shape
    print(f"\nstage A {name}: max |split - fp32| = {err.max():.3e}, max ratio to the screen margin = {(err / bound).max():.4f}")
    assert np.isfinite(r["logits_split"]).all()
    assert (err <= bound).all()
    assert err.max() > 0                                                # (the split product did run)
    assert int(r["L_untouched"]) == 1 and int(r["same_twice"]) == 1
    if c["live"] is not None:
        assert r["logits_split"].tobytes() == r["logits_split_dense"][c["live"]].tobytes()


@pytest.mark.parametrize("name", ["a", "h64"])
def test_stage_a_does_not_follow_the_backwards_layout_knob(staged, name):
    """S2VT_SPLIT_FUSED=0 (the backward's transposed operands; its carve does not count stage A's row planes in AT): the same split
    logits bit for bit -- from AT where they fit ("a"), from BT where AT is too short ("h64": 960 x 128 elements against 64 x 1600)."""
    u, f = staged[("1u", name)], staged[("1", name)]
    if name == "h64":
        D, V, E, H, Tv, Tc = SHAPES["h64"][0]
        N = SHAPES["h64"][1] * SHAPES["h64"][2]
        at_unfused = max(H * (_pad(Tv * N, 64) + _pad(Tc * N, 64)), E * _pad(Tc * N, 64), D * _pad(Tv * 64, 64))
        assert Tc * N * _pad(H + 1, 64) > at_unfused                   # (the shape does leave AT short)
    assert int(u["stage"]) == 1 and int(u["ws_written"]) == 1 and int(u["same_twice"]) == 1
    assert u["logits_split"].tobytes() == f["logits_split"].tobytes()
    assert u["logits_split"].tobytes() != u["logits_fp32"].tobytes()
    for h in HIST:
        assert u["split_" + h].tobytes() == u["fp32_" + h].tobytes(), h


def _split64(x):
    import torch
    from test_gpu_split_grads import _split_ref
    return tuple(t.double().numpy() for t in _split_ref(torch.as_tensor(np.ascontiguousarray(x))))


@pytest.mark.parametrize("name", ["live", "live_b"])
def test_stage_b_decode_partials_vs_float64(staged, name):
    """The decode product [O1[Tv:] ; Wemb[prev]] . lstm2_W[0 : H + E] itself: in live mode the packed partials stay in the workspace
    (dZ2p) behind the forward.  Against the float64 sum of the three split products of the same operands -- the rows gathered through the
    live list, the embedding rows through the previous words -- within the x3-vs-float64 bound of the product's maximum.  "live": a third
    masked (640 rows); "live_b": every position listed (792 rows = the dense product's size), E = 500: the embedding columns span K steps
    and K = 764 is padded to 768."""
    r = staged[("2", name)]
    c = make_case(name)
    D, V, E, H, Tv, Tc = c["dims"]
    N, live = c["N"], c["live"]
    o1 = r["split_O1"].reshape(Tv + Tc, N, H)[Tv:].reshape(-1, H)[live]
    prev_tm = np.concatenate([np.ones((N, 1), np.int32), c["cap"][:, :-1]], 1).T.reshape(-1)     # <bos> = 1, then the caption shifted
    assert np.array_equal(r["split_prev"].view(np.int32)[:Tc * N], prev_tm)
    x = np.concatenate([o1, c["p"]["Wemb"][prev_tm[live]]], 1)
    (ah, al), (bh, bl) = _split64(x), _split64(c["p"]["lstm2_W"][:H + E])
    prod = ah @ bh + ah @ bl + al @ bh
    got = r["split_dZ2p"][:len(live) * 4 * H].reshape(len(live), 4 * H).astype(np.float64)
    bound = 1e-6 * max(1.0, ((H + E) / 1000) ** 0.5) * np.abs(prod).max()
    err = np.abs(got - prod).max()
    print(f"\nstage B {name}: decode partials [{len(live)} x {4 * H}], K = {H + E}: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    # (and they are the split product's, not the fp32 chain's: the fp32 run of the same case left other bits there)
    assert r["split_dZ2p"][:len(live) * 4 * H].tobytes() != r["fp32_dZ2p"][:len(live) * 4 * H].tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_stage_b_step0_gates_and_logits(staged, name, oracle):
    """LSTM2's step 0 starts from zero states, so its activated gates are act(partial + b): against the oracle's pointwise step on a
    float64 sum of the three split products of the same operands (O1[0] . lstm2_W[0:H], hi / lo planes as the casts make them); an
    activation's slope is at most 1, so the gates differ by no more than the partial does -- the x3-vs-float64 bound of the product's
    maximum -- plus the rounding of z to fp32.  The recurrence overwrites an encode partial with the step's gates, and from step 1 on
    those contain h . W_rec as well: only step 0 shows the partial alone.  In the "tv1" case (one encode step) step 0 is ALL Tv . N encode
    rows, three row tiles of the product; the decode partials are read directly in test_stage_b_decode_partials_vs_float64."""
    r = staged[("2", name)]
    c = make_case(name)
    D, V, E, H, Tv, Tc = c["dims"]
    N = c["N"]
    assert int(r["stage"]) == 2 and int(r["L_untouched"]) == 1 and int(r["same_twice"]) == 1
    for hname in ("H1", "C1"):                                          # LSTM1 and the dropout of its output are not touched
        assert r["split_" + hname].tobytes() == r["fp32_" + hname].tobytes(), hname
    assert r["split_O1"].tobytes() == r["fp32_O1"].tobytes()
    (ah, al), (bh, bl) = _split64(r["split_O1"].reshape(Tv + Tc, N, H)[0]), _split64(c["p"]["lstm2_W"][:H])
    prod = ah @ bh + ah @ bl + al @ bh
    z = (prod + c["p"]["lstm2_b"].astype(np.float64)).astype(np.float32)
    _, _, _, gates = oracle.lstm_pointwise(z, np.zeros((N, H), np.float32), want_gates=True)
    got = r["split_G2"].reshape(Tv + Tc, N, 4 * H)[0]
    bound = 1e-6 * max(1.0, (H / 1000) ** 0.5) * np.abs(prod).max() + 2.0 ** -22 * (np.abs(z).max() + 1.0)
    err = np.abs(got.astype(np.float64) - gates.astype(np.float64)).max()
    print(f"\nstage B {name}: step-0 gates max err {err:.3e}, bound {bound:.3e}; states vs fp32: "
          + ", ".join(f"{h} {np.abs(r['split_' + h] - r['fp32_' + h]).max():.2e}" for h in ("H2", "C2", "O2")))
    assert err <= bound
    assert got.tobytes() != r["fp32_G2"].reshape(Tv + Tc, N, 4 * H)[0].tobytes()      # (the split product did run)
    assert np.isfinite(r["logits_split"]).all() and all(np.isfinite(r["split_" + hname]).all() for hname in HIST)
    if c["live"] is not None:
        assert r["logits_split"].tobytes() == r["logits_split_dense"][c["live"]].tobytes()


def _update(env, mode="run"):
    p = subprocess.run([sys.executable, "-c", _CHILD_UPDATE, ROOT, "-", mode], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_stage0_update_is_the_fp32_forwards(gpu):
    """reinforce_update at the rl shape (test_gpu_split_grads._rl_update, lr = 0): S2VT_SPLIT_FWD=0 gives the loss and sum(mask) bits that
    the library gave before the split forward existed, with its split backward on -- recorded from that build in
    tests/golden/split_fwd_rl_update.json -- and those of the model without the split mode (S2VT_SPLIT_GRADS=0: the live entry).
    Printed beside them: the default stage's loss.  At this shape and seed stage 1's loss ROUNDS to the same fp32 bits as the fp32
    forward's (its logits differ by ~1e-6): that is a coincidence of this case, which tests/test_gpu_split_grads.py::
    test_split_knob_off_is_fp32_body (loss bits across S2VT_SPLIT_GRADS) relies on with stage 1 as the default -- DESIGN.md section 5.  If that
    test fails after a change of seed, shape or kernel while this one passes, the forward is as exact as before and only the coincidence
    is gone."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "split_fwd_rl_update.json")))
    off, plain, default = _update(_env(S2VT_SPLIT_FWD="0")), _update(_env(S2VT_SPLIT_GRADS="0")), _update(_env())
    print(f"\nloss bits: golden {golden['loss']}, S2VT_SPLIT_FWD=0 {off['loss']}, S2VT_SPLIT_GRADS=0 {plain['loss']}, default stage {default['loss']}")
    assert off["loss"] == golden["loss"] and off["mask_sum"] == golden["mask_sum"]
    assert off["loss"] == plain["loss"] and off["mask_sum"] == plain["mask_sum"]
    assert off["loss"] == off["loss_twice"]


def test_stage_b_update_vs_float64_autograd(gpu):
    """One reinforce_update (lr = 0) at the rl shape under S2VT_SPLIT_FWD=2 against float64 autograd: the bounds of
    test_gpu_timed_tiles._compare -- 1e-3 on the loss, 2e-4 of each gradient's maximum."""
    out = _update(_env(S2VT_SPLIT_FWD="2"), "ref")
    print("\nstage B update: loss", out["loss_value"], "ref", out["ref_loss"], "grad err", {k: f"{v:.2e}" for k, v in out["grad_err"].items()})
    assert abs(out["loss_value"] - out["ref_loss"]) <= 1e-3 * max(1.0, abs(out["ref_loss"]))
    for n, e in out["grad_err"].items():
        assert e <= 2e-4, (n, e)
    assert out["loss"] == out["loss_twice"]


# ---------------------------------------------------------------------------------------------------- the workspace contract
class SplitFwd(WC.Train):
    """s2vt_teacher_forced_fwd_split (dense or live rows) + s2vt_bptt_bwd_split on caller-owned (ptr, bytes)."""

    @WC._stage
    def fwd(self, ops, env, s, i, state):
        import s2vt_amd
        L = s2vt_amd.lib()
        dims, params = self._setup(ops, s, i, state)
        N = i["N"]
        tws = env.ws(L.s2vt_train_workspace_bytes(C.byref(dims), s.B, N), "train")
        sws = env.ws(L.s2vt_split_grad_workspace_bytes(C.byref(dims), s.B, N), "split_grad")
        logits = env.empty((self._rows(i), dims.n_words))
        lv = (WC._p(state["live"]), len(i["live"])) if self.f == "live" else (None, 0)
        steps = i["steps"] if self.f == "live" else dims.n_caption_lstm_step
        rc = L.s2vt_teacher_forced_fwd_split(C.byref(dims), C.byref(params), WC._p(state["video"]), s.B, N, WC._p(state["cap"]), steps, *lv,
                                             i["keep"], i["seed"], WC._p(state["vid"]), WC._p(state["sid"]), WC._p(logits), WC._p(tws), tws.numel(),
                                             None, 0, 0, WC._p(sws), sws.numel(), WC._stream())
        s2vt_amd._lib.check(rc, "s2vt_teacher_forced_fwd_split")
        state["logits"] = logits

    def check(self, s, i, state):
        """The oracle's logits within the proven margin of this product: |h_r| <= sqrt(H) / keep (an LSTM output is within [-1, 1], dropout
        scales it by 1 / keep), twice that for the residual sum; the gradients within the split backward's bound."""
        d = i["d"]
        ref_logits, ref_g = WC._train_reference(s)
        tm = np.ascontiguousarray(ref_logits.transpose(1, 0, 2)).reshape(-1, d.n_words)
        want = tm[i["live"]] if self.f == "live" else tm[:self._rows(i)]
        H = d.lstm_dim
        hn = (2.0 if s.kind == "residual" else 1.0) * np.sqrt(H) / i["keep"]
        wn = np.sqrt((i["p"]["embed_word_W"].astype(np.float64) ** 2).sum(0))[None, :]
        m = 2.0 ** -10 * ((H + 1023) // 1024) * hn * wn
        bound = m + (np.abs(want.astype(np.float64)) + m + 1.0) * 2.0 ** -20
        assert (np.abs(state["logits"].cpu().numpy().astype(np.float64) - want) <= bound).all()
        dv = state["grads"].pop("d_video")
        WC._assert_grads(state["grads"], {k: v for k, v in ref_g.items() if k != "d_video"}, WC.GRAD_BOUND, f"split fwd {self.f}+{self.b}")
        assert WC._rel(dv.cpu().numpy(), ref_g["d_video"]) <= WC.DVIDEO_BOUND


@pytest.mark.parametrize("fwd", ["plain", "live"])
def test_split_forward_workspace_contract(gpu, fwd):
    """Exact-size dirty windows, a larger shape's windows, containment, and the refusals: a split workspace 256 bytes short is
    S2VT_E_WORKSPACE with nothing written."""
    fam, (_, rows320, _) = SplitFwd(fwd, "split"), WC._train_shapes()
    WC._check_A(fam, rows320)
    WC._check_C(fam, rows320, WC._train_larger(rows320))
    WC._check_D(fam, rows320)


def test_split_forward_refuses_a_misaligned_split_workspace(gpu):
    import torch
    import s2vt_amd
    from s2vt_amd import ops
    L = s2vt_amd.lib()
    c = make_case("a")
    gd = ops.make_dims(*c["dims"])
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    keep_alive = {k: dv(v) for k, v in c["p"].items() if v is not None}
    params = ops.make_params(keep_alive)
    B, N = c["B"], c["N"]
    tws = ops.train_workspace(gd, B, N, "cuda")
    nb = L.s2vt_split_grad_workspace_bytes(C.byref(gd), B, N)
    sws = torch.full((nb + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    logits = torch.zeros(c["dims"][5] * N, c["dims"][1], device="cuda")
    video, cap, vid, sid = dv(c["video"]), dv(c["cap"]), dv(c["vid"]), dv(c["sid"])
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = L.s2vt_teacher_forced_fwd_split(C.byref(gd), C.byref(params), p(video), B, N, p(cap), c["dims"][5], None, 0, 0.9, 99, p(vid), p(sid), p(logits),
                                         p(tws), tws.numel(), None, 0, 0, C.c_void_p(sws.data_ptr() + 128), nb, None)
    torch.cuda.synchronize()
    assert rc == -2
    assert bool((sws == 0x5A).all()) and not logits.any()
    rc = L.s2vt_teacher_forced_fwd_split(C.byref(gd), C.byref(params), p(video), B, N, p(cap), c["dims"][5], None, 0, 0.9, 99, p(vid), p(sid), p(logits),
                                         p(tws), tws.numel(), None, 0, 0, None, nb, None)
    assert rc == -1
