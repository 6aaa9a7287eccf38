"""The bidirectional captioner's self-critical REINFORCE stage on the GPU (s2vt_amd.bidirection_rl; csrc/bidir.hip: s2vt_bidir_sample,
s2vt_bidir_teacher_forced_fwd_rows, s2vt_bidir_bptt_bwd_rows) against the restatements of tests/bidirection_rl_cases.py, which
test_bidirection_rl_cases_cpu.py shows to react to the row -> video map and the ragged mask:
  1. sampler ids bit for bit, by induction over the decode steps; the greedy block is build_sampler's; K = 0; with_greedy = False;
  2. the noise counters carry video_base: two halves of a batch sampled on their own equal the whole;
  3. the rows forward's logits equal the plain driver's on the S-times tiled block, and the CPU restatement, bit for bit;
  4. loss and all eleven gradients against float64 autograd, shared and tiled, within DESIGN.md section 3's bound for gradients;
  5. two runs of the shared backward give equal bits where the sample sum feeds order-preserving products; shared against tiled agree;
  6. guard bands around every output and input window;
  7. one step end to end: the global clip, TF-form Adam, the counters, checkpoints;
  8. the graph surface through Session.run and the train_rl --bidirectional driver."""
import json

import numpy as np
import pytest

import bidirection_cases as BC
import bidirection_rl_cases as RC

pytestmark = pytest.mark.gpu

GRAD_BOUND, LOSS_BOUND = 2e-4, 1e-3          # DESIGN.md section 3; test_gpu_bidirection_train.py's
GRAD_CASES = ["small-odd", "one-tile", "rows-65", "many-rows", "chain-range", "one-step"]

_models = {}


def _model(oracle, name, fresh=False):
    import torch
    from s2vt_amd import bidirection_rl
    if fresh or name not in _models:
        p, d, video, S = RC.case(oracle, name)
        m = bidirection_rl.Reinforce_Caption_Generator(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, video.shape[0],
                                                       d.n_video_lstm_step + d.n_caption_lstm_step, d.n_video_lstm_step, d.n_caption_lstm_step,
                                                       params=p, multisample=S)
        m.dropout_seed = BC.DROP_SEED
        if fresh:
            return m, torch.as_tensor(video).cuda()
        _models[name] = (m, torch.as_tensor(video).cuda())
    return _models[name]


def _time_major(logits):
    N, Tc, V = logits.shape
    return np.ascontiguousarray(logits.transpose(1, 0, 2)).reshape(Tc * N, V)


# ---- 1. sampler ids
@pytest.mark.parametrize("name", list(RC.SAMPLES))
def test_sampler_ids(gpu, oracle, name):
    m, video = _model(oracle, name)
    p, d, v_np, S = RC.case(oracle, name)
    B, Tc = v_np.shape[0], d.n_caption_lstm_step
    ref = RC.reference(oracle, name)
    s, g = m.sample(video, S, True, seed=RC.SAMPLE_SEED)
    assert gpu.chain_timeouts() == 0
    got = np.concatenate([s.cpu().numpy(), g.cpu().numpy()])
    assert got.dtype == np.int32 and tuple(s.shape) == (S * B, Tc) and tuple(g.shape) == (B, Tc)
    # induction over t: the ids so far are the restatement's, so its logits of step t are the logits the device picked from
    vid, sid = RC.row_ids(B, S)
    for t in range(Tc):
        want = oracle.pick_tokens(ref["logits"][:, t].copy(), vid, sid, t, RC.SAMPLE_SEED)
        assert np.array_equal(got[:, t], want), t
    assert np.array_equal(s.cpu().numpy(), ref["sampled"]) and np.array_equal(g.cpu().numpy(), ref["greedy"])
    assert np.array_equal(g.cpu().numpy(), m.build_sampler(video).cpu().numpy())
    none, g0 = m.sample(video, 0)
    assert none is None and np.array_equal(g0.cpu().numpy(), ref["greedy"])
    s1, g1 = m.sample(video, S, False, seed=RC.SAMPLE_SEED)
    assert g1 is None and np.array_equal(s1.cpu().numpy(), ref["sampled"])
    with pytest.raises(ValueError, match="early-exit"):
        m.sample(video, S, stop_at_eos=True)
    assert gpu.chain_timeouts() == 0


@pytest.mark.parametrize("name", BC.DECODING)
def test_sampler_greedy_block_at_the_unbiased_parameters(gpu, oracle, name):
    """at bidirection_cases' own parameters the greedy ids differ from video to video: the greedy block behind two sampled blocks equals
    them only if every decode row reads ITS video's partial and encoder state (row % B)"""
    import torch
    from s2vt_amd import bidirection_rl
    p, d, v_np, *_ = BC.case(oracle, name)
    m = bidirection_rl.Reinforce_Caption_Generator(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, v_np.shape[0], d.n_video_lstm_step + d.n_caption_lstm_step,
                                                   d.n_video_lstm_step, d.n_caption_lstm_step, params=p)
    s, g = m.sample(torch.as_tensor(v_np).cuda(), 2, True, seed=RC.SAMPLE_SEED)
    assert np.array_equal(g.cpu().numpy(), BC.reference(oracle, name)["ids"])
    assert gpu.chain_timeouts() == 0


# ---- 2. noise counters
@pytest.mark.parametrize("name", ["one-tile", "rows-65"])
def test_two_halves_with_their_own_video_base_equal_the_whole(gpu, oracle, name):
    m, video = _model(oracle, name)
    p, d, v_np, S = RC.case(oracle, name)
    B = v_np.shape[0]
    ref = RC.reference(oracle, name)
    h = B // 2
    parts = [m.sample(video[a:b].contiguous(), S, True, seed=RC.SAMPLE_SEED, video_base=a) for a, b in ((0, h), (h, B))]
    whole = ref["sampled"].reshape(S, B, -1)
    for (s, g), (a, b) in zip(parts, ((0, h), (h, B))):
        assert np.array_equal(s.cpu().numpy().reshape(S, b - a, -1), whole[:, a:b])
        assert np.array_equal(g.cpu().numpy(), ref["greedy"][a:b])
    assert gpu.chain_timeouts() == 0


# ---- 3. forward logits
@pytest.mark.parametrize("keep", BC.KEEPS)
@pytest.mark.parametrize("name", list(RC.SAMPLES))
def test_rows_logits_equal_the_tiled_drivers_and_the_restatement(gpu, oracle, name, keep):
    import torch
    m, video = _model(oracle, name)
    p, d, v_np, S = RC.case(oracle, name)
    B = v_np.shape[0]
    cap = torch.as_tensor(RC.reference(oracle, name)["sampled"]).cuda()
    vid, sid = (torch.as_tensor(a).cuda() for a in RC.row_ids(B, S, False))
    rows = gpu.bidir_teacher_forced_fwd_rows(m._dims(), m._params(), video, cap, m._rows_workspace(B, S), keep, BC.DROP_SEED, vid, sid)
    tiled = gpu.bidir_teacher_forced_fwd(m._dims(), m._params(), video.repeat(S, 1, 1).contiguous(), cap, m._workspace(S * B, "cuda"), keep, BC.DROP_SEED,
                                         vid, sid)
    assert gpu.chain_timeouts() == 0
    assert torch.equal(rows, tiled)
    assert np.array_equal(rows.cpu().numpy(), _time_major(RC.teacher_forced(oracle, name, keep)))
    # S = 1 is the plain driver
    one = gpu.bidir_teacher_forced_fwd_rows(m._dims(), m._params(), video, cap[:B].contiguous(), m._rows_workspace(B, 1), keep, BC.DROP_SEED, vid[:B].contiguous(),
                                            sid[:B].contiguous())
    plain = gpu.bidir_teacher_forced_fwd(m._dims(), m._params(), video, cap[:B].contiguous(), m._workspace(B, "cuda"), keep, BC.DROP_SEED, vid[:B].contiguous(),
                                         sid[:B].contiguous())
    assert torch.equal(one, plain)
    assert gpu.chain_timeouts() == 0


# ---- 4. loss and gradients
def _update_lr0(oracle, name, share, mask=None, keep=0.9):
    import torch
    m, video = _model(oracle, name)
    p, d, v_np, S = RC.case(oracle, name)
    ref = RC.reference(oracle, name)
    r, b = RC.rewards(name, S * v_np.shape[0])
    m.set_step(0)
    before = {n: m.p[n].clone() for n in m.p}
    st = m.reinforce_update(video, torch.as_tensor(ref["sampled"]).cuda(), mask, r, b, lr=0.0, keep=keep, share_lstm1=share)
    assert all(torch.equal(m.p[n], before[n]) for n in m.p)                    # lr = 0: TF-form Adam moves nothing
    from s2vt_amd import ops
    ops.zero_(m.store.m, m.store.v)                                            # (the moments it left are not part of what follows)
    m.set_step(0)
    return m, st


def _check_against_autograd(m, st, ref_loss, ref, mask_np):
    loss = float(st.loss)
    print(f"loss {loss:.6f} ref {ref_loss:.6f}")
    assert abs(loss - ref_loss) <= LOSS_BOUND * max(1.0, abs(ref_loss))
    assert float(st.mask_sum) == float(mask_np.sum())
    assert np.array_equal(st.mask.cpu().numpy(), mask_np)
    assert set(m.g) == set(ref) and len(m.g) == 11
    sumsq = 0.0
    for n in sorted(m.g):
        err = np.abs(m.g[n].cpu().numpy().astype(np.float64) - ref[n]).max() / np.abs(ref[n]).max()
        print(f"  {n}: {err:.2e}")
        assert err <= GRAD_BOUND, (n, err)
        sumsq += float((ref[n] ** 2).sum())
    assert abs(float(st.grad_sumsq) - sumsq) <= 1e-3 * sumsq
    slots = m._sumsq.cpu().numpy().astype(np.float64)
    assert abs(slots.sum() - float(st.grad_sumsq)) <= 1e-5 * sumsq and len(slots) == 11


@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("name", GRAD_CASES)
def test_loss_and_gradients_against_float64_autograd(gpu, oracle, name, share):
    from s2vt_amd import hostglue
    ref_loss, ref = RC.torch_grads(oracle, name, 0.9)
    m, st = _update_lr0(oracle, name, share)
    assert gpu.chain_timeouts() == 0
    ids = RC.reference(oracle, name)["sampled"]
    _check_against_autograd(m, st, ref_loss, ref, hostglue.masks_from_ids(ids))             # the device-derived mask is the host's


def test_a_host_mask_cut_one_step_short_of_the_longest_sample(gpu, oracle):
    name = "small-odd"
    mask = RC.reference(oracle, name)["mask"].copy()
    longest = int(mask.sum(1).max())
    mask[:, longest - 1:] = 0
    assert mask.sum() > 0 and not np.array_equal(mask, RC.reference(oracle, name)["mask"])
    ref_loss, ref = RC.torch_grads(oracle, name, 0.9, mask=mask)
    m, st = _update_lr0(oracle, name, True, mask=mask)
    assert gpu.chain_timeouts() == 0
    _check_against_autograd(m, st, ref_loss, ref, mask)


# ---- 5. determinism and the A/B switch
@pytest.mark.parametrize("name", ["small-odd", "rows-65"])
def test_shared_backward_twice_and_against_tiled(gpu, oracle, name):
    import torch
    m, _ = _update_lr0(oracle, name, True)
    first = {n: m.g[n].clone() for n in m.g}
    m, _ = _update_lr0(oracle, name, True)
    # the weight-gradient products accumulate with fp32 atomics when they split their reduction: equal bits are asserted on the sample sum
    # itself (the next test) and, for the tensors it feeds, wherever two runs of the PLAIN backward agree bit for bit at this shape
    again = {n: m.g[n].clone() for n in m.g}
    m, _ = _update_lr0(oracle, name, False)
    tiled = {n: m.g[n].clone() for n in m.g}
    m, _ = _update_lr0(oracle, name, False)
    tiled2 = {n: m.g[n].clone() for n in m.g}
    for n in ("lstm1_fw_W", "lstm1_bw_W", "encode_image_W", "lstm2_W"):
        if torch.equal(tiled[n], tiled2[n]):                                   # the products feeding it are atomic-free at this shape
            assert torch.equal(first[n], again[n]), n
    for n in first:
        scale = float(tiled[n].abs().max())
        assert float((first[n] - tiled[n]).abs().max()) <= GRAD_BOUND * scale, n
    assert gpu.chain_timeouts() == 0


@pytest.mark.parametrize("T,B,S,C", [(3, 5, 3, 128), (2, 65, 2, 256), (1, 1, 1, 4), (4, 7, 9, 36), (2, 150, 3, 192)])
def test_sample_sum_kernel_is_the_ascending_sum_and_repeatable(gpu, T, B, S, C):
    """s2vt_bidir_sample_sum on its own, guarded windows on both sides: the fp32 sum over a video's S rows in ascending s -- the same additions
    in the same order as a loop of elementwise adds, so equal bits -- and two runs agree bit for bit (one owning thread per element)"""
    import torch
    from guardband import Guarded
    rng = np.random.default_rng(T * 1000 + B)
    x = (rng.standard_normal((T, S * B, C)) * np.exp(rng.uniform(-6, 6, (T, S * B, 1)))).astype(np.float32)
    gi = Guarded.of(x.reshape(T * S * B, C), name="dZ2")
    go = Guarded(T * B, C, name="dZ2s")
    assert gi.aligned16 and go.aligned16
    xin = gi.view.view(T, S * B, C)
    gpu.bidir_sample_sum(xin, B, S, out=go.view.view(T, B, C))
    first = go.bits().copy()
    want = xin.view(T, S, B, C)[:, 0].clone()
    for s in range(1, S):
        want = want + xin.view(T, S, B, C)[:, s]
    assert np.array_equal(go.numpy().reshape(T, B, C), want.cpu().numpy())
    go.reset()
    gpu.bidir_sample_sum(xin, B, S, out=go.view.view(T, B, C))
    assert np.array_equal(go.bits(), first)
    gi.assert_intact(); go.assert_intact()
    assert gpu.chain_timeouts() == 0


# ---- 6. guard bands
@pytest.mark.parametrize("name", ["small-odd", "rows-65"])
def test_outputs_stay_inside_guard_bands(gpu, oracle, name):
    import torch
    from guardband import Guarded
    m, video = _model(oracle, name)
    p, d, v_np, S = RC.case(oracle, name)
    ref = RC.reference(oracle, name)
    B, Tc, V = v_np.shape[0], d.n_caption_lstm_step, d.n_words
    gv = Guarded.of(v_np.reshape(B, -1), name="video")
    gs = Guarded(S * B, Tc, dtype=torch.int32, name="sampled")
    gg = Guarded(B, Tc, dtype=torch.int32, name="greedy")
    gpu.bidir_sample(m._dims(), m._params(), gv.view.view(v_np.shape), S, RC.SAMPLE_SEED, 0, True, out=gs.view, ids=gg.view)
    assert np.array_equal(gs.numpy(), ref["sampled"]) and np.array_equal(gg.numpy(), ref["greedy"])
    gc = Guarded.of(ref["sampled"], dtype=torch.int32, fill=2, name="caption")
    gl = Guarded(Tc * S * B, V, name="logits")
    gpu.bidir_teacher_forced_fwd_rows(m._dims(), m._params(), gv.view.view(v_np.shape), gc.view, m._rows_workspace(B, S), keep=1.0, out=gl.view)
    assert np.array_equal(gl.numpy(), _time_major(RC.teacher_forced(oracle, name, 1.0)))
    for g in (gv, gs, gg, gc, gl):
        g.assert_intact()
    assert gpu.chain_timeouts() == 0


# ---- 7. one step end to end
def test_one_step_global_clip_adam_counters_and_checkpoints(gpu, oracle, tmp_path):
    import torch
    from s2vt_amd import bidirection, bidirection_rl, tfckpt
    name = "small-odd"
    m, video = _model(oracle, name, fresh=True)
    p, d, v_np, S = RC.case(oracle, name)
    ref = RC.reference(oracle, name)
    N = S * v_np.shape[0]
    _, g64 = RC.torch_grads(oracle, name, 0.9)
    norm = float(np.sqrt(sum((g64[n] ** 2).sum() for n in g64)))
    scale = 40.0 / norm                                                        # rewards scaled so that the global norm is 40, past 5
    r, b = RC.rewards(name, N)
    lr = 1e-3
    st = m.reinforce_update(video, torch.as_tensor(ref["sampled"]).cuda(), None, r * np.float32(scale), b * np.float32(scale), lr=lr, keep=0.9)
    assert gpu.chain_timeouts() == 0
    assert m.global_step == 1 and m.adam_t == 1 and int(m._applied.item()) == 1
    gn = float(np.sqrt(float(st.grad_sumsq)))
    assert abs(gn - 40.0) <= 0.05
    # TF-form Adam's first step on the globally clipped gradient, float64: one factor 5 / norm for EVERY variable
    fac = 5.0 / max(gn, 5.0)
    lr_t = lr * np.sqrt(1 - 0.999) / (1 - 0.9)
    for n in m.p:
        g = g64[n] * scale * fac
        m1, v1 = 0.1 * g, 0.001 * g * g
        want = p[n].astype(np.float64) - lr_t * m1 / (np.sqrt(v1) + 1e-8)
        big = np.abs(g) > 1e-3 * np.abs(g).max()                               # (where g ~ 0 the step's sign is the gradient error's)
        assert np.abs(m.p[n].cpu().numpy() - want)[big].max() <= 0.02 * lr, n
        assert np.allclose(m.store._view(m.store.m, n).cpu().numpy(), m1, rtol=0, atol=2e-3 * np.abs(m1).max()), n
    # a clip per variable would have left the small variables' steps unscaled: the factor is visibly one
    small = min(g64, key=lambda n: float((g64[n] ** 2).sum()))
    assert np.sqrt(float((g64[small] ** 2).sum())) * scale < 5.0
    mom = m.store._view(m.store.m, small).cpu().numpy()
    assert np.allclose(mom, 0.1 * g64[small] * scale * fac, rtol=0, atol=2e-3 * np.abs(mom).max())
    # checkpoint round trip: variables, moments, adam_t, g_step
    path = str(tmp_path / "rl-0")
    m.save(path)
    names = set(tfckpt.read_checkpoint(path))
    assert {"Wemb/Adam", "Wemb/Adam_1", "s2vt/LSTM2/basic_lstm_cell/weights/Adam", "beta1_power", "beta2_power", "adam_t", "g_step"} <= names
    fresh, _ = _model(oracle, name, fresh=True)
    fresh.restore(path)
    assert fresh.global_step == 1 and fresh.adam_t == 1
    for n in m.p:
        assert torch.equal(fresh.p[n], m.p[n]), n
    assert torch.equal(fresh.store.m, m.store.m) and torch.equal(fresh.store.v, m.store.v) and float(m.store.v.abs().max()) > 0
    # an XE checkpoint of the script's class restores optimistically: variables, zero moments, counters at zero
    xe = bidirection.Video_Caption_Generator(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, 1, 0, d.n_video_lstm_step, d.n_caption_lstm_step, seed=9)
    xe.global_step = 7
    xpath = str(tmp_path / "bimodel-0")
    xe.save(xpath)
    fresh.restore(xpath)
    assert fresh.global_step == 0 and fresh.adam_t == 0
    for n in xe.p:
        assert torch.equal(fresh.p[n], xe.p[n]), n
    assert float(fresh.store.m.abs().max()) == 0.0 and float(fresh.store.v.abs().max()) == 0.0
    assert isinstance(fresh, bidirection_rl.Reinforce_Caption_Generator)


# ---- 8. class surface and driver
def test_graph_surface_through_session_run(gpu, oracle):
    import torch
    from s2vt_amd import bidirection_rl
    name = "small-odd"
    m, video = _model(oracle, name, fresh=True)
    p, d, v_np, S = RC.case(oracle, name)
    ref = RC.reference(oracle, name)
    B = v_np.shape[0]
    r, b = RC.rewards(name, S * B)
    sess = bidirection_rl.Session(m)
    sampled, vph = m.build_multinomial_sampler()
    ids = sess.run(sampled, {vph: v_np})
    assert ids.shape == (B, d.n_caption_lstm_step) and ids.dtype == np.int64
    s1, _ = m.sample(video, 1, False, seed=m.sample_seed + 7919)
    assert np.array_equal(ids, s1.cpu().numpy())
    outs = m.build_loss()
    loss, video_ph, cap_ph, mask_ph = outs
    tiled = np.tile(v_np, (S, 1, 1))
    feed = {video_ph: tiled, cap_ph: ref["sampled"], mask_ph: ref["mask"]}
    lpm = sess.run(loss, feed)
    assert lpm.shape == ref["sampled"].shape and (lpm[ref["mask"] == 0] == 0).all() and (lpm[ref["mask"] == 1] < 0).all()
    rew, base = m.placeholder("rewards"), m.placeholder("base_line")
    train_op, sum_loss = m.reinforce_train_op(outs, rew, base, 0.0)
    feed.update({rew: r, base: b})
    _, sl = sess.run([train_op, sum_loss], feed)
    assert m.global_step == 1
    want = -float((lpm.astype(np.float64) * (r - b).astype(np.float64)[:, None]).sum() / ref["mask"].sum())
    assert abs(sl - want) <= 1e-5 * max(1.0, abs(want))                       # the same pass: dropout seed of step 0, lr = 0 moved nothing
    m.set_step(0)
    st = m.reinforce_update(video, ref["sampled"], ref["mask"], r, b, lr=0.0)
    assert abs(float(st.loss) - sl) <= 1e-6 * max(1.0, abs(sl))
    # the script's own graphs still run through the same session
    gen_video, sentence, _ = m.build_generator()
    sent = sess.run(sentence, {gen_video: v_np[:1]})
    assert np.array_equal(sent, m.build_sampler(video[:1].contiguous(), unshifted_softmax=True)[0].cpu().numpy())
    assert gpu.chain_timeouts() == 0


def test_train_rl_bidirectional_driver(gpu, tmp_path):
    from test_gpu_train_drivers import _corpus
    from s2vt_amd import tfckpt, train_common as tc, train_rl
    rng = np.random.default_rng(0)
    sents, feats, vocab = _corpus(tmp_path, "train", rng)
    corpus = tc.Corpus(sents, feats, vocabulary=vocab)
    cfg = train_rl.rl_config(dim_image=24, lstm_dim=32, word_dim=16, n_video_lstm_step=3, n_caption_lstm_step=8, n_epochs=1, batch_size=8, multisample=3,
                             start_learning_rate=1e-3, max_steps_per_epoch=3, model_path=str(tmp_path / "m"), model_name="rlbi",
                             step_log=str(tmp_path / "rl.jsonl"))
    model, hist = train_rl.train_bidirectional(cfg, corpus, log=lambda *_: None)
    steps = [r for r in map(json.loads, open(tmp_path / "rl.jsonl")) if r["kind"] == "step"]
    assert len(steps) == 3 and model.global_step == 3 and [r["step"] for r in steps] == [1, 2, 3]
    assert all(np.isfinite(r["loss"]) and "reward" in r and "baseline" in r for r in steps)
    sd = tfckpt.read_checkpoint(hist[-1]["checkpoint"])
    assert int(sd["g_step"]) == 3 and "s2vt/LSTM1/bidirectional_rnn/bw/basic_lstm_cell/weights/Adam_1" in sd
    cfg2 = train_rl.rl_config(**{**cfg.__dict__, "model_name": "rlbi2", "step_log": str(tmp_path / "rl2.jsonl"), "max_steps_per_epoch": 1})
    model2, _ = train_rl.train_bidirectional(cfg2, corpus, log=lambda *_: None, resume=hist[-1]["checkpoint"])
    steps2 = [r for r in map(json.loads, open(tmp_path / "rl2.jsonl")) if r["kind"] == "step"]
    assert steps2[0]["step"] == 4 and model2.adam_t == 4
    assert gpu.chain_timeouts() == 0


@pytest.mark.parametrize("extra", [["--residual"], ["--mix-baseline", "0.9"], ["--stop-at-eos"], ["--attr-vocab", "a"], ["--grad-precision", "bf16"]])
def test_flag_does_not_combine(gpu, extra):
    from s2vt_amd import train_rl
    assert callable(train_rl.train_bidirectional)                              # (without the driver the flag itself would be the error)
    with pytest.raises(SystemExit):
        train_rl.main(["--train-sents", "s", "--train-feats", "f", "--vocab", "v", "--bidirectional"] + extra)


def test_the_scripts_class_still_refuses(gpu, oracle):
    from s2vt_amd import bidirection
    p, d, video, S = RC.case(oracle, "small-odd")
    m = bidirection.Video_Caption_Generator(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, 1, 0, d.n_video_lstm_step, d.n_caption_lstm_step, params=p)
    for fn in (m.sample, m.reinforce_update):
        with pytest.raises(ValueError, match="no graph"):
            fn(None)
    from s2vt_amd import bidirection_rl
    assert issubclass(bidirection_rl.Reinforce_Caption_Generator, bidirection.Video_Caption_Generator)
    assert bidirection_rl.Reinforce_Caption_Generator.sample is not bidirection.Video_Caption_Generator.sample
    assert gpu.chain_timeouts() == 0
