"""Self-critical REINFORCE on the temporal-attention captioner: the multinomial sampler, the teacher-forced unroll and its backward on
rows that share image blocks, the update, the class surface and the driver.

Rows are sample-major: row s * B + j is sample s of video j; the greedy block comes last with sample id -1.  The shapes are tiny (the
oracle unrolls and the float64 autograd take a second or two); embed_word_b[0] = 3 makes <eos> likely, so samples end early and the
mask is exercised.  H = 36 is no multiple of 16; B = 24, K = 3 is 72 rows, past the 64-row boundary of the other attention paths.

1. sampler ids bit-exact: the returned ids teacher-forced through oracle.attention_forward, oracle.pick_tokens on every step's logits;
2. the unroll on shared blocks bit-exact vs the oracle and vs the plain entry point on the tiled block;
3. loss and every gradient of reinforce_update vs float64 autograd (hinge open and closed, shared and tiled);
4. one step end to end (clip, TF-Adam, counters, health);  5. build_multinomial_sampler / build_loss / reinforce_train_op;
6. train_attention.train(reinforce=True)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

#          D,  V,   H,  Tv, Tc, B,  K
SHAPES = [(48, 131, 32, 5, 6, 5, 3), (40, 97, 36, 12, 4, 7, 2), (40, 97, 36, 32, 4, 7, 2), (48, 131, 32, 5, 6, 24, 3)]
SEED = 11


def _oracle():
    from oracle import s2vt_oracle
    s2vt_oracle.lib()
    return s2vt_oracle


def _params(shape):
    orc = _oracle()
    D, V, H, Tv, Tc, B, K = shape
    d = orc.Dims(dim_image=D, n_words=V, word_dim=0, lstm_dim=H, n_video_lstm_step=Tv, n_caption_lstm_step=Tc, label_dim=0)
    p = orc.init_attention_params(d, 1234)
    p["embed_word_b"][0] = 3.0
    video = np.random.default_rng(7).standard_normal((B, Tv, D)).astype(np.float32)
    return d, p, video


def _model(shape, **kw):
    from s2vt_amd import attention as A
    D, V, H, Tv, Tc, B, K = shape
    d, p, video = _params(shape)
    m = A.Attention_Caption_Generator(D, V, H, B, Tv, Tc, 0.9, **kw)
    m.load(p)
    return d, p, m, video


def _ids(B, S, video_base=0, greedy=False):
    """(video_id, sample_id) of S sample blocks (+ a greedy block with sample id -1)."""
    vid = np.tile(np.arange(B, dtype=np.int32) + video_base, S + (1 if greedy else 0))
    sid = np.repeat(np.arange(S, dtype=np.int32), B)
    if greedy:
        sid = np.concatenate([sid, np.full(B, -1, np.int32)])
    return vid, sid


@functools.lru_cache(maxsize=None)
def _sampled_once(shape):
    _, _, m, video = _model(shape)
    s, g = m.sample(video, shape[6], True, seed=SEED)
    return s.cpu().numpy(), g.cpu().numpy()


def _sampled(shape):
    """(ids [K*B, Tc], greedy [B, Tc]) of sample() with seed 11 -- drawn once per shape and shared by the tests (each gets its own copy)."""
    s, g = _sampled_once(shape)
    return s.copy(), g.copy()


def _mask(ids):
    from s2vt_amd import hostglue
    return np.asarray(hostglue.masks_from_ids(np.asarray(ids)), np.float32)


def _assert_mask_exercised(mask):
    early = int((mask.sum(1) < mask.shape[1]).sum())
    assert early * 4 >= mask.shape[0], f"only {early} of {mask.shape[0]} rows end early"
    assert 0 < mask.sum() < mask.size and (mask[:, 0] == 1).all()


# ---------------------------------------------------------------------------------------------------------------- 1. sampler
@pytest.mark.parametrize("shape", SHAPES)
def test_sampler_ids_bit_exact_vs_oracle(gpu, oracle, shape):
    D, V, H, Tv, Tc, B, K = shape
    d, p, m, video = _model(shape)
    s, g = _sampled(shape)
    assert s.shape == (K * B, Tc) and g.shape == (B, Tc) and s.dtype == np.int32
    _assert_mask_exercised(_mask(s))
    rows = np.concatenate([s, g])
    logits, _, _ = oracle.attention_forward(p, d, np.tile(video, (K + 1, 1, 1)), rows, None, 1.0)
    vid, sid = _ids(B, K, 0, greedy=True)
    for t in range(Tc):       # by induction over t: the ids up to t-1 are the oracle's, so the logits of step t are, so the pick is
        assert np.array_equal(oracle.pick_tokens(np.ascontiguousarray(logits[:, t]), vid, sid, t, SEED), rows[:, t]), t
    # the greedy block is the greedy decoder, K = 0 is the greedy decoder, and the C entry point with K = 0 gives its ids
    ids0, _ = gpu.attn_decode_greedy(m.dims, m.store.params, m._dev(video, __import__("torch").float32))
    none, g0 = m.sample(video, 0, True)
    assert none is None and np.array_equal(g0.cpu().numpy(), ids0.cpu().numpy()) and np.array_equal(g, ids0.cpu().numpy())
    nk, gk = gpu.attn_sample(m.dims, m.store.params, m._dev(video, __import__("torch").float32), 0, SEED, 0, True)
    assert nk is None and np.array_equal(gk.cpu().numpy(), ids0.cpu().numpy())
    s_only, no_g = m.sample(video, K, False, seed=SEED)
    assert no_g is None and np.array_equal(s_only.cpu().numpy(), s)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]])
def test_sampler_noise_counters_use_the_global_video_index(gpu, shape):
    """Two parts of the batch sampled with their own video_base equal the whole batch: what data parallelism relies on."""
    D, V, H, Tv, Tc, B, K = shape
    _, _, m, video = _model(shape)
    s, g = _sampled(shape)
    h = B // 2
    for lo, hi in ((0, h), (h, B)):
        sp, gp = m.sample(video[lo:hi], K, True, seed=SEED, video_base=lo)
        assert np.array_equal(gp.cpu().numpy(), g[lo:hi])
        assert np.array_equal(sp.cpu().numpy().reshape(K, hi - lo, Tc), s.reshape(K, B, Tc)[:, lo:hi])


# ---------------------------------------------------------------------------------------------------------------- 2. forward
@pytest.mark.parametrize("keep,steps", [(1.0, None), (0.9, None), (0.9, 2)])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_on_shared_blocks_bit_exact(gpu, oracle, shape, keep, steps):
    import torch
    D, V, H, Tv, Tc, B, K = shape
    d, p, m, video = _model(shape)
    cap, _ = _sampled(shape)
    N, seed = K * B, 321
    T = Tc if steps is None else steps
    vid, sid = _ids(B, K)
    tiled = np.ascontiguousarray(np.tile(video, (K, 1, 1)))
    drop = None if keep >= 1.0 else [oracle.dropout_mask(seed, vid, sid, 768 + t, keep, H) for t in range(Tc)]
    ref_l, ref_a, _ = oracle.attention_forward(p, d, tiled, cap, drop, keep)
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dt)
    capd, vd, sd = dev(cap, torch.int32), dev(vid, torch.int32), dev(sid, torch.int32)
    lg, al, _ = gpu.attn_teacher_forced_fwd_rows(m.dims, m.store.params, dev(video, torch.float32), capd, keep, seed, vd, sd, steps=steps, want_alphas=True)
    lg2, al2, _ = gpu.attn_teacher_forced_fwd(m.dims, m.store.params, dev(tiled, torch.float32), capd, keep, seed, vd, sd, steps=steps, want_alphas=True)
    assert lg.shape == (T * N, V) and al.shape == (T, Tv, N)
    assert torch.equal(lg, lg2) and torch.equal(al, al2)
    assert np.array_equal(al.cpu().numpy(), ref_a[:T])
    assert np.array_equal(lg.view(T, N, V).transpose(0, 1).cpu().numpy(), ref_l[:, :T])


# ---------------------------------------------------------------------------------------------------------------- 3. update
def _reference(p, video, cap, mask, r, b, S, seed, keep, beta, mm, H):
    """float64 autograd of (-sum lp mask (r - b) + sum beta max(0, m - sum(alpha[t, 0:8, n])) mask) / sum(mask) on the tiled video."""
    import torch
    from oracle import s2vt_torch as T
    orc = _oracle()
    B, Tc = video.shape[0], cap.shape[1]
    vid, sid = _ids(B, S)
    drop = [orc.dropout_mask(seed, vid, sid, 768 + t, keep, H) for t in range(Tc)]
    pt = T.to_torch(p, torch.float64, True)
    logits, alphas = T.attention_teacher_forced(pt, torch.as_tensor(np.tile(video, (S, 1, 1))).double(), cap, drop, keep)
    mk = torch.as_tensor(mask).double()
    sums = alphas[:, :8, :].sum(1)                                                       # [Tc, N]
    hinge = beta * (torch.clamp(mm - sums, min=0.0).transpose(0, 1) * mk).sum() / mk.sum()
    loss = T.pg_loss(logits, cap, mask, torch.as_tensor(r).double(), torch.as_tensor(b).double()) + hinge
    loss.backward()
    live = sums.detach().numpy().T[mask > 0]
    return float(loss.detach()), {k: v.grad.numpy() for k, v in pt.items()}, live, float(hinge.detach())


def _check_grads(m, ref_g, tol=2e-4):
    line = []
    for k in m.store.names:
        ref = ref_g[k].reshape(m.store.shapes[k])
        got = m.store.g[k].cpu().numpy().astype(np.float64)
        err, bound = np.abs(got - ref).max(), tol * np.abs(ref).max()
        line.append(f"{k} {err:.1e}/{bound:.1e}")
        assert err <= bound, (k, err, bound)
    return ", ".join(line)


CASES = [  # shape index, margin m, hinge open?, explicit host mask + short active_steps?
    (0, 0.5, False, False), (1, 0.9, True, False), (2, 0.5, True, False), (3, 0.5, False, False), (1, 0.9, True, True)]


@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("si,mm,open_,host_mask", CASES)
def test_update_loss_and_gradients_vs_float64_autograd(gpu, si, mm, open_, host_mask, share):
    shape = SHAPES[si]
    D, V, H, Tv, Tc, B, K = shape
    d, p, m, video = _model(shape, m=mm)
    cap, _ = _sampled(shape)
    N, keep = K * B, 0.9
    rng = np.random.default_rng(100 + si)
    r = rng.uniform(-1, 1, N).astype(np.float32); b = rng.uniform(-1, 1, N).astype(np.float32)
    mask = _mask(cap)
    _assert_mask_exercised(mask)
    steps = None
    if host_mask:                            # a mask of the caller's own, cut one step short of the longest sample
        steps = int(mask.sum(1).max()) - 1
        assert 1 <= steps < Tc
        mask = mask.copy(); mask[:, steps:] = 0
    ref_loss, ref_g, sums, ref_hinge = _reference(p, video, cap, mask, r, b, K, m.dropout_seed, keep, m.beta, mm, H)
    if open_:
        assert (sums < mm - 0.1).all() and ref_hinge > 0, (sums.min(), sums.max())     # far from the kink: fp32 and float64 agree on the side
    else:
        assert Tv <= 8 and ref_hinge == 0.0
    st = m.reinforce_update(video, cap, mask if host_mask else None, r, b, lr=0.0, keep=keep, share_image_blocks=share,
                            active_steps=steps if host_mask else "auto")
    if not host_mask:
        assert np.array_equal(st.mask.cpu().numpy(), mask)                               # the device-derived mask
    got = float(st.loss)
    line = _check_grads(m, ref_g)
    print(f"\nreinforce_update {shape} m={mm} share={share} host_mask={host_mask}: loss {got:.7f} ref {ref_loss:.7f} (hinge part {ref_hinge:.5f}, "
          f"first-8 sums {sums.min():.3f}-{sums.max():.3f}); max err / bound: {line}")
    assert abs(got - ref_loss) <= 1e-3 * max(1.0, abs(ref_loss))
    assert abs(float(st.mask_sum) - mask.sum()) == 0
    gn = sum(float((g ** 2).sum()) for g in ref_g.values())
    assert abs(float(st.grad_sumsq) - gn) <= 1e-3 * gn


# ---------------------------------------------------------------------------------------------------------------- 4. one step
@pytest.mark.parametrize("si", [1, 3])
def test_one_step_end_to_end_clip_adam_counters(gpu, si):
    import torch
    from oracle import s2vt_torch as T
    shape = SHAPES[si]
    D, V, H, Tv, Tc, B, K = shape
    d, p, m, video = _model(shape, m=0.9)
    cap, _ = _sampled(shape)
    N, lr, clip = K * B, 1e-4, 5.0
    rng = np.random.default_rng(200 + si)
    r = rng.uniform(-1, 1, N).astype(np.float32); b = rng.uniform(-1, 1, N).astype(np.float32)
    mask = _mask(cap)
    called = []

    def reward_fn():
        called.append(1)
        return r, b
    _, ref_g, _, _ = _reference(p, video, cap, mask, r, b, K, m.dropout_seed, 0.9, m.beta, m.m, H)
    st = m.reinforce_update(video, cap, None, None, None, lr=lr, clip_norm=clip, reward_fn=reward_fn)
    assert called == [1] and np.isfinite(float(st.loss))
    assert m.global_step == 1 and m.adam_t == 1
    g64 = {k: torch.as_tensor(ref_g[k].reshape(m.store.shapes[k])) for k in m.store.names}
    g, norm = T.clip_by_global_norm(g64, clip)
    assert abs(float(st.grad_sumsq) - norm ** 2) <= 1e-3 * norm ** 2
    th = {k: torch.as_tensor(np.asarray(p[k], np.float64).reshape(m.store.shapes[k])) for k in m.store.names}
    zeros = lambda: {k: torch.zeros_like(v) for k, v in th.items()}
    th, _, _ = T.adam_tf(th, g, zeros(), zeros(), 1, lr)
    worst = 0.0
    for k in m.store.names:
        err = float(np.abs(m.store.p[k].cpu().numpy() - th[k].numpy()).max())
        worst = max(worst, err)
        assert err <= 2e-3 * lr + 1e-7, (k, err)
    print(f"\none step {shape}: worst variable error after clip + Adam {worst:.2e} (bound {2e-3 * lr + 1e-7:.2e})")
    before = {k: m.store.p[k].clone() for k in m.store.names}
    st2 = m.reinforce_update(video, cap, None, None, None, lr=lr, clip_norm=clip, reward_fn=reward_fn)
    assert m.global_step == 2 and m.adam_t == 2 and np.isfinite(float(st2.loss)) and len(called) == 2
    assert any(not torch.equal(before[k], m.store.p[k]) for k in m.store.names)
    assert int(m._applied.item()) == 2
    m.check_health()
    assert gpu.chain_timeouts() == 0


# ---------------------------------------------------------------------------------------------------------------- 5. class surface
def test_class_surface_sampler_loss_and_train_op(gpu, oracle):
    import torch
    from s2vt_amd import attention as A
    shape = SHAPES[1]
    D, V, H, Tv, Tc, B, K = shape
    d, p, m, video = _model(shape, m=0.9, multisample=K)
    sess = A.Session(m)
    feats = [video[j].tolist() for j in range(B)]
    # build_multinomial_sampler: a fresh stream per run, a function of (seed, run count)
    sampled_captions, sampler_video = m.build_multinomial_sampler()
    a1 = sess.run(sampled_captions, {sampler_video: feats})
    a2 = sess.run(sampled_captions, {sampler_video: feats})
    assert a1.shape == (B, Tc) and a1.dtype == np.int64 and not np.array_equal(a1, a2)
    _, _, m2, _ = _model(shape, m=0.9, multisample=K)
    sc2, sv2 = m2.build_multinomial_sampler()
    assert np.array_equal(A.Session(m2).run(sc2, {sv2: feats}), a1)
    ref, _ = m.sample(video, 1, False, seed=m.sample_seed + 7919)
    assert np.array_equal(ref.cpu().numpy(), a1)
    # build_loss: lp * mask, fed the K-times tiled block as the reference feeds it (:779-782)
    cap, _ = _sampled(shape)
    mask = _mask(cap)
    N = K * B
    tiled = np.tile(video, (K, 1, 1))
    loss, lv, lc, lm = m.build_loss()
    got = sess.run(loss, {lv: tiled, lc: cap, lm: mask})
    vid, sid = _ids(B, K)
    drop = [oracle.dropout_mask(m.dropout_seed, vid, sid, 768 + t, 0.9, H) for t in range(Tc)]
    ref_l, _, _ = oracle.attention_forward(p, d, np.ascontiguousarray(tiled), cap, drop, 0.9)
    lp = np.stack([oracle.row_losses(np.ascontiguousarray(ref_l[:, t]), cap[:, t], 0.0)[1] for t in range(Tc)], 1)
    assert got.shape == (N, Tc) and np.abs(got - lp * mask).max() <= 1e-5
    assert np.abs(got[mask == 0]).max() == 0 and (got[mask > 0] < 0).all()
    # reinforce_train_op through Session.run is reinforce_update
    rng = np.random.default_rng(5)
    r = rng.uniform(-1, 1, N).astype(np.float32); b = rng.uniform(-1, 1, N).astype(np.float32)
    rewards, base_line = m.placeholder("rewards"), m.placeholder("base_line")
    learning_rate = m.exponential_decay(1e-4, 1000, 0.5)
    train_op, sum_loss = m.reinforce_train_op((loss, lv, lc, lm), rewards, base_line, learning_rate, clip_norm=5)
    _, loss_val = sess.run([train_op, sum_loss], {lv: tiled, lc: cap, lm: mask, rewards: r, base_line: b})
    st = m2.reinforce_update(video, cap, mask, r, b, lr=1e-4, clip_norm=5.0)
    assert m.global_step == 1 and m2.global_step == 1
    assert abs(loss_val - float(st.loss)) <= 1e-6 * max(1.0, abs(loss_val))
    for k in m.store.names:
        assert float((m.store.p[k] - m2.store.p[k]).abs().max()) <= 2e-3 * 1e-4 + 1e-7, k
    assert not torch.equal(m.store.p["embed_word_W"], torch.as_tensor(p["embed_word_W"]).cuda())


# ---------------------------------------------------------------------------------------------------------------- 6. driver
def test_driver_reinforce_three_steps_and_checkpoint(gpu, tmp_path):
    import torch
    from s2vt_amd import train_attention, train_common as tc
    from test_gpu_train_drivers import _corpus
    rng = np.random.default_rng(0)
    sents, feats, vocab = _corpus(tmp_path, "attrl", rng, n_videos=8)
    corpus = tc.Corpus(sents, feats, vocabulary=vocab)
    cfg = train_attention.reinforce_config(dim_image=24, lstm_dim=32, n_video_lstm_step=3, n_caption_lstm_step=8, n_epochs=1, batch_size=4,
                                           max_steps_per_epoch=3, start_learning_rate=1e-3, model_path=str(tmp_path / "m"), model_name="attrl",
                                           step_log=str(tmp_path / "attrl.jsonl"))
    from s2vt_amd import attention as A, hostglue
    wordtoix, _ = hostglue.preProBuildWordVocab(corpus.vocabulary)
    fresh = A.Attention_Caption_Generator(24, len(wordtoix), 32, 4, 3, 8, 0.9, seed=cfg.seed)
    start = {k: fresh.store.p[k].clone() for k in fresh.store.names}
    model, hist = train_attention.train(cfg, corpus, corpus, log=lambda *_: None, reinforce=True, samples=2)
    assert model.global_step == 3 and np.isfinite(hist[-1]["loss"]) and hist[-1]["ciderD"] is not None
    assert any(not torch.equal(start[k], model.store.p[k]) for k in model.store.names)
    import json
    steps = [json.loads(l) for l in open(tmp_path / "attrl.jsonl") if '"step"' in l and '"kind": "step"' in l]
    assert len(steps) == 3 and all(np.isfinite(s["loss"]) and "reward" in s and "baseline" in s for s in steps)
    cfg1 = train_attention.reinforce_config(dim_image=24, lstm_dim=32, n_video_lstm_step=3, n_caption_lstm_step=8, n_epochs=1, batch_size=4,
                                            max_steps_per_epoch=1, model_path=str(tmp_path / "m2"), model_name="attrl2")
    model2, _ = train_attention.train(cfg1, corpus, None, log=lambda *_: None, reinforce=True, samples=2, resume=hist[-1]["checkpoint"])
    assert model2.global_step == 4 and model2.adam_t == 4
