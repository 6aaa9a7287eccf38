"""The mixed sampler (s2vt_sample_mix, ops.sample_mix, Video_Caption_Generator.mix_sample): build_mix_sample of
reinforce_multitask_e2e_attribute_by_groudtruth_greedy_s2vt.py:512-599 -- a greedy decode whose fed word at step t >= 1 is the ground-truth
word with probability p_gt and the row's own argmax otherwise -- decoded beside build_sampler's greedy rows from one encode.

The oracle of the mixed decode is written here from oracle.s2vt_oracle's pieces (frame_embed, encode, lstm1_step, lstm2_step, xw_plus_b,
pick_tokens with sample id -1, philox4x32_10 for the coin).  Ground-truth captions are random ids in [2, V): they differ from the argmax of
a randomly initialised model almost everywhere, and every parity case first asserts ON THE ORACLE that both coin outcomes occur and that a
ground-truth word different from the row's own pick was fed -- otherwise ids equal to the oracle's would not show that the mix is honoured."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIXS = 0x4D495853

SHAPES = {
    "small-odd": (dict(dim_image=64, n_words=131, word_dim=24, lstm_dim=32, n_video_lstm_step=3, n_caption_lstm_step=9), 5),
    "one-tile": (dict(dim_image=128, n_words=260, word_dim=32, lstm_dim=64, n_video_lstm_step=5, n_caption_lstm_step=12), 16),
    # R = 32 <= 64, B % 16 == 0, H >= 132: the plain sampler takes the persistent decode loop and the workspace holds its fragment-order
    # operands; the mixed mode runs the per-step launches beside them
    "persistent-range": (dict(dim_image=256, n_words=2000, word_dim=300, lstm_dim=992, n_video_lstm_step=5, n_caption_lstm_step=8), 16),
    # R = 300: two workgroups of the word-select kernel, a ragged last row tile
    "many-rows": (dict(dim_image=96, n_words=300, word_dim=20, lstm_dim=48, n_video_lstm_step=2, n_caption_lstm_step=7), 150),
}
_cache = {}


def _case(oracle, name):
    """(model, device video, oracle params, oracle dims, ground truth [B, Tc], the encoder state + LSTM1's decode trajectory, the plain
    sampler's greedy ids) of a shape: built once, shared by the tests, never written to."""
    if name not in _cache:
        import torch
        from s2vt_amd import model as M
        dims, B = SHAPES[name]
        mdl = M.Video_Caption_Generator(dims["dim_image"], dims["n_words"], dims["word_dim"], dims["lstm_dim"], B, 0, dims["n_video_lstm_step"],
                                        dims["n_caption_lstm_step"], seed=3, multisample=1)
        rng = np.random.default_rng(1)
        video = np.abs(rng.standard_normal((B, dims["n_video_lstm_step"], dims["dim_image"])) * 0.5).astype(np.float32)
        gt = rng.integers(2, dims["n_words"], (B, dims["n_caption_lstm_step"])).astype(np.int32)
        p = {n: mdl.store.p[n].cpu().numpy() for n in mdl.store.names}
        d = oracle.Dims(label_dim=0, **dims)
        dev_video = torch.as_tensor(video).cuda()
        greedy = mdl.sample(dev_video, 0, True)[1].cpu().numpy()
        _cache[name] = (mdl, dev_video, p, d, gt, _encode(oracle, p, d, video), greedy)
    return _cache[name]


def _encode(oracle, p, d, video):
    """What does not depend on a fed word: the encoder's LSTM2 state and LSTM1's outputs over the decode steps (it sees padding only)."""
    c1, h1, c2, h2 = oracle.encode(p, oracle.frame_embed(p, video))
    out1 = []
    for _ in range(d.n_caption_lstm_step):
        c1, h1, o1, _, _ = oracle.lstm1_step(p, None, c1, h1)
        out1.append(o1)
    return out1, c2, h2


def _coin(oracle, seed, video, step, p_gt):
    """include/s2vt.h: u = ((x >> 9) + 0.5) * 2^-23 of word x of Philox(counter (0, video, 0, step), key (seed_lo, seed_hi ^ 'MIXS')); ground
    truth iff u < p_gt, compared in fp32 (u is exactly representable)."""
    x = oracle.philox4x32_10([0, video, 0, step], [seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ MIXS])[0]
    u = np.float32((int(x) >> 9) * 2.0 ** -23 + 2.0 ** -24)
    return bool(u < np.float32(p_gt))


def _mix_decode(oracle, p, d, enc, gt, p_gt, seed, video_base=0, with_greedy=True):
    """-> (mixed ids [B, Tc], greedy ids [B, Tc] | None, coin [B, Tc] (step 0 unused), fed-a-different-word [B, Tc])"""
    out1, c2, h2 = enc
    B, Tc = gt.shape
    nb = 2 if with_greedy else 1
    c2, h2 = np.tile(c2, (nb, 1)), np.tile(h2, (nb, 1))
    vid = np.tile(np.arange(B, dtype=np.int32) + video_base, nb)
    sid = np.full(nb * B, -1, np.int32)                               # every row picks by argmax
    tok = np.ones(nb * B, np.int32)                                   # <bos>
    ids = np.empty((nb * B, Tc), np.int32)
    coin = np.zeros((B, Tc), bool); differs = np.zeros((B, Tc), bool)
    for t in range(Tc):
        fed = tok.copy()
        for b in range(B if t else 0):
            if _coin(oracle, seed, video_base + b, t, p_gt):
                coin[b, t] = True
                differs[b, t] = gt[b, t - 1] != tok[b]
                fed[b] = gt[b, t - 1]
        c2, h2, o2, _, _ = oracle.lstm2_step(p, np.tile(out1[t], (nb, 1)), fed, c2, h2)
        tok = oracle.pick_tokens(oracle.xw_plus_b(o2, p["embed_word_W"], p["embed_word_b"]), vid, sid, t, seed)
        ids[:, t] = tok
    return ids[:B], (ids[B:] if with_greedy else None), coin, differs


def _assert_mix_is_visible(coin, differs):
    assert coin[:, 1:].any() and not coin[:, 1:].all()               # both coin outcomes occur ...
    assert differs.any()                                              # ... and a ground-truth word replaced a different pick


@pytest.mark.parametrize("prob", [0.9, 0.5])
@pytest.mark.parametrize("name", list(SHAPES))
def test_mixed_ids_equal_the_oracle(gpu, oracle, name, prob):
    mdl, video, p, d, gt, enc, greedy = _case(oracle, name)
    p_gt = np.float32(np.float64(prob) / np.float64(1.00001))
    for seed in (11, (5 << 32) | 12):
        ref_m, ref_g, coin, differs = _mix_decode(oracle, p, d, enc, gt, p_gt, seed)
        _assert_mix_is_visible(coin, differs)
        m, g = mdl.mix_sample(video, gt, prob, True, seed=seed)
        assert m.dtype == g.dtype and tuple(m.shape) == tuple(g.shape) == gt.shape
        assert np.array_equal(m.cpu().numpy(), ref_m)
        assert np.array_equal(g.cpu().numpy(), ref_g)
        assert np.array_equal(g.cpu().numpy(), greedy)                # block 1 = model.sample(video, 0, True)'s greedy ids
        assert not np.array_equal(ref_m, ref_g)
    assert gpu.chain_timeouts() == 0


def test_mixed_ids_without_the_greedy_block(gpu, oracle):
    mdl, video, p, d, gt, enc, _ = _case(oracle, "one-tile")
    ref_m, none, coin, differs = _mix_decode(oracle, p, d, enc, gt, np.float32(0.9 / 1.00001), 21, with_greedy=False)
    _assert_mix_is_visible(coin, differs)
    m, g = mdl.mix_sample(video, gt, 0.9, False, seed=21)
    assert g is None and none is None and np.array_equal(m.cpu().numpy(), ref_m)
    assert gpu.chain_timeouts() == 0


@pytest.mark.parametrize("name", ["small-odd", "persistent-range", "many-rows"])
def test_ends_of_the_range(gpu, oracle, name):
    import torch
    mdl, video, p, d, gt, enc, greedy = _case(oracle, name)
    cap = torch.as_tensor(gt).cuda()
    # p_gt = 0: never the ground truth -- the mixed block is the greedy decode
    m0, g0 = gpu.sample_mix(mdl.dims, mdl.store.params, video, cap, 0.0, seed=4)
    assert np.array_equal(m0.cpu().numpy(), greedy) and np.array_equal(g0.cpu().numpy(), greedy)
    # p_gt = 1: always the ground truth -- the mixed block is the argmax (first maximum) of the teacher-forced logits without dropout
    m1, g1 = gpu.sample_mix(mdl.dims, mdl.store.params, video, cap, 1.0, seed=4)
    logits = oracle.teacher_forced(p, d, video.cpu().numpy(), gt)      # [B, Tc, V], keep = 1
    assert np.array_equal(m1.cpu().numpy(), logits.argmax(-1).astype(np.int32))
    assert np.array_equal(g1.cpu().numpy(), greedy)
    assert not np.array_equal(m1.cpu().numpy(), greedy)
    assert gpu.chain_timeouts() == 0


def test_sharded_batch_draws_the_same_coins(gpu, oracle):
    import torch
    from s2vt_amd import model as M
    dims = SHAPES["one-tile"][0]
    mdl = M.Video_Caption_Generator(dims["dim_image"], dims["n_words"], dims["word_dim"], dims["lstm_dim"], 8, 0, dims["n_video_lstm_step"],
                                    dims["n_caption_lstm_step"], seed=3, multisample=1)
    rng = np.random.default_rng(5)
    video = torch.as_tensor(np.abs(rng.standard_normal((8, dims["n_video_lstm_step"], dims["dim_image"])) * 0.5).astype(np.float32)).cuda()
    gt = rng.integers(2, dims["n_words"], (8, dims["n_caption_lstm_step"])).astype(np.int32)
    m, g = (x.cpu().numpy() for x in mdl.mix_sample(video, gt, 0.5, True, seed=33, video_base=0))
    halves = [[x.cpu().numpy() for x in mdl.mix_sample(video[lo:lo + 4].contiguous(), gt[lo:lo + 4], 0.5, True, seed=33, video_base=lo)] for lo in (0, 4)]
    assert np.array_equal(m, np.concatenate([halves[0][0], halves[1][0]]))
    assert np.array_equal(g, np.concatenate([halves[0][1], halves[1][1]]))
    assert not np.array_equal(m, g)                                    # (the mix took effect)
    # the coins follow the global video id: the second half decoded as videos 0..3 is fed other words
    other = mdl.mix_sample(video[4:].contiguous(), gt[4:], 0.5, False, seed=33, video_base=0)[0].cpu().numpy()
    assert not np.array_equal(other, halves[1][0])
    assert gpu.chain_timeouts() == 0


def test_mixed_call_leaves_the_sampler_state_alone(gpu, oracle):
    """sample -> mix_sample -> reinforce_update(reuse_sampler_state=True) on the first call's samples: the same update, bit for bit, as
    without the mixed call in between (a workspace of its own, ops.sample.last_state untouched).
    The shape is chosen so that the update itself is reproducible bit for bit, or array_equal could not tell the mixed call from run-to-run
    noise: the one order-dependent sum of the backward is the atomic scatter of the word-embedding gradient, where the rows of a word fed
    several times are added in the order the hardware gives (at B = 8, K = 3 two runs of the SAME update differ in 10 - 20 elements of
    theta by ~1e-8, all in Wemb, with or without the mixed call).  A sum of at most two terms does not depend on its order (fp32 addition
    is commutative), so with two rows -- <bos> is fed twice -- and no sampled word fed more than twice (asserted) every element of the
    update is order-free."""
    import torch
    from s2vt_amd import model as M
    B, K, Tc = 2, 1, 10
    mk = lambda: M.Video_Caption_Generator(128, 260, 32, 64, B, 0, 5, Tc, seed=5, multisample=K, dropout_rate=0.9)
    a, b = mk(), mk()
    rng = np.random.default_rng(2)
    video = torch.as_tensor(np.abs(rng.standard_normal((B, 5, 128)) * 0.5).astype(np.float32)).cuda()
    gt = rng.integers(2, 260, (B, Tc)).astype(np.int32)
    r = (rng.random(K * B) * 2).astype(np.float32); bl = np.tile((rng.random(B) * 2).astype(np.float32), K)
    sa, _ = a.sample(video, K, True, seed=9)
    fed = np.concatenate([np.ones(K * B, np.int64), sa.cpu().numpy()[:, :-1].ravel()])
    assert np.bincount(fed).max() <= 2                                 # no word's embedding gradient is a sum of three terms
    state = gpu.sample.last_state
    mix, greedy = a.mix_sample(video, gt, 0.9, True, seed=9)
    assert gpu.sample.last_state is state
    assert not torch.equal(mix, greedy)                                # (the mixed call did run its own decode)
    a.reinforce_update(video, sa, None, r, bl, lr=1e-2, reuse_sampler_state=True)
    sb, _ = b.sample(video, K, True, seed=9)
    b.reinforce_update(video, sb, None, r, bl, lr=1e-2, reuse_sampler_state=True)
    assert torch.equal(sa, sb)
    print("theta max |a - b| =", float((a.store.theta - b.store.theta).abs().max()))
    assert np.array_equal(a.store.theta.cpu().numpy(), b.store.theta.cpu().numpy())
    assert float((a.store.theta - mk().store.theta).abs().max()) > 0  # (and the update moved the variables)
    assert gpu.chain_timeouts() == 0


def test_caption_ids_are_clamped_on_the_device_and_checked_on_the_host(gpu, oracle):
    import torch
    mdl, video, p, d, gt, enc, greedy = _case(oracle, "small-odd")
    V = d.n_words
    bad = gt.copy(); bad[0, 0] = -3; bad[2, 3] = V + 7; bad[4, 1] = -3; bad[1, 5] = V + 7
    clamped = np.clip(bad, 0, V - 1)
    assert (clamped != gt).sum() == 4
    for prob in (1.00001, 0.9):                                        # (p_gt = 1: every one of the four entries is fed)
        got = mdl.mix_sample(video, torch.as_tensor(bad).cuda(), prob, True, seed=8)
        want = mdl.mix_sample(video, torch.as_tensor(clamped).cuda(), prob, True, seed=8)
        for x, y in zip(got, want):
            x = x.cpu().numpy()
            assert np.array_equal(x, y.cpu().numpy()) and x.min() >= 0 and x.max() < V
    fed_all = mdl.mix_sample(video, torch.as_tensor(clamped).cuda(), 1.00001, False, seed=8)[0].cpu().numpy()
    assert not np.array_equal(fed_all, mdl.mix_sample(video, gt, 1.00001, False, seed=8)[0].cpu().numpy())    # the clamped words were read
    with pytest.raises(ValueError):
        mdl.mix_sample(video, bad, 0.9)
    with pytest.raises(ValueError):
        mdl.mix_sample(video, bad.tolist(), 0.9)
    with pytest.raises(ValueError):
        mdl.mix_sample(video, gt[:, :-1], 0.9)
    assert gpu.chain_timeouts() == 0
