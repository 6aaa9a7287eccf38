"""Shapes, parameters and a CPU restatement of the scheduled-sampling unroll (generate_words_tf_s2vt.py:101-211; s2vt_scheduled_fwd,
ops.scheduled_fwd, Video_Caption_Generator.scheduled_update), shared by the scheduled-sampling tests.

The restatement is written from oracle.s2vt_oracle's pieces (frame_embed, encode, lstm1_step, lstm2_step, dropout_masks, xw_plus_b,
pick_tokens with sample id -1, philox4x32_10 for the coin), the way tests/test_gpu_sample_mix.py::_mix_decode restates the mixed decode.

A randomly initialised model almost never picks <eos> = 0, and then the running mask of quirk SQ1 never moves.  Every case therefore adds
BIAS[name] to embed_word_b[0].  The values were chosen on the CPU oracle (nothing here needs a GPU) so that, for every p_gt, seed and
keep the tests use, assert_visible() holds: both coin outcomes occur, a ground-truth word different from the row's own pick was fed, a
row's mask falls to 0 before the last step, a row is still unmasked at the last step, and sum(mask) > 0.  A case that does not meet them
would pass with the feature half built, so every parity test asserts them first."""
import numpy as np

MIXS = 0x4D495853

SHAPES = {
    # ragged tiles everywhere
    "small-odd": (dict(dim_image=64, n_words=131, word_dim=24, lstm_dim=32, n_video_lstm_step=3, n_caption_lstm_step=9), 5),
    "one-tile": (dict(dim_image=128, n_words=260, word_dim=32, lstm_dim=64, n_video_lstm_step=5, n_caption_lstm_step=12), 16),
    # B = 16, H = 992: LSTM1 and LSTM2's encode stage take their persistent form and hand the last history slot to the per-step launches
    "chain-range": (dict(dim_image=256, n_words=2000, word_dim=300, lstm_dim=992, n_video_lstm_step=5, n_caption_lstm_step=8), 16),
    # several workgroups of the per-step kernel, a ragged last row tile
    "many-rows": (dict(dim_image=96, n_words=300, word_dim=20, lstm_dim=48, n_video_lstm_step=2, n_caption_lstm_step=7), 150),
    # Tc = 1: no fed word is ever chosen
    "one-step": (dict(dim_image=64, n_words=131, word_dim=24, lstm_dim=32, n_video_lstm_step=3, n_caption_lstm_step=1), 5),
}
# added to embed_word_b[0]; each from the middle of the range a scan on the CPU oracle found (see the module docstring), checked by test_scheduled_cases_cpu.py
BIAS = {"small-odd": 0.014, "one-tile": 0.0225, "chain-range": 0.184, "many-rows": 0.0125, "one-step": 0.0195}
PROBS = (0.5, 0.9)                                    # true_word_prob; p_gt = prob / 1.00001 (generate_words_tf_s2vt.py:136-139)
SEEDS = (11, (5 << 32) | 12)                          # coin seeds, one with non-zero high 32 bits
KEEPS = (1.0, 0.9)
DROP_SEED = 77
PARAM_SEED = 3

_cache = {}


def p_gt_of(prob):
    return np.float32(np.float64(prob) / np.float64(1.00001))


def case(oracle, name):
    """(oracle params with the bias applied, oracle dims, video [B, Tv, D], ground truth [B, Tc] in [2, V), video ids, sample ids): built
    once on the CPU, shared, never written to.  The parameters are init_reference's (what Video_Caption_Generator(seed=PARAM_SEED) holds)."""
    if name not in _cache:
        from s2vt_amd import model as M
        dims, B = SHAPES[name]
        store = M.ParamStore(M.param_shapes(dims["dim_image"], dims["n_words"], dims["word_dim"], dims["lstm_dim"]), "cpu")
        M.init_reference(store, PARAM_SEED)
        p = {n: store.p[n].numpy().copy() for n in store.names}
        p["embed_word_b"][0] += np.float32(BIAS[name])
        rng = np.random.default_rng(1)
        video = np.abs(rng.standard_normal((B, dims["n_video_lstm_step"], dims["dim_image"])) * 0.5).astype(np.float32)
        gt = rng.integers(2, dims["n_words"], (B, dims["n_caption_lstm_step"])).astype(np.int32)
        vid = np.arange(B, dtype=np.int32)
        sid = np.zeros(B, np.int32)
        _cache[name] = (p, oracle.Dims(label_dim=0, **dims), video, gt, vid, sid)
    return _cache[name]


def coin(oracle, seed, video, sample, step, p_gt):
    """include/s2vt.h: u = ((x >> 9) + 0.5) * 2^-23 of word x of Philox(counter (0, video, sample, step), key (seed_lo, seed_hi ^ 'MIXS'));
    ground truth iff u < p_gt, compared in fp32 (u is exactly representable)."""
    x = oracle.philox4x32_10([0, video, sample, step], [seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ MIXS])[0]
    u = np.float32((int(x) >> 9) * 2.0 ** -23 + 2.0 ** -24)
    return bool(u < np.float32(p_gt))


def scheduled_unroll(oracle, p, d, video, gt, p_gt, coin_seed, vid, sid, keep=1.0, drop_seed=DROP_SEED, loss_weight=1.0):
    """The scheduled unroll on N = B rows (row n = video n).  Returns a dict: logits [Tc*N, V] time-major, generated / fed [N, Tc],
    mask [N, Tc], coef_tm / target_tm [Tc*N], mask_sum, coin [N, Tc] (column 0 unused), differs [N, Tc] (a ground-truth word other
    than the row's own pick was fed), drop (the dropout masks or None)."""
    N, Tc = gt.shape
    V, H, Tv = d.n_words, d.lstm_dim, d.n_video_lstm_step
    drop = oracle.dropout_masks(drop_seed, vid, sid, keep, H, Tv, Tc) if keep < 1.0 else None
    g = (lambda k: None) if drop is None else (lambda k: drop[k])
    c1, h1, c2, h2 = oracle.encode(p, oracle.frame_embed(p, video), g("enc1"), g("enc2"), keep)
    truth = np.clip(gt, 0, V - 1).astype(np.int32)
    argmax_sid = np.full(N, -1, np.int32)
    gen = np.empty((N, Tc), np.int32); fed = np.empty((N, Tc), np.int32); mask = np.empty((N, Tc), np.float32)
    flips = np.zeros((N, Tc), bool); differs = np.zeros((N, Tc), bool)
    logits = np.empty((Tc, N, V), np.float32)
    run = np.ones(N, np.float32)
    for t in range(Tc):
        if t == 0:
            fed[:, 0] = 1                                              # <bos> (:161-163); the coin of step 0 is drawn and unused
        else:
            for n in range(N):
                flips[n, t] = coin(oracle, coin_seed, int(vid[n]), int(sid[n]), t, p_gt)
                differs[n, t] = flips[n, t] and truth[n, t - 1] != gen[n, t - 1]
                fed[n, t] = truth[n, t - 1] if flips[n, t] else gen[n, t - 1]
        c1, h1, o1, _, _ = oracle.lstm1_step(p, None, c1, h1, None if drop is None else drop["dec1"][t], keep)
        c2, h2, o2, _, _ = oracle.lstm2_step(p, o1, fed[:, t].copy(), c2, h2, drop_mask=None if drop is None else drop["dec2"][t], keep=keep)
        logits[t] = oracle.xw_plus_b(o2, p["embed_word_W"], p["embed_word_b"])
        gen[:, t] = oracle.pick_tokens(logits[t], vid, argmax_sid, t, 0)
        run = run * (gen[:, t] != 0).astype(np.float32)               # SQ1 (:194-199): updated before it weighs the step
        mask[:, t] = run
    return dict(logits=logits.reshape(Tc * N, V), generated=gen, fed=fed, mask=mask,
                coef_tm=(np.float32(loss_weight) * mask.T).reshape(-1).astype(np.float32), target_tm=truth.T.reshape(-1).copy(),
                mask_sum=float(mask.sum()), coin=flips, differs=differs, drop=drop)


def visibility(r):
    """The conditions under which equality with the restatement shows that the coin, the fed word and the running mask are honoured.
    With Tc = 1 no word is chosen and no step lies before the last one: what remains is a masked row, an unmasked row and sum(mask) > 0."""
    mask, flips = r["mask"], r["coin"]
    Tc = mask.shape[1]
    out = {"unmasked at the last step": bool((mask[:, -1] == 1).any()), "sum(mask) > 0": r["mask_sum"] > 0}
    if Tc == 1:
        out["a masked row"] = bool((mask[:, 0] == 0).any())
        return out
    out["both coin outcomes"] = bool(flips[:, 1:].any() and not flips[:, 1:].all())
    out["a different ground-truth word was fed"] = bool(r["differs"].any())
    out["a mask falls to 0 before the last step"] = bool((mask[:, :-1] == 0).any())
    return out


def assert_visible(r):
    bad = [k for k, ok in visibility(r).items() if not ok]
    assert not bad, f"the case shows nothing: {bad}"
