"""Shapes, parameters and CPU restatements of the residual S2VT captioner (residual_tf_s2vt.py; S2VT_MODEL_RESIDUAL, s2vt_amd.residual),
shared by the residual tests.  At every decode step (build_model :149-151, build_generator :206-208, build_sampler :263-265)

    output2 = output1 + output2
    logit_words = xw_plus_b(output2, embed_word_W, embed_word_b)

and nothing else differs from tf_s2vt.py.  The fp32 restatements are written from oracle.s2vt_oracle's pieces (frame_embed, encode,
lstm1_step, lstm2_step, dropout_masks, xw_plus_b, pick_tokens) the way tests/scheduled_cases.py restates its unroll: s = fl32(o1 + o2), one
numpy float32 addition, o1 / o2 the DropoutWrapper outputs of the step, LSTM2's state the un-summed h'.  The float64 restatement for the
gradients is the loop of oracle.s2vt_torch.unroll with the same one line added (that function is monolithic).

Making the cases discriminate.  On a randomly initialised model the logits are small against the Gumbel noise, so the multinomial rows
of a plain and a residual decode mostly coincide and an implementation that ignored the model bit would pass.  Every case therefore
multiplies embed_word_W by SCALE.  Scan on the CPU oracle (oracle.init_params seed PARAM_SEED, K = 2, sampler seed 11; multinomial rows
that differ between the plain and the residual decode, of 2 B; every greedy row differs at every scale on all five shapes):

    scale      small-odd   one-tile   many-rows   chain-range   one-step
      1          0 / 10     4 / 32      9 / 300     12 / 32       0 / 10
      8          2 / 10    20 / 32     65 / 300     32 / 32       1 / 10
     16          4 / 10    23 / 32    107 / 300     32 / 32       1 / 10
     32          7 / 10    28 / 32    185 / 300     32 / 32       1 / 10
     64         10 / 10    32 / 32    244 / 300     32 / 32       2 / 10

(the second sampler seed at 32: 6, 32, 169, 32, 3).  SCALE = 32: the smallest scanned scale at which at least half of the multinomial
rows differ at one-tile and many-rows; at 64 chain-range's ids collapse to 44 distinct tokens (108 at 32).  With
model.init_reference(seed 3) in place of oracle.init_params one greedy row of many-rows (149 / 150) decodes alike at every scale, so
the cases take the oracle's initialiser.  test_residual_cases_cpu.py checks assert_visible() for every case, seed and K the GPU tests
use, so a change of either initialiser shows there first.

Stop-at-<eos> cases add EOS_BIAS to embed_word_b[0].  Scan (bias: rows of the 3 B whose first <eos> lies before the last step / rows that
never emit it): small-odd 1: 7 / 8, 2: 9 / 6, 4: 14 / 1, 6: 15 / 0;  one-tile 1: 9 / 38, 2: 25 / 22, 4: 44 / 2, 6: 48 / 0;  many-rows
1: 153 / 291, 2: 189 / 257, 4: 325 / 109, 6: 448 / 0;  odd-dims (EXTRA_SHAPES) 1: 10 / 11, 2: 13 / 8, 4: 19 / 1, 6: 21 / 0 (of 21).  EOS_BIAS = 2: both kinds of
row at every shape."""
import numpy as np

from scheduled_cases import SHAPES                   # noqa: F401  (the five shapes; re-exported)

SCALE = 32.0
PARAM_SEED = 3
SAMPLER_SEEDS = (11, (5 << 32) | 12)                  # one with non-zero high 32 bits
K_SAMPLES = 2
DROP_SEED = 77
EOS_BIAS = {"small-odd": 2.0, "one-tile": 2.0, "many-rows": 2.0, "odd-dims": 2.0}     # (module docstring)
# A shape of the stop-at-<eos> tests only: H and E are no multiples of 4, so every operand fails the vector path's alignment rules and the
# early-exit sampler's live-row launches take the SCALAR live-row form of the residual cell step (the five shapes above all take the vector one)
EXTRA_SHAPES = {"odd-dims": (dict(dim_image=64, n_words=131, word_dim=22, lstm_dim=30, n_video_lstm_step=3, n_caption_lstm_step=9), 7)}

_cache = {}


def case(oracle, name):
    """(params with embed_word_W scaled, oracle dims, video [B, Tv, D]): built once on the CPU, shared, never written to."""
    if name not in _cache:
        dims, B = SHAPES[name] if name in SHAPES else EXTRA_SHAPES[name]
        p = oracle.init_params(oracle.Dims(label_dim=0, **dims), seed=PARAM_SEED)
        p = {n: np.array(v, np.float32) for n, v in p.items()}
        p["embed_word_W"] *= np.float32(SCALE)
        rng = np.random.default_rng(1)
        video = np.abs(rng.standard_normal((B, dims["n_video_lstm_step"], dims["dim_image"])) * 0.5).astype(np.float32)
        _cache[name] = (p, oracle.Dims(label_dim=0, **dims), video)
    return _cache[name]


# (case, K, sampler seed, video_base) of the sampler parity tests.  chain-range at K = 2 is R = 48 rows with B % 16 == 0 and H >= 132: the
# window in which a plain model takes the persistent decode loop, which a residual model must not; many-rows at K = 2 is R = 450 > 384 and
# one-tile at K = 6 is R = 112 (96 < R <= 384): both families of cell-step tiles.
SAMPLE_CASES = [("small-odd", 2, SAMPLER_SEEDS[0], 0), ("small-odd", 2, SAMPLER_SEEDS[1], 1000), ("one-tile", 2, SAMPLER_SEEDS[0], 0),
                ("one-tile", 6, SAMPLER_SEEDS[1], 7), ("many-rows", 2, SAMPLER_SEEDS[0], 0), ("chain-range", 2, SAMPLER_SEEDS[0], 0),
                ("chain-range", 2, SAMPLER_SEEDS[1], 3), ("one-step", 2, SAMPLER_SEEDS[0], 0)]


def decodes(oracle, name, seed, K=K_SAMPLES, eos=False, video_base=0):
    """((ids, greedy) of the residual decode, (ids, greedy) of the plain one) for a case, computed once and shared."""
    key = ("decodes", name, seed, K, eos, video_base)
    if key not in _cache:
        p, d, video = case(oracle, name)
        if eos:
            p = with_eos_bias(p, name)
        _cache[key] = (residual_sample(oracle, p, d, video, K, seed, video_base), residual_sample(oracle, p, d, video, K, seed, video_base, residual=False))
    return _cache[key]


def first_eos(ids):
    """Per row: the index of the first <eos> = 0, or Tc when the row never emits it."""
    Tc = ids.shape[1]
    return np.array([np.where(r == 0)[0][0] if (r == 0).any() else Tc for r in ids])


def with_eos_bias(p, name):
    q = dict(p)
    q["embed_word_b"] = p["embed_word_b"].copy()
    q["embed_word_b"][0] += np.float32(EOS_BIAS[name])
    return q


def _sum(o1, o2, residual):
    return (o1.astype(np.float32) + o2.astype(np.float32)).astype(np.float32) if residual else o2


def residual_sample(oracle, p, d, video, K, seed, video_base=0, with_greedy=True, return_logits=False, residual=True):
    """oracle.sample_captions with the residual sum: K multinomial row blocks + one greedy block from ONE encode, rows sample-major.
    Returns (ids [K B, Tc], greedy [B, Tc] | None[, logits [R B, Tc, V]]).  residual=False: the plain model, through the same code."""
    B, Tc = video.shape[0], d.n_caption_lstm_step
    c1, h1, c2, h2 = oracle.encode(p, oracle.frame_embed(p, video))
    R = K + (1 if with_greedy else 0)
    tile = lambda a: np.tile(a, (R, 1))
    c1, h1, c2, h2 = tile(c1), tile(h1), tile(c2), tile(h2)
    vid = np.tile(np.arange(B, dtype=np.int32) + video_base, R)
    sid = np.repeat(np.arange(R, dtype=np.int32), B)
    if with_greedy:
        sid[K * B:] = -1
    tok = np.ones(R * B, np.int32)                                        # <bos>
    ids = np.empty((R * B, Tc), np.int32)
    all_logits = []
    for t in range(Tc):
        c1, h1, o1, _, _ = oracle.lstm1_step(p, None, c1, h1)
        c2, h2, o2, _, _ = oracle.lstm2_step(p, o1, tok, c2, h2)
        logits = oracle.xw_plus_b(_sum(o1, o2, residual), p["embed_word_W"], p["embed_word_b"])
        tok = oracle.pick_tokens(logits, vid, sid, t, seed)
        ids[:, t] = tok
        if return_logits:
            all_logits.append(logits)
    out = (ids[:K * B], ids[K * B:] if with_greedy else None)
    return out + (np.stack(all_logits, 1),) if return_logits else out


def residual_teacher_forced(oracle, p, d, video_rows, caption, drop=None, keep=1.0, residual=True):
    """oracle.teacher_forced with the residual sum on the DROPPED outputs of both cells.  video_rows [N, Tv, D]; logits [N, Tc, V]."""
    N, Tc = video_rows.shape[0], d.n_caption_lstm_step
    g = (lambda k: None) if drop is None else (lambda k: drop[k])
    c1, h1, c2, h2 = oracle.encode(p, oracle.frame_embed(p, video_rows), g("enc1"), g("enc2"), keep)
    caption = np.ascontiguousarray(caption, np.int32)
    logits = np.empty((N, Tc, d.n_words), np.float32)
    for t in range(Tc):
        prev = np.ones(N, np.int32) if t == 0 else caption[:, t - 1].copy()
        c1, h1, o1, _, _ = oracle.lstm1_step(p, None, c1, h1, None if drop is None else drop["dec1"][t], keep)
        c2, h2, o2, _, _ = oracle.lstm2_step(p, o1, prev, c2, h2, None if drop is None else drop["dec2"][t], keep)
        logits[:, t] = oracle.xw_plus_b(_sum(o1, o2, residual), p["embed_word_W"], p["embed_word_b"])
    return logits


def torch_teacher_forced(pt, video, caption, drop=None, keep=1.0, residual=True, detach_o1=False):
    """The loop of oracle.s2vt_torch.unroll / teacher_forced on torch tensors of pt's dtype, with the residual sum.  logits [N, Tc, V].
    detach_o1: the same values with no gradient through the o1 addend -- what a backward that forgot the ds -> o1 term computes."""
    import torch
    from oracle import s2vt_torch as T
    caption = torch.as_tensor(np.asarray(caption)).long()
    N, Tv, D = video.shape
    Tc = caption.shape[1]
    E, H, dt = pt["encode_image_W"].shape[1], pt["lstm1_W"].shape[1] // 4, pt["lstm1_W"].dtype
    video = torch.as_tensor(video).to(dt)
    emb = (video.reshape(N * Tv, D) @ pt["encode_image_W"] + pt["encode_image_b"]).reshape(N, Tv, E)
    z = lambda: torch.zeros(N, H, dtype=dt)
    c1, h1, c2, h2 = z(), z(), z(), z()
    pad = torch.zeros(N, E, dtype=dt)
    g = (lambda k, t: None) if drop is None else (lambda k, t: torch.as_tensor(drop[k][t]).to(dt))
    for t in range(Tv):
        o1, c1, h1 = T.lstm_cell(emb[:, t], c1, h1, pt["lstm1_W"], pt["lstm1_b"], g("enc1", t), keep)
        o2, c2, h2 = T.lstm_cell(torch.cat([o1, pad], 1), c2, h2, pt["lstm2_W"], pt["lstm2_b"], g("enc2", t), keep)
    out = []
    for t in range(Tc):
        prev = torch.ones(N, dtype=torch.long) if t == 0 else caption[:, t - 1]
        o1, c1, h1 = T.lstm_cell(pad, c1, h1, pt["lstm1_W"], pt["lstm1_b"], g("dec1", t), keep)
        o2, c2, h2 = T.lstm_cell(torch.cat([o1, pt["Wemb"][prev]], 1), c2, h2, pt["lstm2_W"], pt["lstm2_b"], g("dec2", t), keep)
        s = (o1.detach() if detach_o1 else o1) + o2 if residual else o2
        out.append(s @ pt["embed_word_W"] + pt["embed_word_b"])
    return torch.stack(out, 1)


def visibility(name, res, plain):
    """res / plain: (ids [K B, Tc], greedy [B, Tc]) of the residual and of the plain decode of the same case.  The conditions under which
    equality with the residual restatement shows that the model bit is honoured."""
    (s_r, g_r), (s_p, g_p) = res, plain
    B = g_r.shape[0]
    greedy_diff = int((g_r != g_p).any(1).sum())
    multi_diff = int((s_r != s_p).any(1).sum())
    n_multi = s_r.shape[0]
    out = {"the ids are not all one token": len(np.unique(np.concatenate([s_r.ravel(), g_r.ravel()]))) > 1}
    out[f"every greedy row differs ({greedy_diff}/{B})"] = greedy_diff == B
    # at least half of the multinomial rows where the rows are many; at least one at the two 5-video shapes (one-step decodes ONE token per row)
    need = 1 if name in ("small-odd", "one-step") else (n_multi + 1) // 2
    out[f"multinomial rows differ ({multi_diff}/{n_multi}, need {need})"] = multi_diff >= need
    return out


def assert_visible(name, res, plain):
    bad = [k for k, ok in visibility(name, res, plain).items() if not ok]
    assert not bad, f"the case shows nothing: {bad}"
