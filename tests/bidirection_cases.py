"""Shapes, parameters and a CPU restatement of the bidirectional captioner's forward side (bidirection_tf_s2vt.py:85-216;
s2vt_amd.bidirection), shared by the bidirection tests.

The restatement is written from oracle.s2vt_oracle's pieces: frame_embed, gemm_chain, bias_add, lstm_pointwise, xw_plus_b,
pick_tokens (sample id -1 = argmax), softmax_unshifted_argmax, dropout_masks.  LSTM1 is a static_bidirectional_rnn over the Tv frames
and then the Tc zero paddings: the forward cell consumes t = 0 .. T-1, the backward cell t = T-1 .. 0 (through the paddings first),
both from a zero state, output1[t] = [h_fw after t ; h_bw after t]; LSTM2's chain is [output1[t] ; e_t ; h2] @ W2 in ascending k, then the
bias, its DropoutWrapper on LSTM2's Philox codes (build_model only).

Parameters: oracle.init_params(seed 3) for the variables shared with the plain captioner; then, from default_rng(103) in this order,
Glorot-uniform lstm1_fw_W, lstm1_bw_W, lstm2_W and U(-0.02, 0.02) lstm1_fw_b, lstm1_bw_b, lstm2_b.  The LSTM biases are NOT zero: with the
reference's zero biases the backward direction's state stays exactly 0 through the padding prefix, and a driver that skipped the prefix
would pass.  They are small: at a = 0.1 and above the greedy decode collapses to a few tokens.

VARIANTS are four wrong models a half-built driver would compute.  Rows (of B) whose greedy ids differ from the true model's, and
the number of distinct ids the true model emits, with these parameters (test_bidirection_cases_cpu.py asserts at least half the rows at
the four decoding shapes, and different teacher-forced logits at all seven):

    case (B)          forward-order  not-re-reversed  bw-zero  padding-skipped  distinct ids
    small-odd (5)           5               4             5            3             11
    one-tile (16)          16              16            16           13             19
    many-rows (150)       142             144           147          141             48
    chain-range (16)       15              16            16           12             15

(One-step, Tc = 1, does not discriminate on ids -- one token per row -- and the two row-limit shapes are there for the dispatch edge:
those three are compared on logits.)  test_bidirection_cases_cpu.py recomputes every figure and prints it.

The 64- and 65-row shapes at H = 64 sit on the two sides of the one-launch form's row limit."""
import numpy as np

import scheduled_cases as SC

SHAPES = dict(SC.SHAPES)
SHAPES["rows-64"] = (dict(dim_image=48, n_words=150, word_dim=16, lstm_dim=64, n_video_lstm_step=3, n_caption_lstm_step=5), 64)
SHAPES["rows-65"] = (dict(dim_image=48, n_words=150, word_dim=16, lstm_dim=64, n_video_lstm_step=3, n_caption_lstm_step=5), 65)
DECODING = ("small-odd", "one-tile", "many-rows", "chain-range")       # the shapes at which the greedy ids must discriminate
VARIANTS = ("forward-order", "not-re-reversed", "bw-zero", "padding-skipped")
BIAS_A = 0.02
PARAM_SEED, EXTRA_SEED, DROP_SEED = 3, 103, 77
KEEPS = (1.0, 0.9)

_cache = {}


def case(oracle, name):
    """(params, oracle dims, video [B, Tv, D], caption [B, Tc] in [2, V), video ids, sample ids): built once, shared, never written to."""
    if name not in _cache:
        dims, B = SHAPES[name]
        d = oracle.Dims(label_dim=0, **dims)
        E, H = d.word_dim, d.lstm_dim
        q = oracle.init_params(d, seed=PARAM_SEED)
        p = {n: q[n] for n in ("Wemb", "encode_image_W", "encode_image_b", "embed_word_W", "embed_word_b")}
        rng = np.random.default_rng(EXTRA_SEED)
        for n, s in (("lstm1_fw_W", (E + H, 4 * H)), ("lstm1_bw_W", (E + H, 4 * H)), ("lstm2_W", (2 * H + E + H, 4 * H))):
            a = np.sqrt(6.0 / (s[0] + s[1]))
            p[n] = rng.uniform(-a, a, s).astype(np.float32)
        for n in ("lstm1_fw_b", "lstm1_bw_b", "lstm2_b"):
            p[n] = rng.uniform(-BIAS_A, BIAS_A, 4 * H).astype(np.float32)
        rng = np.random.default_rng(1)
        video = np.abs(rng.standard_normal((B, d.n_video_lstm_step, d.dim_image)) * 0.5).astype(np.float32)
        cap = rng.integers(2, d.n_words, (B, d.n_caption_lstm_step)).astype(np.int32)
        _cache[name] = (p, d, video, cap, np.arange(B, dtype=np.int32), np.zeros(B, np.int32))
    return _cache[name]


def _direction(oracle, W, b, emb, T, order):
    """one BasicLSTMCell over the time steps in `order` from a zero state: {t: h after t}.  Input = emb[:, t] for t < Tv, else zeros."""
    B, Tv, E = emb.shape
    H = W.shape[1] // 4
    c = np.zeros((B, H), np.float32); h = np.zeros((B, H), np.float32)
    out = {}
    for t in order:
        if t < Tv:
            z = oracle.gemm_chain(np.ascontiguousarray(emb[:, t]), W[:E])
            oracle.gemm_chain(h, W[E:], z)
        else:
            z = oracle.gemm_chain(h, W[E:])                 # zero rows contribute nothing to the chain
        oracle.bias_add(z, b)
        c, h, _, _ = oracle.lstm_pointwise(z, c)
        out[t] = h
    return out


def output1(oracle, p, d, video, variant=None):
    """[T] arrays [B, 2H] = [fw ; bw] (bidirection_tf_s2vt.py:113-117).  variant: one of VARIANTS, a wrong model."""
    assert variant is None or variant in VARIANTS
    key = ("output1", id(p), id(video), variant)
    cached = any(isinstance(v, tuple) and v and v[0] is p and v[2] is video for v in _cache.values())    # a case's own arrays live as long as the cache: only those are keyed by id
    if cached and key in _cache:
        return _cache[key]
    Tv, Tc, H = d.n_video_lstm_step, d.n_caption_lstm_step, d.lstm_dim
    T = Tv + Tc
    emb = oracle.frame_embed(p, video)
    B = emb.shape[0]
    fw = _direction(oracle, p["lstm1_fw_W"], p["lstm1_fw_b"], emb, T, range(T))
    zero = np.zeros((B, H), np.float32)
    if variant == "forward-order":                          # the backward cell run like the forward one
        bw = _direction(oracle, p["lstm1_bw_W"], p["lstm1_bw_b"], emb, T, range(T))
    elif variant == "bw-zero":
        bw = {t: zero for t in range(T)}
    elif variant == "padding-skipped":                      # the backward cell started at the last frame, the paddings left at zero
        bw = {t: zero for t in range(Tv, T)}
        bw.update(_direction(oracle, p["lstm1_bw_W"], p["lstm1_bw_b"], emb, T, range(Tv - 1, -1, -1)))
    else:
        bw = _direction(oracle, p["lstm1_bw_W"], p["lstm1_bw_b"], emb, T, range(T - 1, -1, -1))
        if variant == "not-re-reversed":                    # chain-step order handed on as if it were time order
            bw = {t: bw[T - 1 - t] for t in range(T)}
    out = [np.concatenate([fw[t], bw[t]], 1) for t in range(T)]
    if cached:
        _cache[key] = out
    return out


def _lstm2_step(oracle, p, d, o1, tok, c, h, mask, keep):
    H, E = d.lstm_dim, d.word_dim
    W = p["lstm2_W"]
    z = oracle.gemm_chain(np.ascontiguousarray(o1), W[:2 * H])
    if tok is not None:
        oracle.gemm_chain(p["Wemb"], W[2 * H:2 * H + E], z, rowidx=np.ascontiguousarray(tok, np.int32))
    oracle.gemm_chain(h, W[2 * H + E:], z)
    oracle.bias_add(z, p["lstm2_b"])
    c, h, out, _ = oracle.lstm_pointwise(z, c, mask, keep)
    return c, h, out


def _encode2(oracle, p, d, o1, drop, keep):
    B, H = o1[0].shape[0], d.lstm_dim
    c = np.zeros((B, H), np.float32); h = np.zeros((B, H), np.float32)
    for t in range(d.n_video_lstm_step):
        c, h, _ = _lstm2_step(oracle, p, d, o1[t], None, c, h, None if drop is None else drop["enc2"][t], keep)
    return c, h


def teacher_forced(oracle, p, d, video, caption, vid, sid, keep=1.0, variant=None, drop_seed=DROP_SEED):
    """build_model's logits [B, Tc, V] (:118-156)."""
    Tv, Tc = d.n_video_lstm_step, d.n_caption_lstm_step
    B = video.shape[0]
    drop = oracle.dropout_masks(drop_seed, vid, sid, keep, d.lstm_dim, Tv, Tc) if keep < 1.0 else None
    o1 = output1(oracle, p, d, video, variant)
    c, h = _encode2(oracle, p, d, o1, drop, keep)
    logits = np.empty((B, Tc, d.n_words), np.float32)
    for t in range(Tc):
        prev = np.ones(B, np.int32) if t == 0 else caption[:, t - 1].copy()
        c, h, out = _lstm2_step(oracle, p, d, o1[Tv + t], prev, c, h, None if drop is None else drop["dec2"][t], keep)
        logits[:, t] = oracle.xw_plus_b(out, p["embed_word_W"], p["embed_word_b"])
    return logits


def greedy(oracle, p, d, video, vid, unshifted=False, variant=None):
    """build_generator's decode (:187-215), row by row the same arithmetic: (ids [B, Tc] int32, logits [B, Tc, V]).
    unshifted: argmax(exp(l) / sum(exp(l))) as written at :211-212, else argmax(l)."""
    Tv, Tc = d.n_video_lstm_step, d.n_caption_lstm_step
    B = video.shape[0]
    o1 = output1(oracle, p, d, video, variant)
    c, h = _encode2(oracle, p, d, o1, None, 1.0)
    tok = np.ones(B, np.int32)
    ids = np.empty((B, Tc), np.int32); logits = np.empty((B, Tc, d.n_words), np.float32)
    sid = np.full(B, -1, np.int32)
    for t in range(Tc):
        c, h, out = _lstm2_step(oracle, p, d, o1[Tv + t], tok, c, h, None, 1.0)
        logits[:, t] = oracle.xw_plus_b(out, p["embed_word_W"], p["embed_word_b"])
        tok = oracle.softmax_unshifted_argmax(logits[:, t].copy()) if unshifted else oracle.pick_tokens(logits[:, t].copy(), vid, sid, t, 0)
        ids[:, t] = tok
    return ids, logits


def reference(oracle, name):
    """{"ids", "ids_unshifted", "logits_greedy", ("tf", keep): logits} of the true model for a case: computed once, shared."""
    key = ("reference", name)
    if key not in _cache:
        p, d, video, cap, vid, sid = case(oracle, name)
        ids, lg = greedy(oracle, p, d, video, vid)
        r = {"ids": ids, "logits_greedy": lg, "ids_unshifted": greedy(oracle, p, d, video, vid, unshifted=True)[0]}
        for keep in KEEPS:
            r[("tf", keep)] = teacher_forced(oracle, p, d, video, cap, vid, sid, keep)
        _cache[key] = r
    return _cache[key]


# ---- float64 restatement for gradients (oracle.s2vt_torch's cell; autograd)
LOSS_WEIGHT, DECAY = 20.0, 5e-5
BIASES = ("lstm1_fw_b", "lstm1_bw_b", "lstm2_b")


def torch_loss(pt, d, video, caption, mask, drop=None, keep=1.0, variant=None, loss_weight=None):
    """build_model's loss (:150-165) on torch tensors of pt's dtype: loss_weight * sum(xent * mask) / sum(mask) + 5e-5 * sum l2_loss over
    the variables without 'bias' in their TF name (all but the three BasicLSTMCell biases).  variant "forward-order": the wrong model."""
    import torch
    from oracle import s2vt_torch as T
    assert variant in (None, "forward-order")
    dt = pt["Wemb"].dtype
    video = torch.as_tensor(video).to(dt)
    caption = torch.as_tensor(np.asarray(caption)).long()
    mask = torch.as_tensor(np.asarray(mask)).to(dt)
    B, Tv, D = video.shape
    Tc, E, H = caption.shape[1], d.word_dim, d.lstm_dim
    Tt = Tv + Tc
    emb = (video.reshape(B * Tv, D) @ pt["encode_image_W"] + pt["encode_image_b"]).reshape(B, Tv, E)
    pad = torch.zeros(B, E, dtype=dt)
    x = lambda t: emb[:, t] if t < Tv else pad

    def run(name, order):
        c = torch.zeros(B, H, dtype=dt); h = torch.zeros(B, H, dtype=dt)
        out = {}
        for t in order:
            _, c, h = T.lstm_cell(x(t), c, h, pt[name + "_W"], pt[name + "_b"])
            out[t] = h
        return out
    fw = run("lstm1_fw", range(Tt))
    bw = run("lstm1_bw", range(Tt) if variant == "forward-order" else range(Tt - 1, -1, -1))
    c = torch.zeros(B, H, dtype=dt); h = torch.zeros(B, H, dtype=dt)
    g = (lambda k, t: None) if drop is None else (lambda k, t: torch.as_tensor(drop[k][t]).to(dt))
    for t in range(Tv):
        _, c, h = T.lstm_cell(torch.cat([fw[t], bw[t], pad], 1), c, h, pt["lstm2_W"], pt["lstm2_b"], g("enc2", t), keep)
    tot = 0.0
    for t in range(Tc):
        prev = torch.ones(B, dtype=torch.long) if t == 0 else caption[:, t - 1]
        out, c, h = T.lstm_cell(torch.cat([fw[Tv + t], bw[Tv + t], pt["Wemb"][prev]], 1), c, h, pt["lstm2_W"], pt["lstm2_b"], g("dec2", t), keep)
        logits = out @ pt["embed_word_W"] + pt["embed_word_b"]
        xent = -torch.log_softmax(logits, 1).gather(1, caption[:, t:t + 1])[:, 0]
        tot = tot + (LOSS_WEIGHT if loss_weight is None else loss_weight) * (xent * mask[:, t]).sum()
    wd = sum((v ** 2).sum() / 2 for n, v in pt.items() if n not in BIASES)
    return tot / mask.sum() + DECAY * wd


def caption_mask(name, cap):
    """ragged lengths, at least one full row and one row of a single word"""
    B, Tc = cap.shape
    rng = np.random.default_rng(len(name))
    lens = rng.integers(1, Tc + 1, B); lens[0] = Tc; lens[-1] = 1
    return (np.arange(Tc)[None, :] < lens[:, None]).astype(np.float32)


def torch_grads(oracle, name, keep, variant=None):
    """(loss, {name: gradient}) in float64 for a case: computed once, shared."""
    key = ("torch_grads", name, keep, variant)
    if key not in _cache:
        import torch
        from oracle import s2vt_torch as T
        p, d, video, cap, vid, sid = case(oracle, name)
        drop = oracle.dropout_masks(DROP_SEED, vid, sid, keep, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step) if keep < 1.0 else None
        pt = T.to_torch(p, torch.float64, True)
        loss = torch_loss(pt, d, video, cap, caption_mask(name, cap), drop, keep, variant)
        loss.backward()
        _cache[key] = (float(loss.detach()), {n: pt[n].grad.numpy().copy() for n in pt})
    return _cache[key]
