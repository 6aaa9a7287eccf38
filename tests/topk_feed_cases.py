"""Shapes, masks and a CPU restatement of the top-k score-weighted unroll (sum_generate_words_tf_s2vt.py:101-275; s2vt_topk_feed_fwd /
_bptt_bwd / _decode, ops.topk_feed_*, Video_Caption_Generator.topk_feed_update), shared by the top-k feed tests.

The restatement is written from oracle.s2vt_oracle's pieces the way tests/averaged_cases.py restates the averaged unroll: the mix enters
lstm2_step through a parameter dict whose "Wemb" is the step's X block, with rowidx = arange(N) -- the same ascending-k chain over a dense
operand.  The mix itself is formed in numpy float32, one rounded operation at a time: S = ((s0 + s1) + s2) + ..., w = s / S, and
x = ((((0 + w0 e0) + w1 e1) + ...) in ascending k.

Shapes: scheduled_cases' small-odd, many-rows (150 rows), one-step (Tc = 1: no mix is ever formed) and chain-range, and averaged_cases'
odd-width (word_dim 25).  Parameters are averaged_cases.tiled_case's recipe on one sample per video: oracle.init_params(seed = 3) with
all four biases uniform in +-0.1; even ground-truth ids (an odd selected word is in no caption); averaged_cases.ragged_mask.

variant= builds the half-built rules tests/test_topk_feed_cases_cpu.py tells the restatement apart from."""
import numpy as np

import averaged_cases as ac
import scheduled_cases as sc

K = 5
SHAPES = {k: sc.SHAPES[k] for k in ("small-odd", "many-rows", "one-step", "chain-range")}
SHAPES["odd-width"] = ac.SHAPES["odd-width"]
GRAD_SHAPES = ("small-odd", "many-rows", "odd-width")           # (chain-range: forward only; one-step: no mix)
KEEPS = (1.0, 0.9)
DROP_SEED = 77
VARIANTS = ("argmax-only", "unnormalised", "softmax-weights", "descending-chain", "truth-mixed")

_cache = {}


def case(oracle, name):
    """(params, dims, video [B, Tv, D], ground truth [B, Tc], mask [B, Tc], video ids, sample ids): built once, shared, never written to."""
    dims, B = SHAPES[name]
    return ac.tiled_case(oracle, dims, B, 1)


def top_k(scores, k):
    """tf.nn.top_k: value descending, index ascending on exact ties (a stable sort of the negated scores)."""
    ids = np.argsort(-np.asarray(scores, np.float32), axis=1, kind="stable")[:, :k].astype(np.int32)
    return np.take_along_axis(np.asarray(scores, np.float32), ids, 1), ids


def mix(scores, Wemb, k, variant=None):
    """(ids [R, k], w [R, k], S [R], x [R, E]) of sum_generate_words_tf_s2vt.py:166-173, every operation rounded to float32 on its own."""
    s, ids = top_k(scores, k)
    if variant == "softmax-weights":
        z = np.asarray(scores, np.float64)
        pr = np.exp(z - z.max(1, keepdims=True))
        s = np.take_along_axis((pr / pr.sum(1, keepdims=True)).astype(np.float32), ids, 1)
    S = s[:, 0].copy()
    for j in range(1, k):
        S = (S + s[:, j]).astype(np.float32)
    w = s.copy() if variant == "unnormalised" else (s / S[:, None]).astype(np.float32)
    if variant == "argmax-only":
        w = np.zeros_like(w); w[:, 0] = 1.0
    x = np.zeros((s.shape[0], Wemb.shape[1]), np.float32)
    for j in (range(k - 1, -1, -1) if variant == "descending-chain" else range(k)):
        x = (x + (w[:, j:j + 1] * Wemb[ids[:, j]]).astype(np.float32)).astype(np.float32)
    return ids, w, S, x


def unroll(oracle, p, d, video, gt, mask, vid, sid, k=K, keep=1.0, drop_seed=DROP_SEED, loss_weight=1.0, variant=None):
    """The top-k unroll on N = B rows.  Returns a dict: logits [Tc*N, V] time-major, generated [N, Tc], coef_tm / target_tm [Tc*N], mask_sum,
    X [Tc, N, E], ids / w [Tc, N, k], S [Tc, N] (block t: what step t was fed; block 0: <bos> with weight 1), drop (the masks or None)."""
    N, Tc = gt.shape
    V, H, Tv, E = d.n_words, d.lstm_dim, d.n_video_lstm_step, d.word_dim
    W = p["Wemb"]
    drop = oracle.dropout_masks(drop_seed, vid, sid, keep, H, Tv, Tc) if keep < 1.0 else None
    g = (lambda key: None) if drop is None else (lambda key: drop[key])
    c1, h1, c2, h2 = oracle.encode(p, oracle.frame_embed(p, video), g("enc1"), g("enc2"), keep)
    truth = np.clip(gt, 0, V - 1).astype(np.int32)
    gen = np.empty((N, Tc), np.int32)
    X = np.empty((Tc, N, E), np.float32)
    ids = np.ones((Tc, N, k), np.int32)
    w = np.zeros((Tc, N, k), np.float32); w[0, :, 0] = 1.0
    S = np.ones((Tc, N), np.float32)
    logits = np.empty((Tc, N, V), np.float32)
    rows = np.arange(N, dtype=np.int32)
    X[0] = W[1]
    for t in range(Tc):
        c1, h1, o1, _, _ = oracle.lstm1_step(p, None, c1, h1, None if drop is None else drop["dec1"][t], keep)
        pt = dict(p, Wemb=np.ascontiguousarray(X[t]))
        c2, h2, o2, _, _ = oracle.lstm2_step(pt, o1, rows, c2, h2, drop_mask=None if drop is None else drop["dec2"][t], keep=keep)
        logits[t] = oracle.xw_plus_b(o2, p["embed_word_W"], p["embed_word_b"])
        i_, w_, S_, x_ = mix(logits[t], W, k, variant)
        gen[:, t] = i_[:, 0]
        if t + 1 < Tc:
            ids[t + 1], w[t + 1], S[t + 1], X[t + 1] = i_, w_, S_, x_
            if variant == "truth-mixed":
                X[t + 1] = ((x_ + W[truth[:, t]]) * np.float32(0.5)).astype(np.float32)
    mk = np.asarray(mask, np.float32)
    return dict(logits=logits.reshape(Tc * N, V), generated=gen, coef_tm=(np.float32(loss_weight) * mk.T).reshape(-1).astype(np.float32),
                target_tm=truth.T.reshape(-1).copy(), mask_sum=ac.mask_sum_fixed_order(mk), X=X, ids=ids, w=w, S=S, drop=drop, truth=truth, mask=mk)


def generate(oracle, p, d, video, k=K, weights_mode=1, unshifted_softmax=True):
    """build_generator (:221-275) for the B videos: no dropout; per step the cell on the mix, the logits, probs = exp(l) / sum exp(l)
    unshifted, the emitted word argmax(probs) (the first of the top-k ids without the softmax), the next mix from the probabilities
    (weights_mode 1) or from the logits (0).  Returns (ids [B, Tc], logits [Tc*B, V] time-major)."""
    B = video.shape[0]
    Tc, V = d.n_caption_lstm_step, d.n_words
    c1, h1, c2, h2 = oracle.encode(p, oracle.frame_embed(p, video))
    rows = np.arange(B, dtype=np.int32)
    x = np.ascontiguousarray(np.broadcast_to(p["Wemb"][1], (B, d.word_dim))).astype(np.float32)
    ids = np.empty((B, Tc), np.int32)
    logits = np.empty((Tc, B, V), np.float32)
    for t in range(Tc):
        c1, h1, o1, _, _ = oracle.lstm1_step(p, None, c1, h1)
        c2, h2, o2, _, _ = oracle.lstm2_step(dict(p, Wemb=x), o1, rows, c2, h2)
        logits[t] = oracle.xw_plus_b(o2, p["embed_word_W"], p["embed_word_b"])
        scores = logits[t]
        if unshifted_softmax:
            emitted, probs = oracle.softmax_unshifted_argmax(logits[t], want_probs=True)
            if weights_mode:
                scores = probs
        i_, _, _, x = mix(scores, p["Wemb"], k)
        ids[:, t] = emitted if unshifted_softmax else i_[:, 0]
    return ids, logits.reshape(Tc * B, V)


def selected_outside_captions(r):
    """Selected words (steps >= 1) that occur in no caption and are not <bos>."""
    if r["generated"].shape[1] == 1:
        return []
    return sorted(set(np.unique(r["ids"][1:]).tolist()) - set(np.unique(r["truth"]).tolist()) - {1})


def visibility(r):
    """The conditions under which equality with the restatement shows that the mix and its gradient are honoured.  With Tc = 1 no mix is
    ever formed: what remains is sum(mask) > 0."""
    out = {"sum(mask) > 0": r["mask_sum"] > 0}
    if r["generated"].shape[1] == 1:
        return out
    out["(a) min |S| >= 0.25"] = bool(np.abs(r["S"]).min() >= 0.25)
    out["(d) a selected word occurs in no caption"] = bool(selected_outside_captions(r))
    out["(e) some row's top-k ids change between steps"] = bool((r["ids"][1:-1] != r["ids"][2:]).any()) if r["ids"].shape[0] > 2 else True
    return out


def assert_visible(r):
    bad = [key for key, ok in visibility(r).items() if not ok]
    assert not bad, f"the case shows nothing: {bad}"


def autograd(p, video, gt, mask, r, keep, loss_weight, decay, detach_weights=False):
    """Loss, parameter gradients and d loss / d logits [Tc*N, V] of sum_generate_words_tf_s2vt.py:101-218 in float64 autograd
    (oracle/s2vt_torch.py's cell), the selected ids r["ids"] as constants: x[t] = sum_j w_j Wemb[ids_j], w = logits[t-1][ids] / their sum,
    differentiable in the scores and in Wemb; Wemb[1] at step 0.  detach_weights: the weights as constants too -- the graph a backward
    without the score edge differentiates.  video: one block per ROW ([N, Tv, D])."""
    import torch
    from oracle import s2vt_torch as T
    pt = T.to_torch(p, torch.float64, True)
    v = torch.as_tensor(video).double()
    N, Tv, D = v.shape
    Tc = gt.shape[1]
    H = pt["lstm1_W"].shape[1] // 4
    E = pt["encode_image_W"].shape[1]
    emb = (v.reshape(N * Tv, D) @ pt["encode_image_W"] + pt["encode_image_b"]).reshape(N, Tv, E)
    z = lambda: torch.zeros(N, H, dtype=torch.float64)
    c1, h1, c2, h2 = z(), z(), z(), z()
    pad = torch.zeros(N, E, dtype=torch.float64)
    drop = r["drop"]
    g = (lambda key, t: None) if drop is None else (lambda key, t: torch.as_tensor(drop[key][t]).double())
    for t in range(Tv):
        o1, c1, h1 = T.lstm_cell(emb[:, t], c1, h1, pt["lstm1_W"], pt["lstm1_b"], g("enc1", t), keep)
        o2, c2, h2 = T.lstm_cell(torch.cat([o1, pad], 1), c2, h2, pt["lstm2_W"], pt["lstm2_b"], g("enc2", t), keep)
    ids = torch.as_tensor(r["ids"]).long()
    logits = []
    for t in range(Tc):
        if t == 0:
            e = pt["Wemb"][ids[0, :, 0]]
        else:
            s = logits[t - 1].gather(1, ids[t])
            w = s / s.sum(1, keepdim=True)
            if detach_weights:
                w = w.detach()
            e = (w.unsqueeze(-1) * pt["Wemb"][ids[t]]).sum(1)
        o1, c1, h1 = T.lstm_cell(pad, c1, h1, pt["lstm1_W"], pt["lstm1_b"], g("dec1", t), keep)
        o2, c2, h2 = T.lstm_cell(torch.cat([o1, e], 1), c2, h2, pt["lstm2_W"], pt["lstm2_b"], g("dec2", t), keep)
        lt = o2 @ pt["embed_word_W"] + pt["embed_word_b"]
        lt.retain_grad()
        logits.append(lt)
    lg = torch.stack(logits, 1)                                                                                          # [N, Tc, V]
    ce = -torch.log_softmax(lg, -1).gather(2, torch.as_tensor(np.clip(gt, 0, lg.shape[2] - 1)).long().unsqueeze(-1)).squeeze(-1)
    mk = torch.as_tensor(mask).double()
    wd = sum(0.5 * (x ** 2).sum() for key, x in pt.items() if key not in ("lstm1_b", "lstm2_b"))
    loss = loss_weight * (ce * mk).sum() / mk.sum() + decay * wd                                                         # :212-218
    loss.backward()
    dlogits = np.concatenate([lt.grad.numpy() for lt in logits], 0)
    return float(loss.detach()), {key: x.grad.numpy() for key, x in pt.items()}, dlogits


def fp32_gradients(p, video, gt, mask, r, keep, loss_weight):
    """The same graph's parameter gradients in float32 autograd, the sum of the scores and the mix formed as the chains the restatement
    forms (ascending k): what a correct fp32 backward of the restated graph computes, to within its own rounding."""
    import torch
    from oracle import s2vt_torch as T
    pt = T.to_torch(p, torch.float32, True)
    v = torch.as_tensor(video).float()
    N, Tv, D = v.shape
    Tc = gt.shape[1]
    H = pt["lstm1_W"].shape[1] // 4
    E = pt["encode_image_W"].shape[1]
    emb = (v.reshape(N * Tv, D) @ pt["encode_image_W"] + pt["encode_image_b"]).reshape(N, Tv, E)
    z = lambda: torch.zeros(N, H)
    c1, h1, c2, h2 = z(), z(), z(), z()
    pad = torch.zeros(N, E)
    drop = r["drop"]
    g = (lambda key, t: None) if drop is None else (lambda key, t: torch.as_tensor(drop[key][t]).float())
    for t in range(Tv):
        o1, c1, h1 = T.lstm_cell(emb[:, t], c1, h1, pt["lstm1_W"], pt["lstm1_b"], g("enc1", t), keep)
        o2, c2, h2 = T.lstm_cell(torch.cat([o1, pad], 1), c2, h2, pt["lstm2_W"], pt["lstm2_b"], g("enc2", t), keep)
    ids = torch.as_tensor(r["ids"]).long()
    logits = []
    for t in range(Tc):
        if t == 0:
            e = pt["Wemb"][ids[0, :, 0]]
        else:
            s = logits[t - 1].gather(1, ids[t])
            S = s[:, 0]
            for j in range(1, s.shape[1]):
                S = S + s[:, j]
            w = s / S.unsqueeze(1)
            e = torch.zeros(N, E)
            for j in range(s.shape[1]):
                e = e + w[:, j:j + 1] * pt["Wemb"][ids[t, :, j]]
        o1, c1, h1 = T.lstm_cell(pad, c1, h1, pt["lstm1_W"], pt["lstm1_b"], g("dec1", t), keep)
        o2, c2, h2 = T.lstm_cell(torch.cat([o1, e], 1), c2, h2, pt["lstm2_W"], pt["lstm2_b"], g("dec2", t), keep)
        logits.append(o2 @ pt["embed_word_W"] + pt["embed_word_b"])
    lg = torch.stack(logits, 1)
    ce = -torch.log_softmax(lg, -1).gather(2, torch.as_tensor(np.clip(gt, 0, lg.shape[2] - 1)).long().unsqueeze(-1)).squeeze(-1)
    mk = torch.as_tensor(mask).float()
    loss = loss_weight * (ce * mk).sum() / mk.sum()
    loss.backward()
    return {key: x.grad.numpy() for key, x in pt.items()}


def rel_err(got, want):
    """Per tensor: the largest difference relative to the reference's largest entry."""
    return {n: float(np.abs(np.asarray(got[n], np.float64) - want[n]).max() / (np.abs(want[n]).max() + 1e-300)) for n in want}
