"""Shapes, masks and a CPU restatement of the averaged-embedding unroll (average_generate_words_tf_s2vt.py:88-165; s2vt_averaged_fwd,
ops.averaged_fwd, Video_Caption_Generator.averaged_update), shared by the averaged-embedding tests.

The restatement is written from oracle.s2vt_oracle's pieces the way tests/scheduled_cases.py restates the scheduled unroll.  The mean
operand enters lstm2_step through a parameter dict whose "Wemb" is the step's Xbar block, with rowidx = arange(N): the same ascending-k
chain over a dense operand.  The mean is formed in fp32 as (a + b) * 0.5 -- one rounded addition and an exact halving.

Shapes, parameters, videos and ground truth are scheduled_cases' small ones (the <eos> bias in them is harmless here: there is no running
mask), plus "odd-width": word_dim = 25.  The mean kernel forms one element per thread, so it has no vector width to be a multiple of; the
other drivers (cell, pick, the backward's products without a live-row list) accept any word_dim, and this shape runs them at an odd one.

variant= builds the half-built unrolls tests/test_averaged_cases_cpu.py tells the restatement apart from."""
import numpy as np

import scheduled_cases as sc

SHAPES = {k: sc.SHAPES[k] for k in ("small-odd", "many-rows", "one-step", "chain-range")}
SHAPES["odd-width"] = (dict(dim_image=48, n_words=97, word_dim=25, lstm_dim=40, n_video_lstm_step=2, n_caption_lstm_step=5), 6)
KEEPS = (1.0, 0.9)
DROP_SEED = 77
VARIANTS = ("truth-only", "argmax-only", "sum", "caption-t", "mean-at-step-0")

_cache = {}


def case(oracle, name):
    """(params, dims, video, ground truth [B, Tc], mask [B, Tc], video ids, sample ids): built once on the CPU, shared, never written to."""
    if name not in _cache:
        if name in sc.SHAPES:
            p, d, video, gt, vid, sid = sc.case(oracle, name)
        else:
            from s2vt_amd import model as M
            dims, B = SHAPES[name]
            store = M.ParamStore(M.param_shapes(dims["dim_image"], dims["n_words"], dims["word_dim"], dims["lstm_dim"]), "cpu")
            M.init_reference(store, sc.PARAM_SEED)
            p = {n: store.p[n].numpy().copy() for n in store.names}
            rng = np.random.default_rng(1)
            video = np.abs(rng.standard_normal((B, dims["n_video_lstm_step"], dims["dim_image"])) * 0.5).astype(np.float32)
            gt = rng.integers(2, dims["n_words"], (B, dims["n_caption_lstm_step"])).astype(np.int32)
            vid, sid = np.arange(B, dtype=np.int32), np.zeros(B, np.int32)
            d = oracle.Dims(label_dim=0, **dims)
        _cache[name] = (p, d, video, gt, ragged_mask(*gt.shape), vid, sid)
    return _cache[name]


def ragged_mask(N, Tc):
    """Rows of different lengths: row 0 all zeros, row 1 all ones, row n >= 2 ones up to a length that walks through 1 .. Tc."""
    m = np.zeros((N, Tc), np.float32)
    for n in range(1, N):
        m[n, :Tc if n == 1 else 1 + (3 * n) % Tc] = 1.0
    return m


def mean_rows(Wemb, a, b):
    return ((Wemb[a] + Wemb[b]) * np.float32(0.5)).astype(np.float32)


def averaged_unroll(oracle, p, d, video, gt, mask, vid, sid, keep=1.0, drop_seed=DROP_SEED, loss_weight=1.0, variant=None):
    """The averaged unroll on N = B rows.  Returns a dict: logits [Tc*N, V] time-major, generated [N, Tc], coef_tm / target_tm [Tc*N],
    mask_sum, ida / idb [Tc, N] (the id pair of every step: (1, 1) at step 0), xbar [Tc, N, E], drop (the dropout masks or None)."""
    N, Tc = gt.shape
    V, H, Tv, E = d.n_words, d.lstm_dim, d.n_video_lstm_step, d.word_dim
    W = p["Wemb"]
    drop = oracle.dropout_masks(drop_seed, vid, sid, keep, H, Tv, Tc) if keep < 1.0 else None
    g = (lambda k: None) if drop is None else (lambda k: drop[k])
    c1, h1, c2, h2 = oracle.encode(p, oracle.frame_embed(p, video), g("enc1"), g("enc2"), keep)
    truth = np.clip(gt, 0, V - 1).astype(np.int32)
    argmax_sid = np.full(N, -1, np.int32)
    gen = np.empty((N, Tc), np.int32)
    ida = np.ones((Tc, N), np.int32); idb = np.ones((Tc, N), np.int32)
    xbar = np.empty((Tc, N, E), np.float32)
    logits = np.empty((Tc, N, V), np.float32)
    rows = np.arange(N, dtype=np.int32)
    for t in range(Tc):
        if t == 0:
            xbar[0] = W[1] if variant != "mean-at-step-0" else mean_rows(W, np.ones(N, np.int64), truth[:, 0])
        else:
            ida[t] = truth[:, t] if variant == "caption-t" else truth[:, t - 1]
            idb[t] = gen[:, t - 1]
            if variant == "truth-only":
                xbar[t] = W[ida[t]]
            elif variant == "argmax-only":
                xbar[t] = W[idb[t]]
            elif variant == "sum":
                xbar[t] = W[ida[t]] + W[idb[t]]
            else:
                xbar[t] = mean_rows(W, ida[t], idb[t])
        c1, h1, o1, _, _ = oracle.lstm1_step(p, None, c1, h1, None if drop is None else drop["dec1"][t], keep)
        pt = dict(p, Wemb=np.ascontiguousarray(xbar[t]))
        c2, h2, o2, _, _ = oracle.lstm2_step(pt, o1, rows, c2, h2, drop_mask=None if drop is None else drop["dec2"][t], keep=keep)
        logits[t] = oracle.xw_plus_b(o2, p["embed_word_W"], p["embed_word_b"])
        gen[:, t] = oracle.pick_tokens(logits[t], vid, argmax_sid, t, 0)
    mk = np.asarray(mask, np.float32)
    total = mask_sum_fixed_order(mk)
    return dict(logits=logits.reshape(Tc * N, V), generated=gen, coef_tm=(np.float32(loss_weight) * mk.T).reshape(-1).astype(np.float32),
                target_tm=truth.T.reshape(-1).copy(), mask_sum=total, ida=ida, idb=idb, xbar=xbar, drop=drop, truth=truth, mask=mk)


def mask_sum_fixed_order(mask):
    """sum(mask) in the order of the library's one-workgroup kernel: thread i adds entries i, i + 256, ..., a shuffle tree per 64 lanes,
    then (s0 + s1) + (s2 + s3).  The masks here are 0 / 1 with small sums, so every order gives the same float; the order is restated anyway."""
    flat = np.asarray(mask, np.float32).reshape(-1)
    lanes = np.zeros(256, np.float32)
    for i in range(256):
        acc = np.float32(0)
        for v in flat[i::256]:
            acc = np.float32(acc + v)
        lanes[i] = acc
    waves = []
    for wv in range(4):
        x = lanes[64 * wv:64 * wv + 64].copy()
        for off in (32, 16, 8, 4, 2, 1):
            x[:off] = (x[:off] + x[off:2 * off]).astype(np.float32)
        waves.append(x[0])
    return float(np.float32(np.float32(waves[0] + waves[1]) + np.float32(waves[2] + waves[3])))


def live_picks(r):
    """The picked words whose lookup carries gradient: the pick of step t - 1 that row n is fed at step t, where the row's mask is non-zero
    at some step >= t."""
    mask = r["mask"]
    live = (mask[:, ::-1].cumsum(1)[:, ::-1] > 0).T                      # [Tc, N]: some step >= t weighs the row
    return set(np.unique(r["idb"][1:][live[1:]]).tolist())


def only_picked_rows(r):
    """Rows of Wemb whose gradient can only come from the second scatter: live picks that are no ground-truth word of the batch and not <bos>."""
    if r["generated"].shape[1] == 1:
        return []
    return sorted(live_picks(r) - set(np.unique(r["truth"]).tolist()) - {1})


def visibility(r):
    """The conditions under which equality with the restatement shows that the mean operand and the second lookup are honoured.  With
    Tc = 1 no mean is ever formed: what remains is sum(mask) > 0."""
    out = {"sum(mask) > 0": r["mask_sum"] > 0}
    if r["generated"].shape[1] == 1:
        return out
    out["a pick differs from the ground truth it is averaged with"] = bool((r["ida"][1:] != r["idb"][1:]).any())
    out["a picked word occurs nowhere in the ground truth"] = bool(only_picked_rows(r))
    return out


def assert_visible(r):
    bad = [k for k, ok in visibility(r).items() if not ok]
    assert not bad, f"the case shows nothing: {bad}"


def tiled_case(oracle, dims, B, rep, seed=4):
    """A case on N = rep * B sample-major rows (row k * B + j = video j, sample k), for the shapes the small ones do not reach:
    (params, dims, video [B, Tv, D], ground truth [N, Tc], mask [N, Tc], video ids [N], sample ids [N])."""
    key = ("tiled", tuple(sorted(dims.items())), B, rep, seed)
    if key not in _cache:
        d = oracle.Dims(label_dim=0, **dims)
        p = oracle.init_params(d, seed=3)
        rng = np.random.default_rng(seed)
        for k in ("lstm1_b", "lstm2_b", "encode_image_b", "embed_word_b"):
            p[k] = rng.uniform(-.1, .1, p[k].shape).astype(np.float32)
        N = B * rep
        video = np.abs(rng.standard_normal((B, d.n_video_lstm_step, d.dim_image)) * 0.5).astype(np.float32)
        gt = (2 * rng.integers(1, d.n_words // 2, (N, d.n_caption_lstm_step))).astype(np.int32)   # even ids: an odd pick is in no caption
        vid = np.tile(np.arange(B, dtype=np.int32), rep); sid = np.repeat(np.arange(rep, dtype=np.int32), B)
        _cache[key] = (p, d, video, gt, ragged_mask(N, d.n_caption_lstm_step), vid, sid)
    return _cache[key]


def autograd(p, video, gt, mask, r, keep, loss_weight, decay):
    """Loss and gradients of average_generate_words_tf_s2vt.py:88-164 in float64 autograd (oracle/s2vt_torch.py's cell), the picked ids
    r["idb"] as constants: x[t] = (Wemb[truth of t-1] + Wemb[pick of t-1]) * 0.5 with both lookups differentiable, Wemb[1] at step 0.
    video: one block per ROW ([N, Tv, D])."""
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
    g = (lambda k, t: None) if drop is None else (lambda k, t: torch.as_tensor(drop[k][t]).double())
    for t in range(Tv):
        o1, c1, h1 = T.lstm_cell(emb[:, t], c1, h1, pt["lstm1_W"], pt["lstm1_b"], g("enc1", t), keep)
        o2, c2, h2 = T.lstm_cell(torch.cat([o1, pad], 1), c2, h2, pt["lstm2_W"], pt["lstm2_b"], g("enc2", t), keep)
    ida, idb = torch.as_tensor(r["ida"]).long(), torch.as_tensor(r["idb"]).long()
    logits = []
    for t in range(Tc):
        e = pt["Wemb"][ida[t]] if t == 0 else (pt["Wemb"][ida[t]] + pt["Wemb"][idb[t]]) * 0.5
        o1, c1, h1 = T.lstm_cell(pad, c1, h1, pt["lstm1_W"], pt["lstm1_b"], g("dec1", t), keep)
        o2, c2, h2 = T.lstm_cell(torch.cat([o1, e], 1), c2, h2, pt["lstm2_W"], pt["lstm2_b"], g("dec2", t), keep)
        logits.append(o2 @ pt["embed_word_W"] + pt["embed_word_b"])
    lg = torch.stack(logits, 1)                                                                                          # [N, Tc, V]
    ce = -torch.log_softmax(lg, -1).gather(2, torch.as_tensor(np.clip(gt, 0, lg.shape[2] - 1)).long().unsqueeze(-1)).squeeze(-1)
    mk = torch.as_tensor(mask).double()
    wd = sum(0.5 * (x ** 2).sum() for k, x in pt.items() if k not in ("lstm1_b", "lstm2_b"))
    loss = loss_weight * (ce * mk).sum() / mk.sum() + decay * wd                                                         # :153-164
    loss.backward()
    return float(loss.detach()), {k: x.grad.numpy() for k, x in pt.items()}
