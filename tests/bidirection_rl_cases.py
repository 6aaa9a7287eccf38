"""Cases and CPU restatements for the bidirectional captioner's self-critical REINFORCE stage (s2vt_amd.bidirection_rl; csrc/bidir.hip:
s2vt_bidir_sample, s2vt_bidir_teacher_forced_fwd_rows, s2vt_bidir_bptt_bwd_rows), shared by the tests of that stage.

Parameters are bidirection_cases.case's with a COPY of embed_word_b whose entry 0 (<eos>) is raised by EOS_BIAS (3.0; 5.0 at chain-range), so that a good part of
the sampled rows end before Tc (the mask is ragged) and at least one does not.  Rows are sample-major: row s * B + j is sample s of
video j, the video of row n is n % B.  S is the number of samples per video of a shape.

Two restatements:
  * sample(): bidirection_cases.greedy's loop on (S + 1) * B rows -- output1 and LSTM2's encoder state tiled per row, the pick
    oracle.pick_tokens(logits, video id, sample id, t, seed) with sample id -1 (argmax) on the last block.  row_video: the row -> video map
    (default n % B; "wrong" = n // S, what a row-major driver would use, for the operands AND the noise counter; "wrong-operands" = n // S
    for the operands only).  The multinomial picks are dominated by the noise: with the right counters and the wrong operands only a
    few rows change (0 of 15 at small-odd, 5 of 80 at one-tile, 7 of 450 at many-rows) and the greedy block, collapsed onto <eos> by
    the raised bias, does not change at all: the sampled ids pin the counters.  The operand map is pinned by the bit-equal logits of the
    rows forward and, for the sampler, by its greedy block at bidirection_cases' own parameters, whose greedy ids tell the videos apart
    (test_gpu_bidirection_rl.py::test_sampler_greedy_block_at_the_unbiased_parameters).
  * torch_objective(): the model body of bidirection_cases.torch_loss on the tiled video in torch (float64 under autograd), then
    oracle.s2vt_torch.pg_loss: - sum lp mask (r - b) / sum(mask), no loss_weight, no weight decay."""
import numpy as np

import bidirection_cases as BC

SAMPLES = {"small-odd": 3, "one-tile": 5, "rows-64": 2, "rows-65": 2, "many-rows": 3, "chain-range": 3, "one-step": 3}
EOS_BIAS = {name: 3.0 for name in SAMPLES}
EOS_BIAS["chain-range"] = 5.0        # |V| = 2000: at 3.0 only 3 of its 48 sampled rows end before Tc; at 5.0, 24 do (test_bidirection_rl_cases_cpu.py)
SAMPLE_SEED = 11
MULTI_STEP = tuple(n for n in SAMPLES if n != "one-step")

_cache = {}


def case(oracle, name):
    """(params, dims, video [B, Tv, D], S): bidirection_cases.case's arrays, embed_word_b copied and raised at <eos>; built once, never written to."""
    if name not in _cache:
        p, d, video, *_ = BC.case(oracle, name)
        q = dict(p)
        q["embed_word_b"] = p["embed_word_b"].copy()
        q["embed_word_b"][0] += np.float32(EOS_BIAS[name])
        _cache[name] = (q, d, video, SAMPLES[name])
    return _cache[name]


def row_ids(B, S, with_greedy=True, video_base=0):
    """(video ids, sample ids) of the sample-major rows, the greedy block last with sample id -1"""
    blocks = S + (1 if with_greedy else 0)
    vid = np.tile(np.arange(B, dtype=np.int32) + video_base, blocks)
    sid = np.repeat(np.arange(blocks, dtype=np.int32), B)
    if with_greedy:
        sid[S * B:] = -1
    return vid, sid


def sample(oracle, p, d, video, S, seed=SAMPLE_SEED, video_base=0, row_video="mod"):
    """(sampled [S * B, Tc], greedy [B, Tc], logits [(S + 1) * B, Tc, V]) int32 / fp32: the sampler restated on the CPU."""
    Tv, Tc = d.n_video_lstm_step, d.n_caption_lstm_step
    B = video.shape[0]
    R = (S + 1) * B
    vid, sid = row_ids(B, S, True, video_base)
    rows = np.arange(R)
    src = rows % B if row_video == "mod" else np.minimum(rows // max(S, 1), B - 1)
    if row_video == "wrong":                               # the video of a row is also its noise counter
        vid = (video_base + src).astype(np.int32)
    o1 = BC.output1(oracle, p, d, video)
    c, h = BC._encode2(oracle, p, d, o1, None, 1.0)
    c, h = np.ascontiguousarray(c[src]), np.ascontiguousarray(h[src])
    tok = np.ones(R, np.int32)
    ids = np.empty((R, Tc), np.int32); logits = np.empty((R, Tc, d.n_words), np.float32)
    for t in range(Tc):
        c, h, out = BC._lstm2_step(oracle, p, d, np.ascontiguousarray(o1[Tv + t][src]), tok, c, h, None, 1.0)
        logits[:, t] = oracle.xw_plus_b(out, p["embed_word_W"], p["embed_word_b"])
        tok = oracle.pick_tokens(logits[:, t].copy(), vid, sid, t, seed)
        ids[:, t] = tok
    return ids[:S * B], ids[S * B:], logits


def reference(oracle, name):
    """{"sampled", "greedy", "logits", "mask"} of a case: computed once, shared, never written to."""
    key = ("reference", name)
    if key not in _cache:
        p, d, video, S = case(oracle, name)
        s, g, lg = sample(oracle, p, d, video, S)
        _cache[key] = {"sampled": s, "greedy": g, "logits": lg, "mask": mask_from_ids(s)}
    return _cache[key]


def mask_from_ids(ids):
    """1 up to and including the first <eos> = 0 (hostglue.masks_from_ids, restated)"""
    eos = ids == 0
    return ((np.cumsum(eos, 1) - eos) == 0).astype(np.float32)


def teacher_forced(oracle, name, keep, drop_seed=BC.DROP_SEED):
    """BC.teacher_forced on the S-times tiled block with the sampled captions and the row ids: [N, Tc, V]; computed once per (case, keep)."""
    key = ("tf", name, keep, drop_seed)
    if key not in _cache:
        p, d, video, S = case(oracle, name)
        B = video.shape[0]
        vid, sid = row_ids(B, S, False)
        tiled = np.ascontiguousarray(np.tile(video, (S, 1, 1)))
        _cache[key] = BC.teacher_forced(oracle, p, d, tiled, reference(oracle, name)["sampled"], vid, sid, keep, drop_seed=drop_seed)
    return _cache[key]


def torch_objective(pt, d, video, caption, mask, rewards, baseline, drop=None, keep=1.0):
    """- sum lp mask (r - b) / sum(mask) on torch tensors of pt's dtype; video [N, Tv, D] is the tiled block (row n = video n % B)."""
    import torch
    from oracle import s2vt_torch as T
    dt = pt["Wemb"].dtype
    video = torch.as_tensor(video).to(dt)
    caption = torch.as_tensor(np.asarray(caption)).long()
    N, Tv, D = video.shape
    Tc, E, H = caption.shape[1], d.word_dim, d.lstm_dim
    Tt = Tv + Tc
    emb = (video.reshape(N * Tv, D) @ pt["encode_image_W"] + pt["encode_image_b"]).reshape(N, Tv, E)
    pad = torch.zeros(N, E, dtype=dt)
    x = lambda t: emb[:, t] if t < Tv else pad

    def run(name, order):
        c = torch.zeros(N, H, dtype=dt); h = torch.zeros(N, H, dtype=dt)
        out = {}
        for t in order:
            _, c, h = T.lstm_cell(x(t), c, h, pt[name + "_W"], pt[name + "_b"])
            out[t] = h
        return out
    fw = run("lstm1_fw", range(Tt))
    bw = run("lstm1_bw", range(Tt - 1, -1, -1))
    c = torch.zeros(N, H, dtype=dt); h = torch.zeros(N, H, dtype=dt)
    g = (lambda k, t: None) if drop is None else (lambda k, t: torch.as_tensor(drop[k][t]).to(dt))
    for t in range(Tv):
        _, c, h = T.lstm_cell(torch.cat([fw[t], bw[t], pad], 1), c, h, pt["lstm2_W"], pt["lstm2_b"], g("enc2", t), keep)
    logits = []
    for t in range(Tc):
        prev = torch.ones(N, dtype=torch.long) if t == 0 else caption[:, t - 1]
        out, c, h = T.lstm_cell(torch.cat([fw[Tv + t], bw[Tv + t], pt["Wemb"][prev]], 1), c, h, pt["lstm2_W"], pt["lstm2_b"], g("dec2", t), keep)
        logits.append(out @ pt["embed_word_W"] + pt["embed_word_b"])
    return T.pg_loss(torch.stack(logits, 1), caption, mask, rewards, baseline)


def rewards(name, N):
    """r, b ~ U(-1, 1) from default_rng(100 + i), i the case's position"""
    rng = np.random.default_rng(100 + list(SAMPLES).index(name))
    return rng.uniform(-1, 1, N).astype(np.float32), rng.uniform(-1, 1, N).astype(np.float32)


def torch_grads(oracle, name, keep, mask=None, drop_seed=BC.DROP_SEED):
    """(loss, {name: gradient}) in float64 for a case's sampled captions (mask None: derived from the ids): computed once, shared."""
    key = ("torch_grads", name, keep, None if mask is None else mask.tobytes(), drop_seed)
    if key not in _cache:
        import torch
        from oracle import s2vt_torch as T
        p, d, video, S = case(oracle, name)
        B = video.shape[0]
        ref = reference(oracle, name)
        vid, sid = row_ids(B, S, False)
        drop = oracle.dropout_masks(drop_seed, vid, sid, keep, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step) if keep < 1.0 else None
        pt = T.to_torch(p, torch.float64, True)
        r, b = rewards(name, S * B)
        loss = torch_objective(pt, d, np.tile(video, (S, 1, 1)), ref["sampled"], ref["mask"] if mask is None else mask, r.astype(np.float64),
                               b.astype(np.float64), drop, keep)
        loss.backward()
        _cache[key] = (float(loss.detach()), {n: pt[n].grad.numpy().copy() for n in pt})
    return _cache[key]
