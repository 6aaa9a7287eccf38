"""A sharpened case for the bidirectional captioner's beam search, and a per-video CPU beam search over the CPU restatement
(bidirection_cases.teacher_forced on every live prefix + a numpy top-k in tf.nn.top_k's order), shared by the beam tests.

bidirection_cases.case's parameters give nearly flat logits (every word within a few hundredths of log(1 / V)): a search on them is
decided by differences in the second decimal and a caption ends whenever <eos> happens to rank third.  As tests/test_gpu_attn_beam.py
does for the attention model, the case is sharpened into the peaked distributions a trained model has: embed_word_W,
lstm2_W and Wemb are scaled (W_SCALE, LSTM_SCALE, WEMB_SCALE), the videos get different strengths (a linear ramp STRENGTH over the batch),
and the <eos> bias is pulled down by EOS_BASE -- out of reach -- and back up by EOS_UP, so that some captions end early and some run all
Tc steps.

The scales and the bias come from a scan on the CPU (this module's `scan`, run once by hand over W_SCALE in {10, 20, 30}, LSTM_SCALE in
{2, 4, 6}, WEMB_SCALE in {5, 10, 20} and EOS_UP in {8 .. 16}), which counts at beam 3, lnf 0 over the B = 5 videos of `small-odd`:

    videos whose beam-3 caption differs from their greedy caption / captions that end on <eos> before Tc / captions that run all Tc steps /
    decode steps in which two live rows share a parent (of 5 videos x 8 steps)

    W_SCALE LSTM_SCALE WEMB_SCALE   EOS_UP 8     10      12      14      16
       10       2         5         5/0/5/35  5/0/5/35  5/3/2/24  0/5/0/5   0/5/0/5
       20       4        10         5/0/5/30  5/0/5/30  5/3/2/27  4/5/0/16  0/5/0/8
       30       6        20         5/0/5/29  5/0/5/29  5/1/4/29  5/2/3/29  2/5/0/23

Of the 135 combinations 69 leave all five captions different from the greedy one and 39 none; below EOS_UP = 12 no caption ends, from 16
on every caption ends.  Chosen: the attention test's scales (30, 6, 20) at EOS_UP = 14, the row 5/2/3/29 -- both exits of the search loop,
and the last bias at which these scales still leave full-length captions.  test_bidirection_beam_cases_cpu.py recomputes that row and
asserts that each count is at least 1."""
import numpy as np

import bidirection_cases as BC

BASE = "small-odd"                                    # H = 32, E = 24, V = 131, Tv = 3, Tc = 9, B = 5
W_SCALE, LSTM_SCALE, WEMB_SCALE = 30.0, 6.0, 20.0
EOS_BASE, EOS_UP = 12.0, 14.0
STRENGTH = (0.2, 3.0)

_cache = {}


def sharpen(p, video, w_scale=W_SCALE, lstm_scale=LSTM_SCALE, wemb_scale=WEMB_SCALE, eos_up=EOS_UP):
    """(params, video) sharpened copies; the inputs are left as they are."""
    q = {n: a.copy() for n, a in p.items()}
    q["embed_word_W"] *= np.float32(w_scale); q["lstm2_W"] *= np.float32(lstm_scale); q["Wemb"] *= np.float32(wemb_scale)
    q["embed_word_b"][0] += np.float32(eos_up - EOS_BASE)
    v = video * np.linspace(STRENGTH[0], STRENGTH[1], video.shape[0], dtype=np.float32)[:, None, None]
    return q, np.ascontiguousarray(v, np.float32)


def case(oracle, name=BASE):
    """(params, oracle dims, video [B, Tv, D]) of the sharpened case: built once, shared, never written to."""
    if name not in _cache:
        p, d, video, _, _, _ = BC.case(oracle, name)
        q, v = sharpen(p, video)
        _cache[name] = (q, d, v)
    return _cache[name]


def topk(logits, k):
    """(ids [n, k], logp [n, k]) in tf.nn.top_k's order -- value descending, index ascending on ties -- with logp = l - lse in float64
    rounded once (the CPU tests compare decisions, not bits)."""
    l = np.asarray(logits, np.float64)
    order = np.lexsort((np.arange(l.shape[1])[None, :].repeat(l.shape[0], 0), -l), axis=1)[:, :k]
    mx = l.max(1, keepdims=True)
    lse = mx + np.log(np.exp(l - mx).sum(1, keepdims=True))
    return order.astype(np.int32), np.take_along_axis(l - lse, order, 1).astype(np.float32)


def cpu_step(oracle, p, d, video_j):
    """step(t, prefixes) -> the logits [n, V] of decode step t for every prefix of ONE video, through the teacher-forced restatement."""
    Tc = d.n_caption_lstm_step

    def step(t, prefixes):
        n = len(prefixes)
        cap = np.zeros((n, Tc), np.int32)
        for i, s in enumerate(prefixes):
            cap[i, :len(s)] = s
        v = np.ascontiguousarray(np.repeat(video_j[None], n, axis=0))
        ids = np.zeros(n, np.int32)
        return BC.teacher_forced(oracle, p, d, v, cap, ids, ids)[:, t]
    return step


def search(step_topk, Tc, k, lnf, trace=None):
    """The bookkeeping of final_beam_search.py:255-290 for one video, restated on plain lists (no heap class: candidates are kept in
    arrival order and ranked by a stable sort on the score, best first).  step_topk(t, prefixes) -> (ids [n, k], logp [n, k]).
    trace (a list): receives, per step t >= 1, the parent row of every live row.  Returns (sentence, logprob, score)."""
    wi, lp = step_topk(0, [[]])
    live = [([int(wi[0, b])], float(lp[0, b]), float(lp[0, b]), 0) for b in range(k)]        # (sentence, logprob, score, parent row)
    final, exclude = [], 0
    for t in range(1, Tc):
        mid = sorted(live, key=lambda c: -c[2])[:k]
        live = []
        if not mid:
            break
        if trace is not None:
            trace.append([c[3] for c in mid])
        wi, lp = step_topk(t, [c[0] for c in mid])
        for r, (sent, logprob, _, _) in enumerate(mid):
            for b in range(k - exclude):
                w = int(wi[r, b])
                s2, l2 = sent + [w], logprob + float(lp[r, b])
                if w == 0:
                    final.append((s2, l2, l2 / len(s2) ** lnf if lnf > 0 else l2, r))
                    exclude += 1
                else:
                    live.append((s2, l2, l2, r))
        if exclude == k:
            break
    best = sorted(final or live, key=lambda c: -c[2])[0]
    return best[0], best[1], best[2]


def cpu_beam(oracle, p, d, video, k, lnf=0.0):
    """[(sentence, logprob, score)] * B and the per-video parent traces, by the CPU restatement."""
    out, traces = [], []
    for j in range(video.shape[0]):
        st = cpu_step(oracle, p, d, video[j])
        tr = []
        out.append(search(lambda t, pre: topk(st(t, pre), k), d.n_caption_lstm_step, k, lnf, tr))
        traces.append(tr)
    return out, traces


def figures(oracle, p, d, video, k=3):
    """(videos whose beam-k caption differs from the greedy one, captions that end on <eos> before Tc, captions of all Tc steps, steps in
    which two live rows share a parent)"""
    Tc = d.n_caption_lstm_step
    beam, traces = cpu_beam(oracle, p, d, video, k)
    greedy, _ = cpu_beam(oracle, p, d, video, 1)
    differ = sum(b[0] != g[0] for b, g in zip(beam, greedy))
    early = sum(len(b[0]) < Tc and b[0][-1] == 0 for b in beam)
    full = sum(len(b[0]) == Tc for b in beam)
    shared = sum(len(set(step)) < len(step) for tr in traces for step in tr)
    return differ, early, full, shared


def scan(oracle, grid=None):
    """The scan behind the constants above: prints one row of figures per combination."""
    p, d, video, _, _, _ = BC.case(oracle, BASE)
    grid = grid or [(w, l, e, u) for w in (10.0, 20.0, 30.0) for l in (2.0, 4.0, 6.0) for e in (5.0, 10.0, 20.0) for u in (8.0, 10.0, 12.0, 14.0, 16.0)]
    rows = []
    for w, l, e, u in grid:
        q, v = sharpen(p, video, w, l, e, u)
        f = figures(oracle, q, d, v)
        rows.append(((w, l, e, u), f))
        print(f"W {w:g} LSTM {l:g} Wemb {e:g} eos_up {u:g}: differ {f[0]} early {f[1]} full {f[2]} shared-parent steps {f[3]}", flush=True)
    return rows


def make(oracle, dims, B):
    """bidirection_cases.case's recipe (same seeds, same order of draws) at dimensions that are not among its shapes:
    (params, oracle dims, video [B, Tv, D])."""
    key = ("make", tuple(sorted(dims.items())), B)
    if key not in _cache:
        d = oracle.Dims(label_dim=0, **dims)
        E, H = d.word_dim, d.lstm_dim
        q = oracle.init_params(d, seed=BC.PARAM_SEED)
        p = {n: q[n] for n in ("Wemb", "encode_image_W", "encode_image_b", "embed_word_W", "embed_word_b")}
        rng = np.random.default_rng(BC.EXTRA_SEED)
        for n, s in (("lstm1_fw_W", (E + H, 4 * H)), ("lstm1_bw_W", (E + H, 4 * H)), ("lstm2_W", (2 * H + E + H, 4 * H))):
            a = np.sqrt(6.0 / (s[0] + s[1]))
            p[n] = rng.uniform(-a, a, s).astype(np.float32)
        for n in ("lstm1_fw_b", "lstm1_bw_b", "lstm2_b"):
            p[n] = rng.uniform(-BC.BIAS_A, BC.BIAS_A, 4 * H).astype(np.float32)
        video = np.abs(np.random.default_rng(1).standard_normal((B, d.n_video_lstm_step, d.dim_image)) * 0.5).astype(np.float32)
        _cache[key] = (p, d, video)
    return _cache[key]


def first_steps(oracle, p, d, video, caption, steps):
    """bidirection_cases.teacher_forced(keep = 1) cut after `steps` decode steps: logits [B, steps, V], the same calls in the same order
    (its LSTM1 pass still covers all T steps -- the backward direction starts at the last padding).  For the one shape at which the
    whole unroll takes the CPU several seconds."""
    Tv = d.n_video_lstm_step
    B = video.shape[0]
    o1 = BC.output1(oracle, p, d, video)
    c, h = BC._encode2(oracle, p, d, o1, None, 1.0)
    logits = np.empty((B, steps, d.n_words), np.float32)
    for t in range(steps):
        prev = np.ones(B, np.int32) if t == 0 else caption[:, t - 1].copy()
        c, h, out = BC._lstm2_step(oracle, p, d, o1[Tv + t], prev, c, h, None, 1.0)
        logits[:, t] = oracle.xw_plus_b(out, p["embed_word_W"], p["embed_word_b"])
    return logits
