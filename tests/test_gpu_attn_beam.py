"""Batched beam search for the temporal-attention captioner (s2vt_attn_beam_*, ops.AttnBeamDecoder, BatchedBeamSearch over it,
Attention_Caption_Generator.beam_search / build_generator(beam_size), train_common.beam_eval, the beam_eval CLI).

1. the step's arithmetic, bit for bit against the CPU oracle's teacher-forced unroll of each hypothesis' word prefix;
2. beam 1 == the greedy decode loop;
3. the whole search, exact, against a per-video driver that teacher-forces every live prefix through the EXISTING unroll
   (ops.attn_teacher_forced_fwd) -- the same floats by 1., so sentences, logprob and score must agree to the byte;
4. a video decodes to the same bytes whatever batch it is in;
5. the model / evaluation / CLI surface."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_SCALE, LSTM_SCALE, WEMB_SCALE = 30.0, 6.0, 20.0           # tools/make_beam_fixtures.py
EOS_BASE = 12.0                                             # the small models start with <eos> this far down: the sweeps bias it back up


def _bytes(x):
    return np.float64(x).tobytes()


def _model(oracle, D, V, H, Tv, Tc, B, seed, scaled=False):
    from s2vt_amd import attention as A
    d = oracle.Dims(dim_image=D, n_words=V, word_dim=0, lstm_dim=H, n_video_lstm_step=Tv, n_caption_lstm_step=Tc, label_dim=0)
    p = oracle.init_attention_params(d, seed)
    rng = np.random.default_rng(seed + 1)
    for k in ("lstm3_b", "embed_att_ba", "embed_nn_bp", "embed_word_b", "encode_image_b"):
        p[k] = rng.uniform(-.1, .1, p[k].shape).astype(np.float32)
    video = np.abs(rng.standard_normal((B, Tv, D)) * 0.5).astype(np.float32)
    if scaled:          # a search with something to decide: sharp logits, videos of different strength, <eos> out of reach until biased
        p["embed_word_W"] *= np.float32(W_SCALE); p["lstm3_W"] *= np.float32(LSTM_SCALE); p["Wemb"] *= np.float32(WEMB_SCALE)
        p["embed_word_b"][0] -= np.float32(EOS_BASE)
        video *= np.linspace(0.2, 3.0, B, dtype=np.float32)[:, None, None]
    m = A.Attention_Caption_Generator(D, V, H, B, Tv, Tc, 0.9)
    m.load(p)
    return d, p, m, video, rng


# ------------------------------------------------------------------------------------------------ 1. the step against the oracle
@pytest.mark.parametrize("D,V,H,Tv,Tc", [(48, 131, 32, 5, 6),        # 16-byte path
                                         (40, 97, 18, 33, 4),        # scalar path (H % 4 != 0); Tv crosses the 32-frame LDS chunk
                                         (40, 97, 36, 12, 4)])
def test_step_bit_exact_against_oracle(gpu, oracle, D, V, H, Tv, Tc):
    import torch
    ops = gpu
    B, beam, k = 3, 4, 3
    d, p, m, video, rng = _model(oracle, D, V, H, Tv, Tc, B, 7)
    w = lambda n: rng.integers(0, V, n).tolist()
    # (video, parent row of the previous step, word) per row
    tree = [
        ([0, 1, 2], [9, 9, 9], [5, 6, 7]),                                  # step 0: one row per video; parent and word are ignored
        ([2, 0, 1, 0, 2, 1, 2], [2, 0, 1, 0, 2, 1, 2], w(7)),               # step 1: 2B + 1 rows, videos (= parents) mixed
        ([2, 0, 2, 0, 2, 2], [4, 1, 0, 3, 4, 6], w(6)),                     # step 2: interleaved, video 1 absent, parent 4 twice
        ([0], [3], w(1)),                                                   # step 3: R = 1
    ]
    dec = ops.AttnBeamDecoder(m.dims, B, beam, m.device)
    # P and Vt once per VIDEO, everything else O(B * beam) rows of H or V floats: no [Tv, H] block per hypothesis
    assert dec.ws.numel() < 4 * (2 * Tv * B * H + B * beam * (Tv * H // 2 + V)) + 64 * 256
    vdev = torch.as_tensor(video).cuda()
    dec.encode(m.store.params, vdev)
    ref = {}                                                                # (video, prefix) -> (logits [Tc, V], alphas [Tc, Tv])

    def reference(vid, prefix):
        key = (vid, tuple(prefix))
        if key not in ref:
            cap = np.zeros((1, Tc), np.int32)
            cap[0, :len(prefix)] = prefix
            lg, al, _ = oracle.attention_forward(p, d, video[[vid]], cap, keep=1.0)
            ref[key] = (lg[0], al[:, :, 0])
        return ref[key]

    prev = None
    for t, (vids, parents, words) in enumerate(tree):
        rows = np.array([vids, parents, words], np.int32)
        ids, lp, logits, alphas = dec.step(m.store.params, t, rows, k, want_logits=True, want_alphas=True)
        prefixes = [[] if t == 0 else prev[parents[i]] + [words[i]] for i in range(len(vids))]
        lg, al = logits.cpu().numpy(), alphas.cpu().numpy()
        assert lg.shape == (len(vids), V) and al.shape == (Tv, len(vids))
        for i, (vid, prefix) in enumerate(zip(vids, prefixes)):
            assert t == 0 or vid == tree[t - 1][0][parents[i]]              # the script is a tree: a row continues its own video
            rl, ra = reference(vid, prefix)
            assert np.array_equal(al[:, i], ra[t]), (t, i)
            assert np.array_equal(lg[i], rl[t]), (t, i)
        tid, tlp = ops.vocab_topk(logits, k)
        assert np.array_equal(ids, tid.cpu().numpy())
        assert np.array_equal(lp.view(np.uint32), tlp.cpu().numpy().view(np.uint32))
        ids2, lp2 = dec.step(m.store.params, t, rows, k)                    # the same step on the workspace's own logits buffer
        assert np.array_equal(ids2, ids) and np.array_equal(lp2.view(np.uint32), lp.view(np.uint32))
        prev = prefixes


# ------------------------------------------------------------------------------------------------ full-dimension models
_BIG = {}


def _big(Tv):
    """BASELINE configs[2] dimensions of the attention captioner (D 1536, V 12000, H 1000, Tc 20, 16 videos), weights scaled as
    tools/make_beam_fixtures.py scales them; one set of variables serves both frame counts."""
    import torch
    from s2vt_amd import attention as A
    if Tv not in _BIG:
        mdl = A.Attention_Caption_Generator(1536, 12000, 1000, 16, Tv, 20, 0.9, seed=11)
        if _BIG:
            first = next(iter(_BIG.values()))[0]
            mdl.store.theta.copy_(first.store.theta)
        else:
            with torch.no_grad():
                mdl.p["embed_word_W"].mul_(W_SCALE); mdl.p["lstm3_W"].mul_(LSTM_SCALE); mdl.p["Wemb"].mul_(WEMB_SCALE)
        rng = np.random.default_rng(5)
        scale = np.linspace(0.2, 2.0, 16, dtype=np.float32)[:, None, None]        # videos of different strength: different beams
        _BIG[Tv] = (mdl, (np.abs(rng.standard_normal((16, Tv, 1536))) * scale * 0.5).astype(np.float32))
    return _BIG[Tv]


# ------------------------------------------------------------------------------------------------ 2. beam 1 == greedy
def _assert_beam1_is_greedy(ops, mdl, video):
    import torch
    Tc = mdl.n_caption_lstm_steps
    ids, _ = ops.attn_decode_greedy(mdl.dims, mdl.store.params, torch.as_tensor(video).cuda())
    ids = ids.cpu().numpy()
    res = mdl.beam_search(video, 1, 0.0)
    assert len(res) == len(video)
    ended = 0
    for j, (s, lp, sc) in enumerate(res):
        g = ids[j].tolist()
        # up to and including the first <eos> -- behind the first word, which the search pushes untested (final_beam_search.py:258-262)
        n = g.index(0, 1) + 1 if 0 in g[1:] else Tc
        assert s == g[:n], j
        assert _bytes(lp) == _bytes(sc)
        ended += n < Tc
    return ended


def test_beam1_equals_greedy_small(gpu, oracle):
    import torch
    _, _, mdl, video, _ = _model(oracle, 24, 60, 20, 5, 7, 9, 3, scaled=True)
    _assert_beam1_is_greedy(gpu, mdl, video)
    with torch.no_grad():
        mdl.p["embed_word_b"][0] += 15.0                                    # ... and with captions that end early
    assert _assert_beam1_is_greedy(gpu, mdl, video) > 0


def test_beam1_equals_greedy_full_dimensions(gpu):
    mdl, video = _big(5)
    _assert_beam1_is_greedy(gpu, mdl, video)


# ------------------------------------------------------------------------------------------------ 3. whole search, independent driver
def _per_video_search(step, Tc, k, lnf):
    """BeamSearchGenerator.generate's bookkeeping (beam_generator.py) for one video over step(t, prefixes) -> (ids [n, k], logp [n, k])."""
    from s2vt_amd.beam_generator import BestK, Hypothesis
    captions, final_captions = BestK(k * k), BestK(k)
    wi, lp = step(0, [[]])
    for b in range(k):
        captions.push(Hypothesis([int(wi[0, b])], 0, float(lp[0, b]), float(lp[0, b])))
    exclude = 0
    for t in range(1, Tc):
        mid = captions.best_first()[:k]
        captions.clear()
        if not mid:
            break
        wi, lp = step(t, [cap.sentence for cap in mid])
        for r, cap in enumerate(mid):
            for b in range(k - exclude):
                w = int(wi[r, b])
                sentence = cap.sentence + [w]
                logprob = cap.logprob + float(lp[r, b])
                score = logprob
                if w == 0:
                    if lnf > 0:
                        score /= len(sentence) ** lnf
                    final_captions.push(Hypothesis(sentence, r, logprob, score))
                    exclude += 1
                else:
                    captions.push(Hypothesis(sentence, r, logprob, score))
        if exclude == k:
            break
    if not final_captions.size():
        final_captions = captions
    best = final_captions.best_first()[0]
    return best.sentence, best.logprob, best.score


def _teacher_forced_step(ops, mdl, video_j, k):
    """step(t, prefixes) through the existing unroll: every live prefix teacher-forced (keep = 1), the logits of step t, vocab_topk."""
    import torch
    Tc, V = mdl.n_caption_lstm_steps, mdl.n_words

    def step(t, prefixes):
        n = len(prefixes)
        cap = np.zeros((n, Tc), np.int32)
        for i, s in enumerate(prefixes):
            cap[i, :len(s)] = s
        v = torch.as_tensor(np.repeat(video_j[None], n, axis=0)).cuda().contiguous()
        logits, _, _ = ops.attn_teacher_forced_fwd(mdl.dims, mdl.store.params, v, torch.as_tensor(cap).cuda(), steps=t + 1)
        ids, lp = ops.vocab_topk(logits.view(t + 1, n, V)[t], k)
        return ids.cpu().numpy(), lp.cpu().numpy()
    return step


def _sweep(ops, mdl, video, configs):
    import torch
    from s2vt_amd.beam_generator import BatchedBeamSearch
    Tc = mdl.n_caption_lstm_steps
    b0 = float(mdl.p["embed_word_b"][0])
    early = full = 0
    for eos in (0.0, 10.0, 20.0, 40.0, 80.0):                                # <eos> bias: until captions of both kinds have been seen
        with torch.no_grad():
            mdl.p["embed_word_b"][0] = b0 + eos
        for k, lnf in configs:
            res = BatchedBeamSearch(mdl, k, lnf).generate(video)
            for j in range(video.shape[0]):
                s, lp, sc = _per_video_search(_teacher_forced_step(ops, mdl, video[j], k), Tc, k, lnf)
                bs, blp, bsc = res[j]
                assert bs == s, (eos, k, lnf, j)
                assert _bytes(blp) == _bytes(lp) and _bytes(bsc) == _bytes(sc), (eos, k, lnf, j)
                early += len(bs) < Tc
                full += len(bs) == Tc
        if early and full:
            break
    with torch.no_grad():
        mdl.p["embed_word_b"][0] = b0
    return early, full


def test_search_equals_independent_driver(gpu, oracle):
    _, _, mdl, video, _ = _model(oracle, 24, 60, 20, 5, 7, 6, 3, scaled=True)
    early, full = _sweep(gpu, mdl, video, [(3, 0.0), (3, 0.5), (5, 0.0), (5, 0.5)])
    assert early > 0 and full > 0                                            # both exits of the loop are covered


def test_search_equals_independent_driver_33_frames(gpu, oracle):
    _, _, mdl, video, _ = _model(oracle, 24, 60, 20, 33, 7, 4, 3, scaled=True)
    early, full = _sweep(gpu, mdl, video, [(3, 0.5)])
    assert early > 0 and full > 0


# ------------------------------------------------------------------------------------------------ 4. batch composition
def test_batch_composition_invariance(gpu):
    from s2vt_amd.beam_generator import BatchedBeamSearch
    mdl, video = _big(32)
    alone = BatchedBeamSearch(mdl, 3, 0.5).generate(video[:5])
    inside = BatchedBeamSearch(mdl, 3, 0.5).generate(video)[:5]
    for (s1, lp1, sc1), (s2, lp2, sc2) in zip(alone, inside):
        assert s1 == s2
        assert _bytes(lp1) == _bytes(lp2) and _bytes(sc1) == _bytes(sc2)


# ------------------------------------------------------------------------------------------------ 5. surface
def test_build_generator_with_beam(gpu, oracle):
    import torch
    from s2vt_amd import model as M
    _, _, mdl, video, _ = _model(oracle, 24, 60, 20, 5, 7, 9, 3, scaled=True)
    with torch.no_grad():
        mdl.p["embed_word_b"][0] += 10.0
    assert mdl.n_caption_lstm_step == 7 and mdl.n_video_lstm_step == 5
    sess = M.Session(mdl)
    vp, words = mdl.build_generator(beam_size=3)                              # length_normalization_factor = 0.5
    got = sess.run(words, {vp: video})
    res = mdl.beam_search(video, 3, 0.5, batch_size=4)                        # chunks of 4, 4, 1
    want = np.zeros((9, 7), np.int64)
    for j, (s, _, _) in enumerate(res):
        want[j, :len(s)] = s
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert any(len(s) < 7 for s, _, _ in res)
    vp, words = mdl.build_generator()                                         # the default is the greedy fetch, as before
    ids, _ = gpu.attn_decode_greedy(mdl.dims, mdl.store.params, torch.as_tensor(video).cuda())
    assert np.array_equal(sess.run(words, {vp: video}), ids.cpu().numpy().astype(np.int64))


def _corpus(tmp_path, name, rng, n_videos=12, d=24, tv=3):
    vocab = ["<en_unk>", "a", "man", "woman", "dog", "cat", "is", "playing", "running", "eating", "the", "guitar", "ball", "food"]
    subj, verb, obj = ["man", "woman", "dog", "cat"], ["playing", "running", "eating"], ["guitar", "ball", "food"]
    feats, sents = str(tmp_path / f"{name}_feat.txt"), str(tmp_path / f"{name}_sents.txt")
    with open(feats, "w") as f, open(sents, "w") as g:
        for v in range(n_videos):
            s, vb, o = subj[v % 4], verb[(v // 4) % 3], obj[v % 3]
            base = np.zeros(d, np.float32); base[v % 4] = 2; base[4 + (v // 4) % 3] = 2; base[8 + v % 3] = 2
            for k in range(tv):
                x = np.abs(base + 0.05 * rng.standard_normal(d)).astype(np.float32)
                f.write(f"vid{v}_frame_{k}," + ",".join(f"{t:.6f}" for t in x) + "\n")
            for cap in (f"a {s} is {vb} the {o}", f"the {s} is {vb}", f"a {s} {vb} a {o}"):
                g.write(f"vid{v}\t{cap}\n")
    return sents, feats, vocab


def test_beam_eval_and_cli(gpu, tmp_path):
    import torch
    from s2vt_amd import attention as A
    from s2vt_amd import hostglue, reward, train_common as tc
    from s2vt_amd.beam_eval import read_captions
    rng = np.random.default_rng(0)
    sents, feats, vocab = _corpus(tmp_path, "test", rng)
    corpus = tc.Corpus(sents, feats, vocabulary=vocab)
    wordtoix, ixtoword = hostglue.preProBuildWordVocab(vocab)
    mdl = A.Attention_Caption_Generator(24, len(wordtoix), 32, 5, 3, 8, 0.9, seed=4)
    with torch.no_grad():
        mdl.p["embed_word_W"].mul_(10.0); mdl.p["lstm3_W"].mul_(4.0)
    scorer = reward.CiderD(corpus.index.refs_by_video(), wordtoix)
    greedy, g_cider = tc.greedy_eval(mdl, corpus, ixtoword, scorer, 5)
    beam1, b_cider = tc.beam_eval(mdl, corpus, ixtoword, scorer, 5, 1, 0.0)
    assert beam1 == greedy and abs(b_cider - g_cider) < 1e-6                     # beam 1 is greedy up to <eos>
    cfg = tc.Config(dim_image=24, lstm_dim=32, word_dim=32, n_video_lstm_step=3, n_caption_lstm_step=8, model_path=str(tmp_path / "m"),
                    model_name="a")
    ckpt = tc.save_checkpoint(mdl, cfg, 0, step_name="Variable")
    vocab_file = tmp_path / "vocab.txt"
    vocab_file.write_text("\n".join(vocab) + "\n")
    out = tmp_path / "beam3.txt"
    r = subprocess.run([sys.executable, "-m", "s2vt_amd.beam_eval", "--checkpoint", ckpt, "--test-sents", sents, "--test-feats", feats,
                        "--vocab", str(vocab_file), "--beam", "3", "--lnf", "0.5", "--batch-size", "5", "--n-caption-lstm-step", "8",
                        "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "CIDEr-D" in r.stdout
    lines = out.read_text().splitlines()
    got = read_captions(out)
    assert len(lines) == len(corpus.index.video_ids) and sorted(got) == sorted(corpus.index.video_ids)
    beam3, _ = tc.beam_eval(mdl, corpus, ixtoword, None, 5, 3, 0.5)
    for v in corpus.index.video_ids:
        assert got[v] == " ".join(w for w in beam3[v].split() if w not in ("<bos>", "<eos>"))
        assert "<eos>" not in got[v] and "<bos>" not in got[v]
