"""Batched beam search (ops.vocab_topk, ops.BeamDecoder, beam_generator.BatchedBeamSearch, model.beam_search, train_common.beam_eval,
the beam_eval CLI): the top-k kernel against numpy and, bit for bit, against the softmax kernel's log-normaliser; the batched path
against the reference-pinned fixture and against the per-video BeamSearchGenerator it restates."""
import json
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "beam_search.json")
W_SCALE, LSTM_SCALE, WEMB_SCALE = 30.0, 6.0, 20.0           # tools/make_beam_fixtures.py


def _close(a, b):
    return abs(a - b) <= 2e-4 * max(1.0, abs(b))


# ---------------------------------------------------------------------------------------------------------------- 1. vocab_topk
def _rows(rng, R, V):
    l = (rng.standard_normal((R, V)) * 3).astype(np.float32)
    if R >= 7:
        l[1, :] = 0.5                                            # every value equal: ids 0..k-1
        l[2, [3, V // 2, V - 1]] = 20.0                          # a three-way tie at the top
        top = np.sort(l[3])[::-1]
        l[3, [5, V // 3, V - 2]] = top[3]                        # ties straddling places 4..6 (k = 5 cuts through them)
        l[4, :V // 2] = 1.0; l[4, V // 2:] = 2.0                 # two plateaus
        l[5, [0, 1]] = 50.0                                      # adjacent tie at the very top
    return l


@pytest.mark.parametrize("R", [1, 7, 320])
@pytest.mark.parametrize("V", [60, 9972, 12000, 12001])
def test_vocab_topk_against_numpy(gpu, R, V):
    import torch
    ops = gpu
    rng = np.random.default_rng(R * 100003 + V)
    l = _rows(rng, R, V)
    lp64 = l.astype(np.float64) - (np.log(np.exp(l.astype(np.float64) - l.max(1, keepdims=True)).sum(1, keepdims=True)) + l.max(1, keepdims=True))
    order = np.argsort(-l, axis=1, kind="stable")                   # value descending, index ascending on ties
    for r in range(min(R, 8)):
        assert np.array_equal(order[r, :16], np.lexsort((np.arange(V), -l[r]))[:16])
    ld4 = ((V + 3) // 4) * 4 + 8
    layouts = [(V, 0), (V + 5, 0), (ld4, 0), (ld4, 1)]      # ld == V; ld > V (odd); ld > V, ld % 4 == 0 (float4s + tail when V % 4);
                                                             # the same with a misaligned row pointer (scalar path)
    for ld, off in layouts:
        host = np.zeros(R * ld + off + 4, np.float32)
        host[off:off + R * ld].reshape(R, ld)[:, :V] = l
        buf = torch.as_tensor(host).cuda()
        view = buf[off:off + R * ld].view(R, ld)[:, :V]
        for k in (1, 2, 3, 5, 8, 16):
            ids, lp = ops.vocab_topk(view, k)
            ids, lp = ids.cpu().numpy(), lp.cpu().numpy()
            assert np.array_equal(ids, order[:, :k]), (ld, off, k)
            assert np.allclose(lp, np.take_along_axis(lp64, ids.astype(np.int64), 1), rtol=0, atol=1e-5)
            for j in range(k):                                       # bit for bit: the softmax kernel's lp of that target
                cp = buf.clone()
                cv = cp[off:off + R * ld].view(R, ld)[:, :V]
                _, lpt = ops.softmax_nll_fwd_bwd(cv, torch.as_tensor(ids[:, j].copy()).cuda(), torch.zeros(R, device="cuda"), 0.0)
                assert np.array_equal(lpt.cpu().numpy().view(np.uint32), lp[:, j].copy().view(np.uint32)), (ld, off, k, j)
        if R >= 7:
            assert ids[1].tolist() == list(range(16))


# ---------------------------------------------------------------------------------------------------------------- 2. golden fixture
def test_batched_matches_reference_fixture(gpu, oracle):
    from s2vt_amd import model as M
    from s2vt_amd.beam_generator import BatchedBeamSearch
    gold = json.load(open(GOLD))
    dm = gold["dims"]
    d = oracle.Dims(label_dim=0, **dm)
    groups = OrderedDict()
    for c in gold["cases"]:
        groups.setdefault((c["param_seed"], c["beam_size"], c["length_normalization_factor"]), []).append(c)
    assert len(groups) == 12 and all(len(g) == 3 for g in groups.values())
    models, finished, full = {}, 0, 0
    for (ps, k, lnf), cases in groups.items():
        if ps not in models:
            p = oracle.init_params(d, seed=ps)
            p["embed_word_W"] *= np.float32(gold["scales"]["embed_word_W"])
            p["lstm1_W"] *= np.float32(gold["scales"]["lstm_W"]); p["lstm2_W"] *= np.float32(gold["scales"]["lstm_W"])
            p["Wemb"] *= np.float32(gold["scales"]["Wemb"])
            p["embed_word_b"][0] += np.float32(gold["eos_bias"][str(ps)])
            mdl = M.Video_Caption_Generator(dm["dim_image"], dm["n_words"], dm["word_dim"], dm["lstm_dim"], 1, 0,
                                            dm["n_video_lstm_step"], dm["n_caption_lstm_step"])
            mdl.store.load(p)
            models[ps] = mdl
        video = np.stack([np.asarray(c["video"], np.float32).reshape(dm["n_video_lstm_step"], dm["dim_image"]) for c in cases])
        res = BatchedBeamSearch(models[ps], k, lnf).generate(video)            # the group's 3 videos in ONE call
        for c, (s, lp, sc) in zip(cases, res):
            assert s == c["sentence"], (ps, k, lnf)
            assert _close(lp, c["logprob"]) and _close(sc, c["score"]), (ps, k, lnf)
            finished += s[-1] == 0
            full += len(s) == dm["n_caption_lstm_step"] and s[-1] != 0
    assert finished > 0 and full > 0                                             # both exits of the loop are covered


# ---------------------------------------------------------------------------------------------------------------- 3./4. realistic dims
_BIG = {}


def _big_model():
    """BASELINE configs[2] dimensions, weights scaled as tools/make_beam_fixtures.py scales them."""
    if "m" not in _BIG:
        import torch
        from s2vt_amd import model as M
        mdl = M.Video_Caption_Generator(1536, 12000, 500, 1000, 16, 0, 5, 20, seed=11)
        p = mdl.store.p
        with torch.no_grad():
            p["embed_word_W"].mul_(W_SCALE); p["lstm1_W"].mul_(LSTM_SCALE); p["lstm2_W"].mul_(LSTM_SCALE); p["Wemb"].mul_(WEMB_SCALE)
        rng = np.random.default_rng(5)
        scale = np.linspace(0.2, 2.0, 16, dtype=np.float32)[:, None, None]        # videos of different strength: different beams
        video = (np.abs(rng.standard_normal((16, 5, 1536))) * scale).astype(np.float32)
        _BIG["m"], _BIG["v"] = mdl, video
    return _BIG["m"], _BIG["v"]


def test_batched_equals_per_video_configs2(gpu):
    import torch
    from s2vt_amd.beam_generator import BatchedBeamSearch, BeamSearchGenerator
    mdl, video = _big_model()
    Tc = mdl.n_caption_lstm_step
    b0 = float(mdl.store.p["embed_word_b"][0])
    early = full = 0
    for eos in (0.0, 10.0, 20.0, 40.0, 80.0):                    # <eos> bias: until captions of both kinds have been seen
        with torch.no_grad():
            mdl.store.p["embed_word_b"][0] = b0 + eos
        for k in (3, 5):
            for lnf in (0.0, 0.5):
                res = BatchedBeamSearch(mdl, k, lnf).generate(video)
                for j in range(video.shape[0]):
                    s, lp, sc = BeamSearchGenerator(mdl, k, lnf).generate(video[j:j + 1])
                    bs, blp, bsc = res[j]
                    assert bs == s, (eos, k, lnf, j)
                    assert _close(blp, lp) and _close(bsc, sc), (eos, k, lnf, j)
                    early += len(bs) < Tc
                    full += len(bs) == Tc
        if early and full:
            break
    with torch.no_grad():
        mdl.store.p["embed_word_b"][0] = b0
    assert early > 0 and full > 0


def test_batch_composition_invariance(gpu):
    from s2vt_amd.beam_generator import BatchedBeamSearch
    mdl, video = _big_model()
    for k in (3, 5):
        gen = BatchedBeamSearch(mdl, k, 0.5)
        alone = gen.generate(video[:5])
        inside = BatchedBeamSearch(mdl, k, 0.5).generate(video)[:5]
        for (s1, lp1, sc1), (s2, lp2, sc2) in zip(alone, inside):
            assert s1 == s2
            assert np.float64(lp1).tobytes() == np.float64(lp2).tobytes() and np.float64(sc1).tobytes() == np.float64(sc2).tobytes()


# ---------------------------------------------------------------------------------------------------------------- 5. model surface
def test_model_beam_search_equals_build_generator(gpu):
    import torch
    from s2vt_amd import model as M
    mdl = M.Video_Caption_Generator(24, 60, 12, 20, 1, 0, 3, 7, seed=3)
    with torch.no_grad():
        mdl.store.p["embed_word_W"].mul_(W_SCALE); mdl.store.p["lstm2_W"].mul_(LSTM_SCALE)
        mdl.store.p["embed_word_b"][0] += 3.0
    rng = np.random.default_rng(2)
    videos = np.abs(rng.standard_normal((9, 3, 24))).astype(np.float32)
    sess = M.Session(mdl)
    for k, lnf in ((1, 0.0), (3, 0.0), (4, 0.5)):
        got = mdl.beam_search(videos, k, lnf, batch_size=4)                       # chunks of 4, 4, 1
        assert len(got) == 9
        vp, sent, _ = mdl.build_generator(beam_size=k, length_normalization_factor=lnf)
        for j in range(9):
            ref = sess.run(sent, {vp: videos[j:j + 1]})
            ids = [0] * 7
            ids[:len(got[j][0])] = got[j][0]
            if k > 1:
                assert ids == [int(w) for w in ref], (k, lnf, j)
            else:                                                                 # beam 1 == greedy up to its <eos>
                assert got[j][0] == [int(w) for w in ref][:len(got[j][0])], (k, j)


# ---------------------------------------------------------------------------------------------------------------- 6. evaluation
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
    from s2vt_amd import hostglue, reward, train_common as tc
    from s2vt_amd import model as M
    from s2vt_amd.beam_eval import read_captions
    rng = np.random.default_rng(0)
    sents, feats, vocab = _corpus(tmp_path, "test", rng)
    corpus = tc.Corpus(sents, feats, vocabulary=vocab)
    wordtoix, ixtoword = hostglue.preProBuildWordVocab(vocab)
    mdl = M.Video_Caption_Generator(24, len(wordtoix), 16, 32, 5, 11, 3, 8, seed=4)
    with torch.no_grad():
        mdl.store.p["embed_word_W"].mul_(10.0); mdl.store.p["lstm2_W"].mul_(4.0)
    scorer = reward.CiderD(corpus.index.refs_by_video(), wordtoix)
    greedy, g_cider = tc.greedy_eval(mdl, corpus, ixtoword, scorer, 5)
    beam1, b_cider = tc.beam_eval(mdl, corpus, ixtoword, scorer, 5, 1, 0.0)
    assert beam1 == greedy and abs(b_cider - g_cider) < 1e-6                     # beam 1 is greedy up to <eos>
    cfg = tc.Config(dim_image=24, lstm_dim=32, word_dim=16, n_video_lstm_step=3, n_caption_lstm_step=8, model_path=str(tmp_path / "m"),
                    model_name="b")
    ckpt = tc.save_checkpoint(mdl, cfg, 0)
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
