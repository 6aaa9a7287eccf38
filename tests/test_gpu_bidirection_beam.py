"""Batched beam search for the bidirectional captioner (s2vt_bidir_beam_*, ops.BidirBeamDecoder, BatchedBeamSearch over it,
bidirection_beam.Beam_Caption_Generator.beam_search / build_generator(beam_size), train_common.beam_eval, the beam_eval CLI).

1. the step's arithmetic, bit for bit against the CPU restatement's teacher-forced unroll of each hypothesis' video and word prefix
   (bidirection_cases.teacher_forced), along a hand-written row tree; its top-k against ops.vocab_topk; guard bands round its outputs;
2. beam 1 == the greedy decode;
3. the whole search, exact, against a per-video driver that teacher-forces every live prefix through the model's own
   teacher_forced_logits at B = 1 -- the same floats by 1., so sentences, logprob and score must agree to the byte -- on the sharpened
   case of tests/bidirection_beam_cases.py, which test_bidirection_beam_cases_cpu.py shows to discriminate;
4. a video decodes to the same bytes whatever batch it is in;
5. the class surface and both kinds of checkpoint;
6. train_common.beam_eval and the CLI."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import bidirection_beam_cases as C
import bidirection_cases as BC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bytes(x):
    return np.float64(x).tobytes()


def _generator(p, d, B, cls=None):
    from s2vt_amd import bidirection_beam
    cls = cls or bidirection_beam.Beam_Caption_Generator
    return cls(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, B, d.n_video_lstm_step + d.n_caption_lstm_step, d.n_video_lstm_step,
               d.n_caption_lstm_step, params=p)


_sharp = {}


def _sharpened(oracle):
    """(model, params, dims, video) of the sharpened case: one model for the tests that only read it"""
    if not _sharp:
        p, d, video = C.case(oracle)
        _sharp["m"] = (_generator(p, d, video.shape[0]), p, d, video)
    return _sharp["m"]


# ------------------------------------------------------------------------------------------------ 1. the step against the oracle
def _tree(B, V, rng):
    """(video, parent row of the previous step, word) per row and step.  B = 3: the hand-written tree; B = 5: 20 rows at step 1 (a second
    16-row tile), 17 at step 2."""
    w = lambda n: rng.integers(0, V, n).tolist()
    if B == 3:
        parents = [[9, 9, 9],                                    # step 0: one row per video; the parent is ignored, the word is <bos>
                   [2, 0, 1, 0, 2, 1, 2],                        # step 1: 2B + 1 rows, videos (= parents) mixed
                   [4, 1, 0, 3, 4, 6],                           # step 2: interleaved, video 1 absent, parent 4 twice
                   [3]]                                          # step 3: R = 1
    else:
        parents = [[9] * B, [(B - 1 - i) % B for i in range(4 * B)], [(7 * i + 3) % (4 * B) for i in range(16)] + [3], [11]]
    tree, vids = [], list(range(B))
    for t, par in enumerate(parents):
        vids = list(range(B)) if t == 0 else [vids[q] for q in par]
        tree.append((vids, par, [1] * len(par) if t == 0 else w(len(par))))
    return tree


@pytest.mark.parametrize("dims,B", [(BC.SHAPES["small-odd"][0], 3),                                                    # 16-byte path
                                    (dict(dim_image=40, n_words=97, word_dim=10, lstm_dim=18, n_video_lstm_step=4, n_caption_lstm_step=4), 3),   # scalar path: H % 4 != 0
                                    (BC.SHAPES["small-odd"][0], 5)])                                                    # R = 20 crosses a 16-row tile
def test_step_bit_exact_against_oracle(gpu, oracle, dims, B):
    import torch
    import s2vt_amd
    from guardband import Guarded
    ops = gpu
    L = s2vt_amd.lib()
    beam, k = 4, 3
    p, d, video = C.make(oracle, dims, B)
    V, Tc = d.n_words, d.n_caption_lstm_step
    m = _generator(p, d, B)
    tree = _tree(B, V, np.random.default_rng(7))
    if B == 3:
        assert 1 not in tree[2][0] and tree[2][1].count(4) == 2 and len(tree[3][0]) == 1
    else:
        assert len(tree[1][0]) == 20 and len(tree[2][0]) == 17
    dec = ops.BidirBeamDecoder(m._dims(), B, beam, m.device)
    vdev = torch.as_tensor(video).cuda()
    dec.encode(m.store.params, vdev)
    ref = {}

    def reference(vid, prefix):
        key = (vid, tuple(prefix))
        if key not in ref:
            cap = np.zeros((1, Tc), np.int32)
            cap[0, :len(prefix)] = prefix
            z = np.zeros(1, np.int32)
            ref[key] = BC.teacher_forced(oracle, p, d, np.ascontiguousarray(video[[vid]]), cap, z, z)[0]
        return ref[key]

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    prev = None
    for t, (vids, parents, words) in enumerate(tree):
        R = len(vids)
        rows = np.array([vids, parents, words], np.int32)
        prefixes = [[] if t == 0 else prev[parents[i]] + [words[i]] for i in range(R)]
        # the C entry on guarded outputs
        drows = torch.as_tensor(rows).cuda()
        gids = Guarded(R, k, dtype=torch.int32, name="top_ids")
        glp, glg = Guarded(R, k, name="top_logp"), Guarded(R, V, name="logits_out")
        rc = L.s2vt_bidir_beam_step(ctypes.byref(m._dims()), ctypes.byref(m.store.params), B, beam, t, R, ctypes.c_void_p(drows[0].data_ptr()),
                                    ctypes.c_void_p(drows[1].data_ptr()), ctypes.c_void_p(drows[2].data_ptr()), k, gids.ptr, glp.ptr, glg.ptr,
                                    ctypes.c_void_p(dec.ws.data_ptr()), dec.ws.numel(), stream)
        assert rc == 0
        lg = glg.numpy()
        for g in (gids, glp, glg):
            g.assert_intact()
        for i, (vid, prefix) in enumerate(zip(vids, prefixes)):
            assert np.array_equal(lg[i], reference(vid, prefix)[t]), (t, i)
        tid, tlp = ops.vocab_topk(glg.view.contiguous(), k)
        assert np.array_equal(gids.numpy(), tid.cpu().numpy())
        assert np.array_equal(glp.bits(), tlp.cpu().numpy().view(np.int32))
        # the same step again, through the decoder, on the workspace's own logits buffer: the same bits (the state it read is intact)
        ids2, lp2 = dec.step(m.store.params, t, rows, k)
        assert np.array_equal(ids2, gids.numpy()) and np.array_equal(lp2.view(np.int32), glp.bits())
        ids3, lp3, lg3 = dec.step(m.store.params, t, rows, k, want_logits=True)
        assert np.array_equal(lg3.cpu().numpy(), lg) and np.array_equal(ids3, ids2)
        prev = prefixes
    assert ops.chain_timeouts() == 0


def test_two_steps_where_the_encode_stage_is_persistent(gpu, oracle):
    """chain-range (H = 992, B = 16), beam 2: LSTM1 and LSTM2's encode steps take their persistent forms and hand slot Tv of the history to
    the gathered-state cell launch.  Reference: teacher_forced's first two decode steps (bidirection_beam_cases.first_steps)."""
    import torch
    p, d, video, *_ = BC.case(oracle, "chain-range")
    B, V = video.shape[0], d.n_words
    m = _generator(p, d, B)
    dec = gpu.BidirBeamDecoder(m._dims(), B, 2, m.device)
    dec.encode(m.store.params, torch.as_tensor(video).cuda())
    rng = np.random.default_rng(5)
    rows0 = np.array([np.arange(B), np.zeros(B), np.ones(B)], np.int32)
    vids = np.concatenate([np.arange(B), np.arange(B)[::-1]]).astype(np.int32)          # both hypotheses of a video; parents = videos
    words = rng.integers(2, V, 2 * B).astype(np.int32)
    ids0, lp0, lg0 = dec.step(m.store.params, 0, rows0, 3, want_logits=True)
    ids1, lp1, lg1 = dec.step(m.store.params, 1, np.array([vids, vids, words], np.int32), 3, want_logits=True)
    assert gpu.chain_timeouts() == 0
    lg0, lg1 = lg0.cpu().numpy(), lg1.cpu().numpy()
    for half in (0, 1):
        sl = slice(half * B, (half + 1) * B)
        cap = np.zeros((B, d.n_caption_lstm_step), np.int32)
        cap[vids[sl], 0] = words[sl]
        want = C.first_steps(oracle, p, d, video, cap, 2)
        if half == 0:
            assert np.array_equal(lg0, want[:, 0])
        assert np.array_equal(lg1[sl], want[vids[sl], 1]), half
    t1, l1 = gpu.vocab_topk(torch.as_tensor(lg1).cuda(), 3)
    assert np.array_equal(ids1, t1.cpu().numpy()) and np.array_equal(lp1.view(np.int32), l1.cpu().numpy().view(np.int32))


# ------------------------------------------------------------------------------------------------ 2. beam 1 == greedy
def _assert_beam1_is_greedy(m, video, batch_size=64):
    import torch
    Tc = m.n_caption_lstm_step
    ids = m.build_sampler(torch.as_tensor(video).cuda()).cpu().numpy()
    res = m.beam_search(video, 1, 0.0, batch_size)
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


def test_beam1_equals_greedy_sharpened(gpu, oracle):
    m, p, d, video = _sharpened(oracle)
    _assert_beam1_is_greedy(m, video)                                         # the greedy captions of the case run all Tc steps ...
    q = {n: a.copy() for n, a in p.items()}
    q["embed_word_b"][0] += np.float32(2.0)                                   # ... and with <eos> 2 further up (CPU restatement: 3 of 5 end at the second word)
    ended = _assert_beam1_is_greedy(_generator(q, d, video.shape[0]), video)
    assert 0 < ended < video.shape[0]


def test_beam1_equals_greedy_many_rows(gpu, oracle):
    p, d, video, *_ = BC.case(oracle, "many-rows")                            # B = 150 in one batch: steps of 150 rows, past the 96-row tile
    _assert_beam1_is_greedy(_generator(p, d, 150), video, 150)


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


_tf_rows = {}


def _teacher_forced_step(ops, m, video, j, k):
    """step(t, prefixes) through the existing unroll at B = 1: every live prefix teacher-forced (keep = 1), the logits of step t,
    vocab_topk.  The logits of a (video, prefix) are computed once and shared by the configurations."""
    import torch
    Tc, V = m.n_caption_lstm_step, m.n_words
    vj = torch.as_tensor(np.ascontiguousarray(video[j:j + 1])).cuda()

    def step(t, prefixes):
        rows = []
        for s in prefixes:
            key = (j, tuple(s))
            if key not in _tf_rows:
                cap = np.zeros((1, Tc), np.int32)
                cap[0, :len(s)] = s
                _tf_rows[key] = m.teacher_forced_logits(vj, torch.as_tensor(cap).cuda(), keep=1.0).view(Tc, V).clone()
            rows.append(_tf_rows[key][t])
        ids, lp = ops.vocab_topk(torch.stack(rows).contiguous(), k)
        return ids.cpu().numpy(), lp.cpu().numpy()
    return step


@pytest.mark.parametrize("lnf", [0.0, 0.7])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_search_equals_independent_driver(gpu, oracle, k, lnf):
    from s2vt_amd.beam_generator import BatchedBeamSearch
    m, p, d, video = _sharpened(oracle)
    Tc = d.n_caption_lstm_step
    res = BatchedBeamSearch(m, k, lnf).generate(video)
    early = full = 0
    for j in range(video.shape[0]):
        s, lp, sc = _per_video_search(_teacher_forced_step(gpu, m, video, j, k), Tc, k, lnf)
        bs, blp, bsc = res[j]
        assert bs == s, (k, lnf, j)
        assert _bytes(blp) == _bytes(lp) and _bytes(bsc) == _bytes(sc), (k, lnf, j)
        early += len(bs) < Tc
        full += len(bs) == Tc
    assert early > 0 and full > 0                                              # both exits of the loop are covered
    assert gpu.chain_timeouts() == 0


# ------------------------------------------------------------------------------------------------ 4. batch composition
def test_batch_composition_invariance(gpu, oracle):
    from s2vt_amd.beam_generator import BatchedBeamSearch
    m, p, d, video = _sharpened(oracle)
    for j in (1, 2):                                                           # one caption of all Tc steps, one that ends early
        alone = BatchedBeamSearch(m, 3, 0.7).generate(video[[j]])[0]
        first = BatchedBeamSearch(m, 3, 0.7).generate(video[[j, 0, 4]])[0]
        last = BatchedBeamSearch(m, 3, 0.7).generate(video[[0, 3, 4, (j + 1) % 3, 0, 3, j]])[6]
        for s, lp, sc in (first, last):
            assert s == alone[0]
            assert _bytes(lp) == _bytes(alone[1]) and _bytes(sc) == _bytes(alone[2])


# ------------------------------------------------------------------------------------------------ 5. surface
def test_class_surface_and_checkpoints(gpu, oracle, tmp_path):
    import torch
    from s2vt_amd import bidirection, bidirection_beam, bidirection_rl
    m, p, d, video = _sharpened(oracle)
    Tc, B = d.n_caption_lstm_step, video.shape[0]
    res = m.beam_search(video, 3, 0.0, batch_size=2)                           # chunks of 2, 2, 1
    assert any(len(s) < Tc for s, _, _ in res) and any(len(s) == Tc for s, _, _ in res)
    v0 = torch.as_tensor(video[2:3]).cuda()
    vid, sent, probs = m.build_generator(v0, beam_size=3)
    want = np.zeros(Tc, np.int32)
    want[:len(res[2][0])] = res[2][0]
    assert vid is v0 and probs == [] and sent.dtype == torch.int32 and np.array_equal(sent.cpu().numpy(), want)
    # without beam_size: the parent's graph, unchanged
    xe = _generator(p, d, B, bidirection.Video_Caption_Generator)
    _, greedy, _ = m.build_generator(v0)
    assert np.array_equal(greedy.cpu().numpy(), xe.build_generator(v0)[1].cpu().numpy())
    nodes = m.build_generator()
    assert len(nodes) == 3 and nodes[2] == []
    with pytest.raises(ValueError, match="no graph for beam search"):
        xe.beam_search(video)
    with pytest.raises(ValueError):
        m.build_generator(beam_size=3)                                         # a beam decode needs its video
    # an XE checkpoint and a REINFORCE checkpoint both load
    rl = _generator(p, d, B, bidirection_rl.Reinforce_Caption_Generator)
    xe.save(str(tmp_path / "xe"))
    rl.set_step(7)
    rl.save(str(tmp_path / "rl"))
    for path, step in ((tmp_path / "xe", 0), (tmp_path / "rl", 7)):
        fresh = bidirection_beam.Beam_Caption_Generator(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, B, d.n_video_lstm_step + Tc, d.n_video_lstm_step,
                                                        Tc, seed=99)
        assert not torch.equal(fresh.p["lstm2_W"], m.p["lstm2_W"])
        fresh.restore(str(path))
        assert all(torch.equal(fresh.p[n], m.p[n]) for n in bidirection.VARIABLES) and fresh.global_step == step
        got = fresh.beam_search(video, 3, 0.0)
        assert [g[0] for g in got] == [r[0] for r in res] and all(_bytes(g[1]) == _bytes(r[1]) for g, r in zip(got, res))


# ------------------------------------------------------------------------------------------------ 6. beam_eval and the CLI
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
    from s2vt_amd import beam_eval, bidirection_beam, hostglue, reward, train_common as tc
    from s2vt_amd.beam_eval import read_captions
    rng = np.random.default_rng(0)
    sents, feats, vocab = _corpus(tmp_path, "test", rng)
    corpus = tc.Corpus(sents, feats, vocabulary=vocab)
    wordtoix, ixtoword = hostglue.preProBuildWordVocab(vocab)
    mdl = bidirection_beam.Beam_Caption_Generator(24, len(wordtoix), 16, 32, 5, 11, 3, 8, seed=4)
    with torch.no_grad():
        mdl.p["embed_word_W"].mul_(10.0); mdl.p["lstm2_W"].mul_(4.0)
    scorer = reward.CiderD(corpus.index.refs_by_video(), wordtoix)
    greedy, g_cider = tc.greedy_eval(mdl, corpus, ixtoword, scorer, 5)
    beam1, b_cider = tc.beam_eval(mdl, corpus, ixtoword, scorer, 5, 1, 0.0)
    assert beam1 == greedy and abs(b_cider - g_cider) < 1e-6                     # beam 1 is greedy up to <eos>
    ckpt = str(tmp_path / "bidir-0")
    mdl.save(ckpt)
    vocab_file = tmp_path / "vocab.txt"
    vocab_file.write_text("\n".join(vocab) + "\n")
    beam3, _ = tc.beam_eval(mdl, corpus, ixtoword, None, 5, 3, 0.5)
    args = ["--checkpoint", ckpt, "--test-sents", sents, "--test-feats", feats, "--vocab", str(vocab_file), "--beam", "3", "--lnf", "0.5",
            "--batch-size", "5", "--n-caption-lstm-step", "8"]
    # auto-detection, as a user runs it; --model bidirectional in this process
    out = tmp_path / "beam3.txt"
    r = subprocess.run([sys.executable, "-m", "s2vt_amd.beam_eval"] + args + ["--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "CIDEr-D" in r.stdout
    out2 = tmp_path / "beam3_named.txt"
    assert beam_eval.main(args + ["--model", "bidirectional", "--out", str(out2)]) == 0
    assert out.read_text() == out2.read_text()
    got = read_captions(out)
    assert len(out.read_text().splitlines()) == len(corpus.index.video_ids) and sorted(got) == sorted(corpus.index.video_ids)
    for v in corpus.index.video_ids:
        assert got[v] == " ".join(w for w in beam3[v].split() if w not in ("<bos>", "<eos>"))
        assert "<eos>" not in got[v] and "<bos>" not in got[v]
