"""ROUGE-L on the device (csrc/rouge.hip, s2vt_rouge_l_score through reward.RougeL.score_ids_device): bit-equal to the host library and to the
string restatement of tests/rouge_cases.py on the four cases (p and r included), deterministic, strided ids and guarded buffers, a loud NaN for
a video index outside the corpus, row counts on both sides of a wave boundary -- and the drivers end to end with reward="rouge"."""
import json

import numpy as np
import pytest

import rouge_cases as RC
from guardband import Guarded

pytestmark = pytest.mark.gpu


def _scorer(name, **kw):
    from s2vt_amd import reward
    c = RC.case(name)
    return c, reward.RougeL(c["refs_by_video"], c["wordtoix"], device="cuda", **kw)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("name", RC.CASES)
def test_device_equals_host_and_restatement_bit_for_bit(gpu, name):
    c, sc = _scorer(name)
    e = RC.expected(name)
    ids, vrow = _dev(c["ids"]), _dev(c["video_of_row"])
    out, pr = sc.score_ids_device(ids, vrow, want_pr=True)
    assert out.dtype.is_floating_point and tuple(out.shape) == (len(c["ids"]),) and tuple(pr.shape) == (len(c["ids"]), 2)
    assert np.array_equal(_bits(out), e["f32"].view(np.uint32))
    assert np.array_equal(_bits(out), sc.score_ids(c["ids"], c["video_of_row"]).view(np.uint32))
    assert np.array_equal(_bits(pr), e["pr"].view(np.uint64))
    again, pr2 = sc.score_ids_device(ids, vrow, want_pr=True)                   # two runs give equal bits
    assert np.array_equal(_bits(again), _bits(out)) and np.array_equal(_bits(pr2), _bits(pr))
    assert np.array_equal(_bits(sc.score_ids_device(ids, vrow)), _bits(out))     # without pr_out


def test_other_beta_on_the_device(gpu):
    c, sc = _scorer("ragged", beta=2.0)
    want = RC.score_rows(c, beta=2.0)[0].astype(np.float32)
    assert np.array_equal(_bits(sc.score_ids_device(_dev(c["ids"]), _dev(c["video_of_row"]))), want.view(np.uint32))


@pytest.mark.parametrize("name", ["ragged", "long"])
def test_strided_ids_and_guarded_outputs(gpu, name):
    import torch
    from s2vt_amd import ops
    c, sc = _scorer(name)
    e = RC.expected(name)
    N, Tc = c["ids"].shape
    ids = Guarded.of(c["ids"], ld=Tc + 3, dtype=torch.int32, lead=65, name="ids")          # a view into a wider buffer, 4-byte aligned only
    vrow = Guarded.of(c["video_of_row"], dtype=torch.int32, fill=0, name="video_of_row")
    out = Guarded(1, N, dtype=torch.float32, lead=67, name="out")
    pr = Guarded(N, 2, dtype=torch.float64, lead=65, name="pr_out")
    assert ids.view.stride(0) == Tc + 3
    toks, offs, video_refs, n_refs = sc._dev
    ops.rouge_l_score(toks, offs, video_refs, n_refs, ids.view, vrow.view.reshape(-1), sc.beta2, out=out.view.reshape(-1), pr_out=pr.view, want_pr=True)
    torch.cuda.synchronize()
    assert np.array_equal(out.bits().reshape(-1).view(np.uint32), e["f32"].view(np.uint32))
    assert np.array_equal(pr.bits().view(np.uint64), e["pr"].view(np.uint64))
    for g in (ids, vrow, out, pr):
        g.assert_intact()


def test_video_out_of_range_is_nan_in_that_row_only(gpu):
    c, sc = _scorer("ragged")
    e = RC.expected("ragged")
    v = c["video_of_row"].copy()
    v[7], v[64], v[129] = -1, len(c["refs_by_video"]), 2 ** 31 - 1
    out, pr = sc.score_ids_device(_dev(c["ids"]), _dev(v), want_pr=True)
    got, gpr = out.cpu().numpy(), pr.cpu().numpy()
    bad = np.zeros(len(v), bool)
    bad[[7, 64, 129]] = True
    assert np.isnan(got[bad]).all() and np.isnan(gpr[bad]).all()
    assert np.array_equal(got[~bad].view(np.uint32), e["f32"][~bad].view(np.uint32))
    assert np.array_equal(gpr[~bad].view(np.uint64), e["pr"][~bad].view(np.uint64))


@pytest.mark.parametrize("rows", [1, 3, 64, 65])
def test_row_counts_cut_from_the_same_case(gpu, rows):
    c, sc = _scorer("ragged")
    e = RC.expected("ragged")
    out = sc.score_ids_device(_dev(c["ids"][:rows]), _dev(c["video_of_row"][:rows]))
    assert tuple(out.shape) == (rows,) and np.array_equal(_bits(out), e["f32"][:rows].view(np.uint32))


def test_no_rows(gpu):
    import torch
    c, sc = _scorer("tiny")
    out = sc.score_ids_device(torch.empty((0, 4), dtype=torch.int32, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda"))
    assert tuple(out.shape) == (0,)


# ------------------------------------------------------------------------------------------------------------------------ drivers
def _record_samples(model, K):
    """Wrap model.sample so that every training call (K samples + greedy) leaves its ids on the host."""
    seen, inner = [], model.sample

    def sample(video, k=0, *a, **kw):
        s, g = inner(video, k, *a, **kw)
        if k == K:
            seen.append((s.cpu().numpy().copy(), g.cpu().numpy().copy()))
        return s, g
    model.sample = sample
    return seen


def _mean_tol(n):
    """Two float32 means of n values in [0, 1] summed in different orders: each partial sum <= n carries at most 2^-24 n of rounding, n - 1
    additions, then the division by n -- (n - 1) 2^-24 per mean, and the quotient's own half ulp."""
    return 2.0 * n * 2.0 ** -24


def test_train_rl_with_rouge_end_to_end(gpu, tmp_path):
    from test_gpu_train_drivers import _corpus
    from s2vt_amd import hostglue, model as M, reward, train_common as tc, train_rl
    rng = np.random.default_rng(0)
    sents, feats, vocab = _corpus(tmp_path, "train", rng)
    corpus = tc.Corpus(sents, feats, vocabulary=vocab)
    K, B = 3, 8
    cfg = train_rl.rl_config(dim_image=24, lstm_dim=32, word_dim=16, n_video_lstm_step=3, n_caption_lstm_step=8, n_epochs=1, batch_size=B, multisample=K,
                             start_learning_rate=1e-3, max_steps_per_epoch=3, model_path=str(tmp_path / "m"), model_name="rlrouge",
                             step_log=str(tmp_path / "rl.jsonl"), reward="rouge")
    wordtoix, _ = hostglue.preProBuildWordVocab(corpus.vocabulary)
    model = M.Video_Caption_Generator(24, len(wordtoix), 16, 32, B, 11, 3, 8, bias_init_vector=None, seed=cfg.seed, multisample=K, device="cuda:0")
    seen = _record_samples(model, K)
    model, hist = train_rl.train(cfg, corpus, corpus, model=model, log=lambda *_: None)
    recs = [json.loads(l) for l in open(tmp_path / "rl.jsonl")]
    steps = [r for r in recs if r["kind"] == "step"]
    assert len(steps) == 3 == len(seen) and all(np.isfinite(r["loss"]) for r in steps) and np.isfinite(hist[-1]["loss"])
    # the logged means are the host scorer's on the very ids of the step: the batches are re-drawn as the driver draws them
    import random
    host = reward.RougeL(corpus.index.refs_by_video(), wordtoix)
    batches = list(tc.epoch_batches(len(corpus.captions), B, random.Random(cfg.seed)))[:3]
    for rec, (s_ids, g_ids), idx in zip(steps, seen, batches):
        rows = np.asarray([corpus.index.row[v] for v in corpus.captions[idx, 0]], np.int32)
        r, b = host.score_ids(s_ids, np.tile(rows, K)), host.score_ids(g_ids, rows)
        assert abs(rec["reward"] - float(r.astype(np.float64).mean())) <= _mean_tol(len(r)), (rec, r)
        assert abs(rec["baseline"] - float(b.astype(np.float64).mean())) <= _mean_tol(len(b)), (rec, b)
    epoch = [r for r in recs if r["kind"] == "epoch"]
    assert len(epoch) == 1 and "rougeL" in epoch[0] and "ciderD" not in epoch[0] and 0.0 <= epoch[0]["rougeL"] <= 1.0
    assert "rougeL" in hist[-1] and "ciderD" not in hist[-1]
    assert gpu.chain_timeouts() == 0


def test_default_reward_keeps_its_keys(gpu, tmp_path):
    from test_gpu_train_drivers import _corpus
    from s2vt_amd import train_common as tc, train_rl
    sents, feats, vocab = _corpus(tmp_path, "train", np.random.default_rng(0))
    corpus = tc.Corpus(sents, feats, vocabulary=vocab)
    cfg = train_rl.rl_config(dim_image=24, lstm_dim=32, word_dim=16, n_video_lstm_step=3, n_caption_lstm_step=8, n_epochs=1, batch_size=8, multisample=2,
                             start_learning_rate=1e-3, max_steps_per_epoch=1, model_path=str(tmp_path / "m"), model_name="rlcider", step_log=str(tmp_path / "c.jsonl"))
    assert cfg.reward == "cider"
    _, hist = train_rl.train(cfg, corpus, corpus, log=lambda *_: None)
    recs = [json.loads(l) for l in open(tmp_path / "c.jsonl")]
    assert "ciderD" in hist[-1] and "rougeL" not in hist[-1] and all("reward" in r and "baseline" in r for r in recs if r["kind"] == "step")


@pytest.mark.parametrize("mode", ["multitask", "mixed", "mix_baseline"])
def test_train_rl_modes_with_rouge(gpu, tmp_path, mode):
    from test_gpu_train_drivers import _corpus
    from s2vt_amd import train_common as tc, train_rl
    sents, feats, vocab = _corpus(tmp_path, "train", np.random.default_rng(0))
    corpus = tc.Corpus(sents, feats, vocabulary=vocab)
    kw = dict(multitask=dict(multisample=2), mixed=dict(multisample=2, lambda_loss=0.5), mix_baseline=dict(multisample=1, mix_baseline=0.9))[mode]
    cfg = train_rl.rl_config(dim_image=24, lstm_dim=32, word_dim=16, n_video_lstm_step=3, n_caption_lstm_step=8, n_epochs=1, batch_size=8,
                             start_learning_rate=1e-3, max_steps_per_epoch=1, model_path=str(tmp_path / "m"), model_name=mode, reward="rouge",
                             step_log=str(tmp_path / "s.jsonl"), **kw)
    attrs = None if mode == "mix_baseline" else ["man", "woman", "dog", "cat"]
    model, hist = train_rl.train(cfg, corpus, corpus, log=lambda *_: None, attr_vocabulary=attrs)
    step = [json.loads(l) for l in open(tmp_path / "s.jsonl")][0]
    assert model.global_step == 1 and np.isfinite(hist[-1]["loss"]) and "rougeL" in hist[-1] and "ciderD" not in hist[-1]
    assert 0.0 <= step["reward"] <= 1.0 and 0.0 <= step["baseline"] <= 1.0


def test_bidirectional_and_attention_one_step_with_rouge(gpu, tmp_path):
    from test_gpu_train_drivers import _corpus
    from s2vt_amd import train_attention, train_common as tc, train_rl
    sents, feats, vocab = _corpus(tmp_path, "train", np.random.default_rng(0), n_videos=8)
    corpus = tc.Corpus(sents, feats, vocabulary=vocab)
    cfg = train_rl.rl_config(dim_image=24, lstm_dim=32, word_dim=16, n_video_lstm_step=3, n_caption_lstm_step=8, n_epochs=1, batch_size=4, multisample=2,
                             start_learning_rate=1e-3, max_steps_per_epoch=1, model_path=str(tmp_path / "b"), model_name="bi", reward="rouge",
                             step_log=str(tmp_path / "bi.jsonl"))
    model, hist = train_rl.train_bidirectional(cfg, corpus, corpus, log=lambda *_: None)
    step = [json.loads(l) for l in open(tmp_path / "bi.jsonl")][0]
    assert model.global_step == 1 and np.isfinite(step["loss"]) and 0.0 <= step["reward"] <= 1.0 and "rougeL" in hist[-1] and "ciderD" not in hist[-1]
    acfg = train_attention.reinforce_config(dim_image=24, lstm_dim=32, n_video_lstm_step=3, n_caption_lstm_step=8, n_epochs=1, batch_size=4,
                                            max_steps_per_epoch=1, start_learning_rate=1e-3, model_path=str(tmp_path / "a"), model_name="att",
                                            step_log=str(tmp_path / "att.jsonl"), reward="rouge")
    amodel, ahist = train_attention.train(acfg, corpus, corpus, log=lambda *_: None, reinforce=True, samples=2)
    astep = [json.loads(l) for l in open(tmp_path / "att.jsonl")][0]
    assert amodel.global_step == 1 and np.isfinite(astep["loss"]) and 0.0 <= astep["reward"] <= 1.0 and 0.0 <= astep["baseline"] <= 1.0
    assert "rougeL" in ahist[-1] and "ciderD" not in ahist[-1]
    assert gpu.chain_timeouts() == 0


def test_e2e_reinforce_one_step_with_rouge(gpu, tmp_path):
    import os
    import torch
    from PIL import Image
    from s2vt_amd import data, train_e2e
    rng = np.random.default_rng(1)
    vocab = ["<en_unk>", "a", "red", "green", "blue", "square", "is", "shown"]
    colours = {"red": (220, 30, 30), "green": (30, 220, 30), "blue": (30, 30, 220)}
    sent = tmp_path / "sents.txt"
    with open(sent, "w") as f:
        for v in range(6):
            name = list(colours)[v % 3]
            os.makedirs(tmp_path / "frames" / f"vid{v}")
            for k in range(1, 4):
                img = np.clip(np.asarray(colours[name])[None, None, :] + rng.integers(-20, 20, (24, 24, 3)), 0, 255).astype(np.uint8)
                Image.fromarray(img).save(tmp_path / "frames" / f"vid{v}" / f"{k:06d}.jpg")
            f.write(f"vid{v}\ta {name} square is shown\nvid{v}\ta {name} square\n")
    sents, frames = data.get_video_frame_caption_pair(str(sent), str(tmp_path / "frames"), 3)
    torch.manual_seed(0)
    cnn = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, stride=2), torch.nn.ReLU(), torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(),
                              torch.nn.Linear(8, 24), torch.nn.ReLU())
    cfg = train_e2e.e2e_config(dim_image=24, lstm_dim=32, word_dim=16, n_video_lstm_step=3, n_caption_lstm_step=8, n_epochs=1, batch_size=4, multisample=2,
                               max_steps_per_epoch=1, start_learning_rate=1e-3, model_path=str(tmp_path / "m"), model_name="e2e_rouge", reward="rouge")
    trainer, hist = train_e2e.train_reinforce(cfg, sents, frames, vocab, cnn=cnn, width=24, height=24, log=lambda *_: None, test=(sents, frames))
    assert trainer.model.global_step == 1 and np.isfinite(hist[-1]["loss"]) and np.isfinite(hist[-1]["advantage"])
    assert "rougeL" in hist[-1] and "ciderD" not in hist[-1] and 0.0 <= hist[-1]["rougeL"] <= 1.0


def test_unknown_reward_is_refused(gpu):
    from s2vt_amd import train_attention, train_e2e, train_rl
    base = ["--train-sents", "s", "--train-feats", "f", "--vocab", "v"]
    with pytest.raises(SystemExit):
        train_rl.main(base + ["--reward", "bleu"])
    with pytest.raises(SystemExit):
        train_rl.main(base + ["--bidirectional", "--reward", "bleu"])
    with pytest.raises(SystemExit):
        train_attention.main(base + ["--reinforce", "--reward", "bleu"])
    with pytest.raises(SystemExit):
        train_e2e.main(["--train-sents", "s", "--frames", "f", "--vocab", "v", "--reinforce", "--reward", "bleu"])
