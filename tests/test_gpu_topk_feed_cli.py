"""train_xe --topk-feed on the tiny synthetic corpus of tests/test_gpu_train_drivers.py, then beam_eval --topk-feed on its checkpoint: the
driver takes topk_feed_update with the script's rule (sum_generate_words_tf_s2vt.py:429-435: SGD, clip_by_norm per variable, loss_weight
20, lr halved every 20000 steps), evaluates with that script's generator, and the flag combines with none of the other training rules."""
import json

import numpy as np
import pytest

from test_gpu_train_drivers import _corpus

pytestmark = pytest.mark.gpu


def test_driver_trains_and_evaluates_by_the_topk_rule(gpu, tmp_path, monkeypatch, capsys):
    from s2vt_amd import beam_eval, model as M, train_common as tcm, train_xe
    rng = np.random.default_rng(0)
    sents, feats, vocab = _corpus(tmp_path, "train", rng)
    corpus = tcm.Corpus(sents, feats, vocabulary=vocab)
    dims = dict(dim_image=24, lstm_dim=32, word_dim=16, n_video_lstm_step=3, n_caption_lstm_step=8)
    cfg = tcm.Config(n_epochs=2, batch_size=8, start_learning_rate=1e-2, decay_steps=3, model_path=str(tmp_path / "m"), model_name="topk",
                     step_log=str(tmp_path / "topk.jsonl"), **dims)
    calls, decodes = [], []
    plain, plain_gen = M.Video_Caption_Generator.topk_feed_update, M.Video_Caption_Generator.generate_topk_feed

    def spy(self, *a, **kw):
        calls.append((kw["k"], kw["clip"], kw["optimizer"], kw["clip_norm"]))
        return plain(self, *a, **kw)

    def spy_gen(self, *a, **kw):
        decodes.append(kw.get("k"))
        return plain_gen(self, *a, **kw)
    monkeypatch.setattr(M.Video_Caption_Generator, "topk_feed_update", spy)
    monkeypatch.setattr(M.Video_Caption_Generator, "generate_topk_feed", spy_gen)
    model, hist = train_xe.train(cfg, corpus, corpus, log=lambda *_: None, optimizer="sgd", topk_feed=5)
    steps = [r for r in map(json.loads, open(tmp_path / "topk.jsonl")) if r["kind"] == "step"]
    assert len(steps) == len(calls) > 3 and set(calls) == {(5, "per_variable", "sgd", 10.0)}
    assert model.loss_weight == 20 and model.adam_t == 0 and model.global_step == len(steps)
    assert all(np.isfinite(r["loss"]) for r in steps) and np.isfinite(hist[-1]["loss"])
    assert steps[-1]["lr"] == 1e-2 * 0.5 ** (len(steps) // 3) < steps[0]["lr"]          # the staircase on the model's step counter
    assert hist[-1]["loss"] < hist[0]["loss"]
    assert decodes and set(decodes) == {5} and hist[-1]["ciderD"] is not None            # the epoch's evaluation used the script's generator
    with pytest.raises(ValueError):
        train_xe.train(cfg, corpus, None, log=lambda *_: None, topk_feed=5, scheduled_sampling=0.5)
    with pytest.raises(ValueError):
        train_xe.train(cfg, corpus, None, log=lambda *_: None, topk_feed=5, averaged_embedding=True)

    # beam_eval --topk-feed on the checkpoint: greedy captions by the generator's rule, the ids generate_topk_feed gives
    decodes.clear()
    vocab_file = tmp_path / "vocab.txt"
    vocab_file.write_text("\n".join(vocab) + "\n")
    out = tmp_path / "caps.txt"
    rc = beam_eval.main(["--checkpoint", hist[-1]["checkpoint"], "--test-sents", sents, "--test-feats", feats, "--vocab", str(vocab_file),
                         "--n-caption-lstm-step", "8", "--batch-size", "8", "--out", str(out), "--topk-feed", "--topk-k", "5"])
    assert rc == 0 and decodes and set(decodes) == {5}
    assert "top-5 feed" in capsys.readouterr().out
    caps = beam_eval.read_captions(str(out))
    assert sorted(caps) == sorted(corpus.index.video_ids)
    from s2vt_amd import hostglue
    _, ixtoword = hostglue.preProBuildWordVocab(corpus.vocabulary)
    ids = plain_gen(model, corpus.features.batch(corpus.index.video_ids), k=5).cpu().numpy()
    for v, row in zip(corpus.index.video_ids, ids):
        assert caps[v] == beam_eval.caption_text(row, ixtoword), v
    assert gpu.chain_timeouts() == 0


@pytest.mark.parametrize("extra", [["--residual"], ["--scheduled-sampling", "0.5"], ["--ss-k", "5000"], ["--bidirectional"], ["--averaged-embedding"],
                                   ["--topk-k", "9"], ["--grad-precision", "bf16"]])
def test_flag_does_not_combine(gpu, extra):
    from s2vt_amd import train_xe
    with pytest.raises(SystemExit):
        train_xe.main(["--train-sents", "s", "--train-feats", "f", "--vocab", "v", "--topk-feed"] + extra)


def test_beam_eval_flag_is_for_plain_s2vt(gpu):
    from s2vt_amd import beam_eval
    for extra in (["--residual"], ["--model", "attention"], ["--topk-k", "0"]):
        with pytest.raises(SystemExit):
            beam_eval.main(["--checkpoint", "c", "--test-sents", "s", "--test-feats", "f", "--vocab", "v", "--topk-feed"] + extra)
