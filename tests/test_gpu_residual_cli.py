"""The residual flag through the callers, on the tiny synthetic corpus of tests/test_gpu_train_drivers.py: train_xe / train_rl with
Config(residual=True) build a residual model and write the flag into the epoch records of the JSONL step log; `beam_eval --residual` decodes a
checkpoint as the residual captioner."""
import json

import numpy as np
import pytest

from test_gpu_train_drivers import _corpus

pytestmark = pytest.mark.gpu


def test_drivers_and_beam_eval_carry_the_flag(gpu, tmp_path):
    from s2vt_amd import beam_eval, hostglue, train_common as tc, train_rl, train_xe
    from s2vt_amd.beam_eval import read_captions
    rng = np.random.default_rng(0)
    sents, feats, vocab = _corpus(tmp_path, "train", rng)
    corpus = tc.Corpus(sents, feats, vocabulary=vocab)
    dims = dict(dim_image=24, lstm_dim=32, word_dim=16, n_video_lstm_step=3, n_caption_lstm_step=8)
    quiet = lambda *_: None
    cfg = tc.Config(n_epochs=2, batch_size=8, start_learning_rate=2e-2, model_path=str(tmp_path / "m"), model_name="xe_res",
                    step_log=str(tmp_path / "xe.jsonl"), residual=True, **dims)
    model, hist = train_xe.train(cfg, corpus, corpus, log=quiet)
    assert model.residual and model.dims.reserved == 1 and np.isfinite(hist[-1]["loss"])
    epochs = [r for r in map(json.loads, open(tmp_path / "xe.jsonl")) if r["kind"] == "epoch"]
    assert len(epochs) == 2 and all(r["residual"] is True for r in epochs)
    with pytest.raises(ValueError, match="residual"):
        train_xe.train(cfg, corpus, None, log=quiet, scheduled_sampling=0.5)
    rl = train_rl.rl_config(n_epochs=1, batch_size=8, multisample=3, start_learning_rate=1e-3, model_path=str(tmp_path / "m"), model_name="rl_res",
                            step_log=str(tmp_path / "rl.jsonl"), residual=True, **dims)
    model2, hist2 = train_rl.train(rl, corpus, corpus, restore=hist[-1]["checkpoint"], log=quiet)
    assert model2.residual and np.isfinite(hist2[-1]["loss"])
    assert [r["residual"] for r in map(json.loads, open(tmp_path / "rl.jsonl")) if r["kind"] == "epoch"] == [True]
    plain_cfg = tc.Config(n_epochs=1, batch_size=8, model_path=str(tmp_path / "m"), model_name="xe_plain", step_log=str(tmp_path / "p.jsonl"), **dims)
    plain, _ = train_xe.train(plain_cfg, corpus, None, log=quiet)
    assert not plain.residual and [r["residual"] for r in map(json.loads, open(tmp_path / "p.jsonl")) if r["kind"] == "epoch"] == [False]

    # beam_eval --residual on the residual run's checkpoint: the captions of the residual model's own beam search, not the plain model's
    wordtoix, ixtoword = hostglue.preProBuildWordVocab(corpus.vocabulary)
    vocab_file = tmp_path / "vocab.txt"
    vocab_file.write_text("\n".join(vocab) + "\n")
    outs = {}
    for flag in ([], ["--residual"]):
        out = tmp_path / f"beam{len(flag)}.txt"
        rc = beam_eval.main(["--checkpoint", hist2[-1]["checkpoint"], "--test-sents", sents, "--test-feats", feats, "--vocab", str(vocab_file),
                             "--beam", "3", "--batch-size", "5", "--n-caption-lstm-step", "8", "--out", str(out)] + flag)
        assert rc == 0
        outs[len(flag)] = read_captions(out)
    want, _ = tc.beam_eval(model2, corpus, ixtoword, None, 5, 3, 0.0)
    for v in corpus.index.video_ids:
        assert outs[1][v] == " ".join(w for w in want[v].split() if w not in ("<bos>", "<eos>"))
    assert outs[0] != outs[1]
