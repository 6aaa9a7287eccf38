"""train_xe --averaged-embedding on the tiny synthetic corpus of tests/test_gpu_train_drivers.py: the driver takes averaged_update with the
script's rule (average_generate_words_tf_s2vt.py:358-371: SGD, clip_by_norm per variable, loss_weight 20, lr halved every 40000 steps), and
the flag combines with none of the other training rules."""
import json

import numpy as np
import pytest

from test_gpu_train_drivers import _corpus

pytestmark = pytest.mark.gpu


def test_driver_trains_by_the_averaged_rule(gpu, tmp_path, monkeypatch):
    from s2vt_amd import model as M, train_common as tc, train_xe
    rng = np.random.default_rng(0)
    sents, feats, vocab = _corpus(tmp_path, "train", rng)
    corpus = tc.Corpus(sents, feats, vocabulary=vocab)
    dims = dict(dim_image=24, lstm_dim=32, word_dim=16, n_video_lstm_step=3, n_caption_lstm_step=8)
    cfg = tc.Config(n_epochs=2, batch_size=8, start_learning_rate=1e-2, decay_steps=3, model_path=str(tmp_path / "m"), model_name="avg",
                    step_log=str(tmp_path / "avg.jsonl"), **dims)
    calls = []
    plain = M.Video_Caption_Generator.averaged_update

    def spy(self, *a, **kw):
        calls.append((kw["clip"], kw["optimizer"], kw["clip_norm"]))
        return plain(self, *a, **kw)
    monkeypatch.setattr(M.Video_Caption_Generator, "averaged_update", spy)
    model, hist = train_xe.train(cfg, corpus, None, log=lambda *_: None, optimizer="sgd", averaged_embedding=True)
    steps = [r for r in map(json.loads, open(tmp_path / "avg.jsonl")) if r["kind"] == "step"]
    assert len(steps) == len(calls) > 3 and set(calls) == {("per_variable", "sgd", 10.0)}
    assert model.loss_weight == 20 and model.adam_t == 0 and model.global_step == len(steps)
    assert all(np.isfinite(r["loss"]) for r in steps) and np.isfinite(hist[-1]["loss"])
    assert steps[-1]["lr"] == 1e-2 * 0.5 ** (len(steps) // 3) < steps[0]["lr"]          # the staircase on the model's step counter
    assert hist[-1]["loss"] < hist[0]["loss"]
    calls.clear()
    cfg2 = tc.Config(**{**cfg.__dict__, "n_epochs": 1, "model_name": "avg_adam", "step_log": ""})
    model2, _ = train_xe.train(cfg2, corpus, None, log=lambda *_: None, optimizer="adam", averaged_embedding=True)
    assert set(calls) == {("global", "adam", 10.0)} and model2.adam_t == len(calls)
    with pytest.raises(ValueError):
        train_xe.train(cfg2, corpus, None, log=lambda *_: None, averaged_embedding=True, scheduled_sampling=0.5)
    assert gpu.chain_timeouts() == 0


@pytest.mark.parametrize("extra", [["--residual"], ["--scheduled-sampling", "0.5"], ["--ss-k", "5000"], ["--bidirectional"]])
def test_flag_does_not_combine(gpu, extra):
    from s2vt_amd import train_xe
    with pytest.raises(SystemExit):
        train_xe.main(["--train-sents", "s", "--train-feats", "f", "--vocab", "v", "--averaged-embedding"] + extra)
