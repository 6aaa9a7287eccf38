"""`train_xe --bidirectional` / train_xe.train_bidirectional on the tiny synthetic corpus of tests/test_gpu_train_drivers.py: the script's
training rule (SGD, clip_by_norm per variable, the staircase decay) through the project's driver, a version-1 checkpoint per epoch under the
TF names, resuming from it, and the flag's refusal to combine with the other variants."""
import json

import numpy as np
import pytest

from test_gpu_train_drivers import _corpus

pytestmark = pytest.mark.gpu


def test_driver_trains_saves_and_resumes(gpu, tmp_path):
    from s2vt_amd import tfckpt, train_common as tc, train_xe
    rng = np.random.default_rng(0)
    sents, feats, vocab = _corpus(tmp_path, "train", rng)
    corpus = tc.Corpus(sents, feats, vocabulary=vocab)
    cfg = tc.Config(dim_image=24, lstm_dim=32, word_dim=16, n_video_lstm_step=3, n_caption_lstm_step=8, n_epochs=3, batch_size=8, start_learning_rate=0.01,
                    decay_steps=5, clip_norm=10.0, model_path=str(tmp_path / "m"), model_name="bimodel", step_log=str(tmp_path / "bi.jsonl"))
    lines = []
    model, hist = train_xe.train_bidirectional(cfg, corpus, log=lines.append)
    steps = [r for r in map(json.loads, open(tmp_path / "bi.jsonl")) if r["kind"] == "step"]
    per_epoch = (36 - 1) // 8                                                   # full batches only, as the reference walks them
    assert len(steps) == 3 * per_epoch and model.global_step == len(steps) and model.loss_weight == 20
    assert [r["lr"] for r in steps] == [0.01 * 0.5 ** (i // 5) for i in range(len(steps))]      # staircase on the step counter
    assert all(np.isfinite(r["loss"]) for r in steps) and hist[-1]["loss"] < hist[0]["loss"]
    assert len(hist) == 3 and any("Epoch 2 is done" in s for s in lines)
    sd = tfckpt.read_checkpoint(hist[-1]["checkpoint"])
    assert "s2vt/LSTM1/bidirectional_rnn/bw/basic_lstm_cell/weights" in sd and int(sd["Variable"]) == len(steps)
    assert np.array_equal(sd["s2vt/LSTM2/basic_lstm_cell/weights"], model.p["lstm2_W"].cpu().numpy())
    # resume: the variables and the step counter (hence the rate) come back
    cfg2 = tc.Config(**{**cfg.__dict__, "n_epochs": 1, "model_name": "bimodel_resumed", "step_log": str(tmp_path / "bi2.jsonl")})
    model2, hist2 = train_xe.train_bidirectional(cfg2, corpus, log=lambda *_: None, resume=hist[-1]["checkpoint"])
    steps2 = [r for r in map(json.loads, open(tmp_path / "bi2.jsonl")) if r["kind"] == "step"]
    assert steps2[0]["step"] == len(steps) + 1 and steps2[0]["lr"] == 0.01 * 0.5 ** (len(steps) // 5)
    assert gpu.chain_timeouts() == 0


@pytest.mark.parametrize("extra", [["--residual"], ["--scheduled-sampling", "0.5"], ["--optimizer", "sgd"], ["--grad-precision", "bf16"]])
def test_flag_does_not_combine(gpu, extra):
    from s2vt_amd import train_xe
    with pytest.raises(SystemExit):
        train_xe.main(["--train-sents", "s", "--train-feats", "f", "--vocab", "v", "--bidirectional"] + extra)
