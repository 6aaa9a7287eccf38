"""The step of reinforce_multitask_e2e_attribute_by_groudtruth_greedy_s2vt.py -- the greedy caption is the policy's sample, the baseline is the
reward of a mixed decode (build_mix_sample: greedy, fed the ground-truth word with probability 0.9 / 1.00001) -- replayed through the drop-in
class (:825-858 the graphs, :957-979 the step) and run by the driver (train_rl, mix_baseline)."""
import json

import numpy as np
import pytest

from test_gpu_replay_multitask import B, _build, _twin_equal
from test_gpu_replay_train import _vocab
from test_gpu_sample_mix import _assert_mix_is_visible, _encode, _mix_decode
from test_gpu_train_drivers import _corpus

pytestmark = pytest.mark.gpu


def test_replay_groundtruth_greedy_step(gpu, oracle):
    from s2vt_amd.hostglue import decode_captions_masks, sentence_padding_toix
    from s2vt_amd.model import Session
    wordtoix, ixtoword = _vocab()
    lambda_loss, start_learning_rate = 0.3, 1e-3
    d, p, model, twin, feats, features_batch, _, _, rng = _build(oracle, 0, 0.2, seed=11)
    # a larger word embedding and no output bias: with the initialisers' scale the argmax of this small model is the same word whatever it
    # is fed, and the mixed caption could not be told from the greedy one
    p["Wemb"] = (p["Wemb"] * 8).astype(np.float32); p["embed_word_b"] = np.zeros_like(p["embed_word_b"])
    model.store.load(p); twin.store.load(p)
    Tc = d.n_caption_lstm_step
    video_batch = features_batch

    # ---- :825-858
    model_loss, model_features, model_captions, model_caption_masks, _ = model.build_model()
    sampled_captions, multinomial_video_features, mix_captions = model.build_mix_sample()        # 0.9 ground truth baseline (:828)
    greedy_captions, greedy_video_features = model.build_sampler()
    rewards = model.placeholder("rewards", [None])
    base_line = model.placeholder("base_line", [None])
    loss, loss_features, loss_captions, loss_masks = model.build_loss()
    sess = Session(model)
    learning_rate = model.exponential_decay(start_learning_rate, 300000, 0.5)
    train_op, sum_loss = model.multitask_train_op((loss, loss_features, loss_captions, loss_masks), rewards, base_line, learning_rate, clip_norm=5,
                                                  build_model_outputs=(model_loss, model_features, model_captions, model_caption_masks, _),
                                                  lambda_loss=lambda_loss)
    assert mix_captions.shape == (B, Tc)

    # ---- :950-962
    captions_batch = ["w1 w2 w3", "w7 notaword w9 w10 w11 w12 w13 w14 w15 w16", "w5 w40 w41 w42", "w200 w201 w202 w203 w204"]
    captions_ind, captions_mask = sentence_padding_toix(captions_batch, wordtoix, Tc)
    samples, greedy_words = sess.run([sampled_captions, greedy_captions], feed_dict={
        multinomial_video_features: video_batch, greedy_video_features: video_batch, mix_captions: captions_ind})
    assert samples.dtype == np.int64 and samples.shape == (B, Tc) == greedy_words.shape
    alone = sess.run(sampled_captions, feed_dict={multinomial_video_features: video_batch, mix_captions: captions_ind})
    assert alone.shape == (B, Tc)                                     # (fetched alone: the second run, fresh coins)
    gt = np.asarray(captions_ind, np.int32)
    seed1 = model.sample_seed + 7919
    ref_m, ref_g, coin, differs = _mix_decode(oracle, p, d, _encode(oracle, p, d, feats), gt, np.float32(0.9 / 1.00001), seed1)
    _assert_mix_is_visible(coin, differs)
    assert np.array_equal(samples, ref_m) and np.array_equal(greedy_words, ref_g) and not np.array_equal(samples, greedy_words)
    mask, multi_decoded = decode_captions_masks(samples, ixtoword)
    greedy_mask, greedy_decoded = decode_captions_masks(greedy_words, ixtoword)
    b = (rng.random(B) * 2).tolist()                                  # stand in for evaluate_captions_cider(ref_decoded, multi_decoded), :967
    r = (rng.random(B) * 2).tolist()                                  # ... (ref_decoded, greedy_decoded), :968

    # ---- :978-979: the update runs on the GREEDY ids with their own mask
    feed_dict = {loss_masks: greedy_mask, loss_captions: greedy_words, loss_features: video_batch, rewards: r, base_line: b,
                 model_features: video_batch, model_captions: captions_ind, model_caption_masks: captions_mask}
    _, loss_val = sess.run([train_op, sum_loss], feed_dict)
    assert np.isfinite(loss_val) and model.global_step == 1

    # ---- the direct calls on a second model
    mix, greedy = twin.mix_sample(feats, captions_ind, 0.9, True, seed=seed1)
    assert np.array_equal(mix.cpu().numpy(), samples) and np.array_equal(greedy.cpu().numpy(), greedy_words)
    st = twin.mixed_update(feats, greedy, np.asarray(greedy_mask, np.float32), np.asarray(r, np.float32), np.asarray(b, np.float32), captions_ind,
                           captions_mask, start_learning_rate, lambda_loss=lambda_loss, clip_norm=5.0, decay_all=True)
    assert abs(float(st.loss) + lambda_loss * _l2(p, model.decay_value) - loss_val) <= 1e-5 * max(1.0, abs(loss_val))
    _twin_equal(model, twin)
    assert gpu.chain_timeouts() == 0


def _l2(p, decay):
    """weight_decay_loss over every variable (the multitask scripts' predicate), pre-update: what sum_loss carries beside mixed_update's loss"""
    return decay * sum(0.5 * float((v.astype(np.float64) ** 2).sum()) for v in p.values())


def test_rl_driver_with_the_mixed_baseline(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from s2vt_amd import train_common as tc, train_rl
    rng = np.random.default_rng(0)
    sents, feats, vocab = _corpus(tmp_path, "train", rng, n_videos=8)
    corpus = tc.Corpus(sents, feats, vocabulary=vocab)
    quiet = lambda *_: None
    for lam, name in ((0.0, "pg"), (0.5, "mixed")):
        cfg = train_rl.rl_config(dim_image=24, lstm_dim=32, word_dim=16, n_video_lstm_step=3, n_caption_lstm_step=8, n_epochs=1, batch_size=8,
                                 multisample=1, start_learning_rate=1e-3, model_path=str(tmp_path / "m"), model_name=name, max_steps_per_epoch=2,
                                 mix_baseline=0.9, lambda_loss=lam, step_log=str(tmp_path / f"{name}.jsonl"))
        model, hist = train_rl.train(cfg, corpus, None, log=quiet)
        steps = [json.loads(l) for l in open(tmp_path / f"{name}.jsonl")]
        steps = [s for s in steps if s["kind"] == "step"]
        assert len(steps) == 2 == model.global_step
        assert all(np.isfinite(s["loss"]) and np.isfinite(s["reward"]) and np.isfinite(s["baseline"]) for s in steps)
        assert np.isfinite(hist[-1]["loss"])
    bad = train_rl.rl_config(dim_image=24, lstm_dim=32, word_dim=16, n_video_lstm_step=3, n_caption_lstm_step=8, n_epochs=1, batch_size=8,
                             multisample=2, model_path=str(tmp_path / "m"), mix_baseline=0.9)
    with pytest.raises(ValueError, match="must be 1"):
        train_rl.train(bad, corpus, None, log=quiet)
    from s2vt_amd import ops
    assert ops.chain_timeouts() == 0
