"""The body of residual_tf_s2vt.py's train(), replayed through the drop-in class in the manner of tests/test_gpu_replay_train.py:
model (:410-419), build_model (:421), exponential_decay over 20000 steps + Adam + clip_by_global_norm 5 -> train_op (:429-435),
build_sampler (:454), two sess.run([train_op, tf_loss]) steps, then build_generator on one video (test(), :206-208 in its graph).
Every fetch is compared with the restatements of tests/residual_cases.py."""
import numpy as np
import pytest

import residual_cases as RC
from test_gpu_replay_train import _check_update

pytestmark = pytest.mark.gpu

B = 4


def test_replay_residual_train(gpu, oracle):
    import torch
    from s2vt_amd import hostglue, residual
    from s2vt_amd.model import Session
    from oracle import s2vt_torch as T
    p, d, video = RC.case(oracle, "one-tile")
    feats = video[:B]
    features_batch = [feats[j].tolist() for j in range(B)]
    Tc, V = d.n_caption_lstm_step, d.n_words
    vocabulary = ["<en_unk>"] + [f"w{i}" for i in range(V - 3)]
    wordtoix, ixtoword = hostglue.preProBuildWordVocab(vocabulary, word_count_threshold=0)
    assert len(wordtoix) == V
    start_learning_rate = 1e-3

    # ---- residual_tf_s2vt.py:410-435
    model = residual.Video_Caption_Generator(dim_image=d.dim_image, n_words=len(wordtoix), word_dim=d.word_dim, lstm_dim=d.lstm_dim, batch_size=B,
                                             n_lstm_steps=d.n_video_lstm_step + Tc, n_video_lstm_step=d.n_video_lstm_step,
                                             n_caption_lstm_step=Tc, bias_init_vector=None)
    model.store.load(p)
    tf_loss, tf_video, tf_caption, tf_caption_mask, tf_probs = model.build_model()
    sess = Session(model)
    learning_rate = model.exponential_decay(start_learning_rate, 20000, 0.5)
    train_op = model.minimize((tf_loss, tf_video, tf_caption, tf_caption_mask, tf_probs), learning_rate, clip_norm=5)
    greedy_captions, greedy_video_features = model.build_sampler()

    captions_batch = ["w1 w2 w3", "w7 notaword w9 w10 w11 w12 w13 w14 w15 w16 w17 w18 w19", "w5", "w200 w201 w202 w203 w204"]
    captions_ind, captions_mask = hostglue.sentence_padding_toix(captions_batch, wordtoix, Tc)
    cap32 = np.asarray(captions_ind, np.int32)
    m_arr = np.asarray(captions_mask, np.float32)
    vid = np.arange(B, dtype=np.int32); sid = np.zeros(B, np.int32)
    feed_dict = {tf_video: features_batch, tf_caption: captions_ind, tf_caption_mask: captions_mask}

    cur = p
    for step in range(2):
        dseed = model.dropout_seed + 104729 * model.global_step
        drop = oracle.dropout_masks(dseed, vid, sid, model.dropout_rate, d.lstm_dim, d.n_video_lstm_step, Tc)
        # forward-only fetches: the loss and the per-step logits of the summed output
        loss_fwd, probs = sess.run([tf_loss, tf_probs], feed_dict)
        ref_logits = RC.residual_teacher_forced(oracle, cur, d, feats, cap32, drop, model.dropout_rate)
        assert np.array_equal(np.transpose(probs, (1, 0, 2)), ref_logits), step
        assert not np.array_equal(ref_logits, RC.residual_teacher_forced(oracle, cur, d, feats, cap32, drop, model.dropout_rate, residual=False))
        ref_fwd = oracle.xe_loss(cur, d, ref_logits, cap32, m_arr, q1=True)
        assert abs(loss_fwd - ref_fwd) <= 1e-4 * max(1.0, abs(ref_fwd)), step
        pt = T.to_torch(cur, torch.float64, True)
        lg = RC.torch_teacher_forced(pt, feats, cap32, drop, model.dropout_rate)
        ref_loss = T.xe_loss(pt, lg, cap32, m_arr, q1=True)
        ref_loss.backward()
        _, loss_val = sess.run([train_op, tf_loss], feed_dict=feed_dict)
        assert abs(loss_val - float(ref_loss)) <= 1e-4 * max(1.0, abs(float(ref_loss))), step
        assert sess.run(learning_rate) == start_learning_rate and model.global_step == step + 1
        ref_g = {k: v.grad.numpy() for k, v in pt.items()}
        if step == 0:
            _check_update(model, cur, ref_g, start_learning_rate, 5.0)           # gradients, and the variables after clip + TF-Adam from zero slots
        else:
            for n in model.store.names:
                g = model.store.g[n].cpu().numpy().astype(np.float64)
                assert np.abs(g - ref_g[n]).max() <= 2e-4 * np.abs(ref_g[n]).max() + 1e-9, n
        cur = {n: model.store.p[n].cpu().numpy() for n in model.store.names}

    # ---- the greedy graph (:454) and build_generator on one video, on the trained weights
    g = sess.run(greedy_captions, feed_dict={greedy_video_features: features_batch})
    _, ref_g = RC.residual_sample(oracle, cur, d, feats, 0, 0)
    _, plain_g = RC.residual_sample(oracle, cur, d, feats, 0, 0, residual=False)
    assert np.array_equal(g, ref_g) and not np.array_equal(ref_g, plain_g)
    gen_video, sentence, _ = model.build_generator()
    words = sess.run(sentence, {gen_video: feats[:1]})
    assert [int(w) for w in words] == ref_g[0].tolist()
