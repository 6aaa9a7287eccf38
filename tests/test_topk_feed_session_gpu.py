"""The top-k feed script through the drop-in class's Session, beside tests/test_gpu_replay_topk_feed.py: its train() (sum_generate_words_tf_s2vt.py
:429-435) replayed at the script's own loss_weight of 20, and build_generator(topk_feed=k) (:221-275) fetched word by word."""
import numpy as np
import pytest

import topk_feed_cases as tc

pytestmark = pytest.mark.gpu

NAME = "small-odd"


def test_replay_at_the_scripts_loss_weight(gpu, oracle):
    """tests/test_gpu_replay_topk_feed.py's replay at loss_weight 20, the script's (that file takes 60, so that the clip acts).  At this
    case's size the largest per-variable norm is then 4.4 (float64 autograd, embed_word_b): the clip of 10 acts on no variable."""
    loss_weight = 20
    import torch
    from s2vt_amd import model as M
    from s2vt_amd.model import Session
    dims, B = tc.SHAPES[NAME]
    p0, d, feats, gt, cmask, vid, sid = tc.case(oracle, NAME)
    Tc, V = d.n_caption_lstm_step, d.n_words
    mk = lambda: M.Video_Caption_Generator(dim_image=d.dim_image, n_words=d.n_words, word_dim=d.word_dim, lstm_dim=d.lstm_dim, batch_size=B,
                                           n_lstm_steps=d.n_video_lstm_step + Tc, n_video_lstm_step=d.n_video_lstm_step,
                                           n_caption_lstm_step=Tc, bias_init_vector=None, multisample=1, loss_weight=loss_weight)
    model, fused = mk(), mk()
    model.store.load(p0)
    features_batch = [feats[j].tolist() for j in range(B)]          # the reference feeds lists
    captions_ind, captions_mask = gt.tolist(), cmask.tolist()
    start_learning_rate = 1e-3

    # ---- sum_generate_words_tf_s2vt.py:429-435
    tf_loss, tf_video, tf_caption, tf_caption_mask, tf_probs, tf_steps = model.build_topk_feed_model()
    sess = Session(model)
    learning_rate = model.exponential_decay(start_learning_rate, 20000, 0.5)
    train_op = model.minimize((tf_loss, tf_video, tf_caption, tf_caption_mask, tf_probs, tf_steps), learning_rate, clip_norm=10)
    assert len(tf_probs) == Tc
    m0, v0 = model.store.m.clone(), model.store.v.clone()
    fused._keep_topk_feed_logits = True
    names = model.store.names
    clipped_any = False

    for it in range(3):
        fused.store.theta.copy_(model.store.theta)
        fused.set_step(model.global_step)
        p = {n: model.store.p[n].cpu().numpy().copy() for n in names}                      # the variables this step starts from
        r = tc.unroll(oracle, p, d, feats, gt, cmask, vid, sid, keep=model.dropout_rate,
                      drop_seed=model.dropout_seed + 104729 * model.global_step, loss_weight=model.loss_weight)
        wd = fused.l2_term()
        lr_now = sess.run(learning_rate)
        st = fused.topk_feed_update(feats, gt, cmask, lr=lr_now, clip_norm=10.0, clip="per_variable", optimizer="sgd")

        feed_dict = {tf_video: features_batch, tf_caption: captions_ind, tf_caption_mask: captions_mask, tf_steps: it}   # (steps: fed, unused)
        if it < 2:
            _, loss_val = sess.run([train_op, tf_loss], feed_dict=feed_dict)
        else:
            out = sess.run([train_op, tf_loss] + tf_probs, feed_dict=feed_dict)
            loss_val, probs = out[1], out[2:]
            assert all(q.shape == (B, V) and q.dtype == np.float32 for q in probs)
            assert np.array_equal(np.stack(probs).reshape(Tc * B, V), r["logits"])
            assert np.array_equal(np.stack(probs).reshape(Tc * B, V), fused.last_topk_feed["probs"].cpu().numpy())
        assert np.array_equal(model.last_topk_feed["generated"].cpu().numpy(), r["generated"])
        assert torch.equal(model.last_topk_feed["generated"], st.generated)
        print(f"step {it}: loss {loss_val!r} fused {float(st.loss) + wd!r}")
        assert abs(loss_val - (float(st.loss) + wd)) <= 1e-6 * abs(loss_val)
        lr = sess.run(learning_rate)
        assert lr == start_learning_rate and model.global_step == it + 1 == fused.global_step
        # the update: a float64 replay of tf.clip_by_norm(grad, 10) per variable and the SGD step on the gradients in the bucket
        moved = 0.0
        for n in names:
            g = model.store.g[n].cpu().numpy().astype(np.float64)
            nrm = float((g ** 2).sum()) ** 0.5
            clipped_any |= nrm > 10.0
            want = p[n].astype(np.float64) - lr_now * g * (10.0 / max(nrm, 10.0))
            got = model.store.p[n].cpu().numpy()
            assert np.allclose(got, want, rtol=2e-5, atol=2e-6), n
            assert np.allclose(got, fused.store.p[n].cpu().numpy(), rtol=1e-6, atol=1e-8), n
            moved = max(moved, np.abs(got - p[n]).max())
        assert moved > 0
    assert not clipped_any                                           # the clip acts on no variable at the script's 20
    assert torch.equal(model.store.m, m0) and torch.equal(model.store.v, v0) and model.adam_t == 0       # plain gradient descent
    assert gpu.chain_timeouts() == 0



def test_build_generator_with_the_topk_feed(gpu, oracle):
    """build_generator(topk_feed=k) through Session.run, one video fed as a list (:221-275): the word fetches are generate_topk_feed's ids
    of that video, which are the restatement's; beam search over the soft feed is refused."""
    from s2vt_amd import model as M
    from s2vt_amd.model import Session
    dims, B = tc.SHAPES[NAME]
    p, d, feats, *_ = tc.case(oracle, NAME)
    Tc = d.n_caption_lstm_step
    model = M.Video_Caption_Generator(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, B, 0, d.n_video_lstm_step, Tc, multisample=1)
    model.store.load(p)
    video, sentence, _ = model.build_generator(topk_feed=tc.K)
    assert len(sentence) == Tc
    sess = Session(model)
    ref_ids, _ = tc.generate(oracle, p, d, feats, k=tc.K)
    for j in (0, 3):
        words = sess.run(sentence, feed_dict={video: [feats[j].tolist()]})
        assert [int(w) for w in words] == ref_ids[j].tolist()
        assert [int(w) for w in words] == model.generate_topk_feed(feats[j:j + 1], k=tc.K).cpu().numpy()[0].tolist()
    with pytest.raises(ValueError):
        model.build_generator(beam_size=3, topk_feed=tc.K)
    assert gpu.chain_timeouts() == 0
