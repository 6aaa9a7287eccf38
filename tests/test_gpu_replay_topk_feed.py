"""The top-k feed script's train(), replayed statement by statement through the drop-in class: sum_generate_words_tf_s2vt.py:429-435
(build_model, exponential_decay(start, g_step, 20000, 0.5, staircase), GradientDescentOptimizer, tf.clip_by_norm(grad, 10) per variable ->
train_op) and the loop's sess.run([train_op, tf_loss], {tf_video, tf_caption, tf_caption_mask, steps}), sess.run(learning_rate).

Three steps on the small-odd case of tests/topk_feed_cases.py.  Every fetch is checked against the fused topk_feed_update of a second model
that starts each step from the variables READ BACK from the first (a 1e-7 difference in the variables may flip a later top-k, so the steps
are never chained across the two), and the update against a float64 replay of clip and step on the gradients the device left in the
bucket, rtol 2e-5 / atol 2e-6."""
import numpy as np
import pytest

import topk_feed_cases as tc

pytestmark = pytest.mark.gpu

NAME = "small-odd"


def test_replay_topk_feed_train(gpu, oracle):
    import torch
    from s2vt_amd import model as M
    from s2vt_amd.model import Session
    dims, B = tc.SHAPES[NAME]
    p0, d, feats, gt, cmask, vid, sid = tc.case(oracle, NAME)
    Tc, V = d.n_caption_lstm_step, d.n_words
    mk = lambda: M.Video_Caption_Generator(dim_image=d.dim_image, n_words=d.n_words, word_dim=d.word_dim, lstm_dim=d.lstm_dim, batch_size=B,
                                           n_lstm_steps=d.n_video_lstm_step + Tc, n_video_lstm_step=d.n_video_lstm_step,
                                           n_caption_lstm_step=Tc, bias_init_vector=None, multisample=1, loss_weight=60)
    # (the script's loss_weight is 20; at this case's size its largest per-variable norm is 4.4 -- float64 autograd, embed_word_b -- so 60
    #  puts that one variable above the clip of 10 and leaves the next, 5.3, below)
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
    assert clipped_any                                               # the clip acts on some variable
    assert torch.equal(model.store.m, m0) and torch.equal(model.store.v, v0) and model.adam_t == 0       # plain gradient descent
    assert gpu.chain_timeouts() == 0


def test_learning_rate_staircase_at_20000(gpu):
    from s2vt_amd import model as M
    from s2vt_amd.model import Session
    model = M.Video_Caption_Generator(64, 131, 24, 32, 5, 0, 3, 9, multisample=1)
    lr = model.exponential_decay(1e-3, 20000, 0.5)
    sess = Session(model)
    for step, want in ((0, 1e-3), (19999, 1e-3), (20000, 5e-4), (40000, 2.5e-4)):
        model.set_step(step)
        assert sess.run(lr) == want


def test_forward_fetches_leave_the_variables_alone(gpu, oracle):
    """Fetching loss / probs alone evaluates the forward only: the restatement's logits, the loss of :212-218, no update; steps may be
    left unfed."""
    from s2vt_amd import model as M
    from s2vt_amd.model import Session
    dims, B = tc.SHAPES[NAME]
    p, d, feats, gt, cmask, vid, sid = tc.case(oracle, NAME)
    Tc = d.n_caption_lstm_step
    model = M.Video_Caption_Generator(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, B, 0, d.n_video_lstm_step, Tc, multisample=1)
    model.store.load(p)
    before = model.store.theta.clone()
    loss, video, caption, caption_mask, probs, steps = model.build_topk_feed_model()
    sess = Session(model)
    r = tc.unroll(oracle, p, d, feats, gt, cmask, vid, sid, keep=model.dropout_rate, drop_seed=model.dropout_seed, loss_weight=model.loss_weight)
    out = sess.run([loss] + probs, feed_dict={video: feats, caption: gt, caption_mask: cmask})
    assert np.array_equal(np.stack(out[1:]).reshape(-1, d.n_words), r["logits"])
    nll = np.concatenate([oracle.row_losses(np.ascontiguousarray(r["logits"][t * B:(t + 1) * B]), gt[:, t].copy(), 0.0)[0] for t in range(Tc)])
    want = float((r["coef_tm"].astype(np.float64) * nll).sum() / r["mask_sum"]) + model.l2_term()
    assert abs(out[0] - want) <= 1e-4 * max(1.0, abs(want))
    with pytest.raises(KeyError):
        sess.run(loss, feed_dict={video: feats, caption: gt})        # caption_mask is an input here (:106)
    assert model.global_step == 0 and bool((model.store.theta == before).all())
