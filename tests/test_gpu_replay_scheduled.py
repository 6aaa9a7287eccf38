"""The scheduled-sampling script's train(), replayed statement by statement through the drop-in class: generate_words_tf_s2vt.py:405-418
(model, build_model, exponential_decay(1e-3, g_step, 20000, 0.5, staircase), GradientDescentOptimizer, clip_by_global_norm 10 ->
train_op) and :441-457 (sess.run([train_op, tf_loss], {tf_video, tf_caption, tf_steps}), steps += 1, sess.run(learning_rate)).

Three steps on the one-tile case of tests/scheduled_cases.py.  Each step's expected loss, gradients and update are computed from the
variables READ BACK FROM THE DEVICE before that step: a 1e-7 difference in the variables may flip a later argmax, so the steps are never
chained through the restatement."""
import numpy as np
import pytest

import scheduled_cases as sc

pytestmark = pytest.mark.gpu

NAME = "one-tile"


def test_replay_scheduled_train(gpu, oracle):
    import torch
    from s2vt_amd import model as M
    from s2vt_amd.model import Session
    from oracle import s2vt_torch as T
    dims, B = sc.SHAPES[NAME]
    p0, d, feats, gt, vid, sid = sc.case(oracle, NAME)
    Tc, V = d.n_caption_lstm_step, d.n_words
    model = M.Video_Caption_Generator(dim_image=d.dim_image, n_words=d.n_words, word_dim=d.word_dim, lstm_dim=d.lstm_dim, batch_size=B,
                                      n_lstm_steps=d.n_video_lstm_step + Tc, n_video_lstm_step=d.n_video_lstm_step,
                                      n_caption_lstm_step=Tc, bias_init_vector=None, multisample=1)
    model.store.load(p0)
    features_batch = [feats[j].tolist() for j in range(B)]          # the reference feeds lists
    captions_ind = gt.tolist()
    start_learning_rate = 1e-3

    # ---- generate_words_tf_s2vt.py:405-418
    tf_loss, tf_video, tf_caption, tf_caption_mask, tf_probs, tf_steps = model.build_scheduled_model()
    sess = Session(model)
    learning_rate = model.exponential_decay(start_learning_rate, 20000, 0.5)
    train_op = model.minimize((tf_loss, tf_video, tf_caption, tf_caption_mask, tf_probs, tf_steps), learning_rate, clip_norm=10, optimizer="sgd")
    assert len(tf_probs) == Tc
    m0, v0 = model.store.m.clone(), model.store.v.clone()

    steps = 0
    runs = 0                                                         # runs of the graph so far: run n draws coin seed ... + 104723 * n
    for it in range(3):
        p = {n: model.store.p[n].cpu().numpy().copy() for n in model.store.names}          # the variables this step starts from
        runs += 1
        coin_seed = model.sample_seed + 7919 * (model.global_step + 1) + 104723 * runs
        dseed = model.dropout_seed + 104729 * model.global_step
        r = sc.scheduled_unroll(oracle, p, d, feats, gt, sc.p_gt_of(0.5), coin_seed, vid, sid, keep=model.dropout_rate, drop_seed=dseed,
                                loss_weight=model.loss_weight)
        sc.assert_visible(r)
        pt = T.to_torch(p, torch.float64, True)
        fed = torch.as_tensor(r["fed"]).long()
        lg = T.unroll(pt, torch.as_tensor(feats).double(), lambda t, _: fed[:, t], Tc, r["drop"], model.dropout_rate)
        ce = -torch.log_softmax(lg, -1).gather(2, torch.as_tensor(gt).long().unsqueeze(-1)).squeeze(-1)
        mask = torch.as_tensor(r["mask"]).double()
        wd = sum(0.5 * (x ** 2).sum() for k, x in pt.items() if k not in ("lstm1_b", "lstm2_b"))
        ref_loss = model.loss_weight * (ce * mask).sum() / mask.sum() + model.decay_value * wd          # :198-210
        ref_loss.backward()
        ref_g = {k: x.grad.numpy() for k, x in pt.items()}

        # ---- :441-447 (the last step also fetches caption_mask and probs, with the reference's shapes)
        feed_dict = {tf_video: features_batch, tf_caption: captions_ind, tf_steps: steps}
        if it < 2:
            _, loss_val = sess.run([train_op, tf_loss], feed_dict=feed_dict)
        else:
            out = sess.run([train_op, tf_loss, tf_caption_mask] + tf_probs, feed_dict=feed_dict)
            loss_val, cmask, probs = out[1], out[2], out[3:]
            assert cmask.shape == (Tc, B, 1) and cmask.dtype == np.float32 and np.array_equal(cmask[:, :, 0], r["mask"].T)
            assert all(q.shape == (B, V) for q in probs) and np.array_equal(np.stack(probs).reshape(Tc * B, V), r["logits"])
        steps += 1
        print(f"step {it}: loss {loss_val!r} reference {float(ref_loss.detach())!r}")
        assert abs(loss_val - float(ref_loss.detach())) <= 1e-4 * max(1.0, abs(float(ref_loss.detach())))
        lr = sess.run(learning_rate)
        assert lr == start_learning_rate and model.global_step == it + 1

        # the gradients the train_op differentiated (in the bucket, before the clip scale) vs float64 autograd
        g_gpu = {}
        for n in model.store.names:
            g_gpu[n] = model.store.g[n].cpu().numpy().astype(np.float64)
            scale = np.abs(ref_g[n]).max() + 1e-30
            assert np.abs(g_gpu[n] - ref_g[n]).max() <= 2e-4 * scale + 1e-9, n
        # the update: tf.clip_by_global_norm(10) + GradientDescentOptimizer in float64 on those gradients
        nrm = np.sqrt(sum((g ** 2).sum() for g in g_gpu.values()))
        s = 10.0 / max(nrm, 10.0)
        moved = 0.0
        for n in model.store.names:
            got = model.store.p[n].cpu().numpy()
            want = p[n].astype(np.float64) - lr * g_gpu[n] * s
            assert np.allclose(got, want, rtol=2e-5, atol=2e-6), n
            moved = max(moved, np.abs(got - p[n]).max())
        assert moved > 0
    assert torch.equal(model.store.m, m0) and torch.equal(model.store.v, v0) and model.adam_t == 0       # plain gradient descent
    assert gpu.chain_timeouts() == 0


def test_forward_fetches_and_the_schedule(gpu, oracle):
    """Fetching loss / caption_mask / probs alone evaluates the forward only; with k_value the fed step count sets the probability
    (p = k / (k + exp(steps / k)), :134): a huge step count never feeds the ground truth, step 0 with a huge k always does."""
    from s2vt_amd import model as M
    from s2vt_amd.model import Session
    dims, B = sc.SHAPES[NAME]
    p, d, feats, gt, vid, sid = sc.case(oracle, NAME)
    Tc = d.n_caption_lstm_step
    model = M.Video_Caption_Generator(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, B, 0, d.n_video_lstm_step, Tc, multisample=1)
    model.store.load(p)
    before = model.store.theta.clone()
    loss, video, caption, cmask, probs, steps = model.build_scheduled_model(k_value=50.0)
    sess = Session(model)
    dseed = model.dropout_seed + 104729 * model.global_step
    for n_run, (s, prob) in enumerate([(10 ** 6, 0.0), (0, 50.0 / 51.0)], start=1):
        seed = model.sample_seed + 7919 * (model.global_step + 1) + 104723 * n_run
        r = sc.scheduled_unroll(oracle, p, d, feats, gt, sc.p_gt_of(prob), seed, vid, sid, keep=model.dropout_rate, drop_seed=dseed)
        out = sess.run([loss, cmask] + probs, feed_dict={video: feats, caption: gt, steps: s})
        assert np.array_equal(out[1][:, :, 0], r["mask"].T) and np.array_equal(np.stack(out[2:]).reshape(-1, d.n_words), r["logits"])
        nll = np.concatenate([oracle.row_losses(np.ascontiguousarray(r["logits"][t * B:(t + 1) * B]), gt[:, t].copy(), 0.0)[0] for t in range(Tc)])
        want = float((r["coef_tm"].astype(np.float64) * nll).sum() / r["mask_sum"]) + model.l2_term()
        assert abs(out[0] - want) <= 1e-4 * max(1.0, abs(want))
        if prob == 0.0:
            assert not r["coin"].any()
    with pytest.raises(KeyError):
        sess.run(loss, feed_dict={video: feats, caption: gt})        # the schedule reads `steps`
    assert model.global_step == 0 and bool((model.store.theta == before).all())
