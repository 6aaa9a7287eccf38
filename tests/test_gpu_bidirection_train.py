"""Training the bidirectional captioner (s2vt_amd.bidirection; bidirection_tf_s2vt.py:150-165 and :369-375): loss and the gradients of all
eleven variables against float64 autograd of the restatement in tests/bidirection_cases.py, within DESIGN.md section 3's bound for
gradients (max |g - ref| <= 2e-4 of the tensor's largest reference entry; loss within 1e-3 relative); the backward direction's kernel
gradient is far from what a backward cell run in forward order would give; tf.clip_by_norm acts per variable; one SGD step."""
import numpy as np
import pytest

import bidirection_cases as BC

pytestmark = pytest.mark.gpu

GRAD_BOUND, LOSS_BOUND = 2e-4, 1e-3
CASES = ["small-odd", "one-tile", "rows-65", "one-step"]


def _model(oracle, name):
    import torch
    from s2vt_amd import bidirection
    p, d, video, cap, vid, sid = BC.case(oracle, name)
    m = bidirection.Video_Caption_Generator(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, video.shape[0], d.n_video_lstm_step + d.n_caption_lstm_step,
                                            d.n_video_lstm_step, d.n_caption_lstm_step, params=p)
    dev = lambda a: torch.as_tensor(a).cuda()
    return m, dev(video), dev(cap), dev(BC.caption_mask(name, cap)), dev(vid), dev(sid)


@pytest.mark.parametrize("keep", BC.KEEPS)
@pytest.mark.parametrize("name", CASES)
def test_loss_and_gradients_against_float64_autograd(gpu, oracle, name, keep):
    m, video, cap, mask, vid, sid = _model(oracle, name)
    assert m.loss_weight == 20 and m.decay_value == 5e-5
    ref_loss, ref = BC.torch_grads(oracle, name, keep)
    loss, g = m.loss_and_grads(video, cap, mask, keep=keep, seed=BC.DROP_SEED, video_id=vid, sample_id=sid)
    assert gpu.chain_timeouts() == 0
    print(f"{name} keep {keep}: loss {loss:.6f} ref {ref_loss:.6f}")
    assert abs(loss - ref_loss) <= LOSS_BOUND * abs(ref_loss)
    assert set(g) == set(ref) and len(g) == 11
    for n in sorted(g):
        err = np.abs(g[n].cpu().numpy().astype(np.float64) - ref[n]).max() / np.abs(ref[n]).max()
        print(f"  {n}: {err:.2e}")
        assert err <= GRAD_BOUND, (n, err)


def test_backward_direction_gradient_is_not_the_forward_order_one(gpu, oracle):
    name = "small-odd"
    m, video, cap, mask, vid, sid = _model(oracle, name)
    _, ref = BC.torch_grads(oracle, name, 1.0)
    _, wrong = BC.torch_grads(oracle, name, 1.0, variant="forward-order")
    _, g = m.loss_and_grads(video, cap, mask, keep=1.0)
    n = "lstm1_bw_W"
    scale = np.abs(ref[n]).max()
    assert np.abs(wrong[n] - ref[n]).max() / scale > 10 * GRAD_BOUND          # the two models differ visibly in this tensor ...
    assert np.abs(g[n].cpu().numpy() - wrong[n]).max() / scale > 10 * GRAD_BOUND   # ... and the library computes the true one


def test_clip_is_per_variable_and_one_sgd_step(gpu, oracle):
    """scale ONE variable's gradient so that only its norm exceeds 10: only it is rescaled (tf.clip_by_norm per variable, :369-375), and
    the step is theta - lr * clipped gradient for every variable"""
    import torch
    name = "small-odd"
    m, video, cap, mask, vid, sid = _model(oracle, name)
    _, g = m.loss_and_grads(video, cap, mask, keep=1.0)
    norms = {n: float(g[n].double().norm()) for n in g}
    assert max(norms.values()) < 10.0, norms                                   # nothing is clipped as it stands
    big = "lstm2_W"
    s = 25.0 / norms[big]
    g[big].mul_(s)
    sumsq = torch.as_tensor([(norms[n] * (s if n == big else 1.0)) ** 2 for n in m.p], dtype=torch.float32).cuda()
    before = {n: m.p[n].clone() for n in m.p}
    lr = 0.01
    m.global_step = 0
    m.apply_clipped(g, lr, 10.0, sumsq=sumsq)
    for n in m.p:
        gn = g[n].double() * (10.0 / 25.0 if n == big else 1.0)
        want = before[n].double() - lr * gn
        tol = 4 * np.finfo(np.float32).eps * float(before[n].abs().max() + lr * gn.abs().max())      # two fp32 roundings of the update, a few ulps of the clip factor
        assert float((m.p[n].double() - want).abs().max()) <= tol, n


def test_xe_update_moves_every_variable_and_lowers_the_loss(gpu, oracle):
    name = "small-odd"
    m, video, cap, mask, vid, sid = _model(oracle, name)
    before = {n: m.p[n].clone() for n in m.p}
    first = m.minimize(video, cap, mask, optimizer="sgd", clip="per_variable", keep=1.0)
    for _ in range(2):
        last = m.xe_update(video, cap, mask, keep=1.0)
    assert m.global_step == 3 and last < first
    assert all(not bool((m.p[n] == before[n]).all()) for n in m.p)
    with pytest.raises(ValueError, match="no graph"):
        m.minimize(video, cap, mask, optimizer="adam")


@pytest.mark.parametrize("tf_version", [1, 2])
def test_checkpoint_round_trip_under_the_tf_names(gpu, oracle, tmp_path, tf_version):
    """three steps, save as the script's Saver would name things, restore into a fresh model: same variables, same step count, and
    build_generator (the script's test() body, :448-461) decodes the same sentence as the trained model and as the CPU restatement on
    the variables read back from the device"""
    from s2vt_amd import bidirection, tfckpt
    name = "small-odd"
    m, video, cap, mask, vid, sid = _model(oracle, name)
    for _ in range(3):
        m.xe_update(video, cap, mask)                                           # the script's dropout_rate and decayed rate
    path = str(tmp_path / "bimodel-0")
    m.save(path, tf_version=tf_version)
    names = set(tfckpt.read_checkpoint(path))
    assert {"Wemb", "s2vt/LSTM1/bidirectional_rnn/fw/basic_lstm_cell/weights", "s2vt/LSTM1/bidirectional_rnn/bw/basic_lstm_cell/biases",
            "s2vt/LSTM2/basic_lstm_cell/weights", "Variable"} <= names and len(names) == 12
    p, d, v_np, *_ = BC.case(oracle, name)
    fresh = bidirection.Video_Caption_Generator(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, 1, 0, d.n_video_lstm_step, d.n_caption_lstm_step, seed=9)
    fresh.restore(path)
    assert fresh.global_step == 3
    trained = {n: m.p[n].cpu().numpy() for n in m.p}
    for n in m.p:
        assert np.array_equal(fresh.p[n].cpu().numpy(), trained[n]) and not np.array_equal(trained[n], p[n]), n
    ref = BC.greedy(oracle, trained, d, v_np, vid.cpu().numpy(), unshifted=True)[0]
    for b in range(v_np.shape[0]):
        _, sentence, _ = fresh.build_generator(video[b:b + 1].contiguous())
        assert np.array_equal(sentence.cpu().numpy(), ref[b]), b


def test_xe_update_clips_through_the_librarys_own_norm_slots(gpu, oracle):
    """loss_weight = 200 pushes two variables' gradient norms over 10 and leaves nine below: xe_update must rescale exactly those two, by the
    squared norms s2vt_grad_finalize left in each variable's own slot -- a cross-wired or shared slot would move the wrong variables"""
    import torch
    from oracle import s2vt_torch as T
    name = "small-odd"
    m, video, cap, mask, vid, sid = _model(oracle, name)
    m.loss_weight = 200.0
    p, d, v_np, c_np, *_ = BC.case(oracle, name)
    pt = T.to_torch(p, torch.float64, True)
    BC.torch_loss(pt, d, v_np, c_np, BC.caption_mask(name, c_np), None, 1.0, loss_weight=200.0).backward()
    ref = {n: pt[n].grad.numpy() for n in pt}
    norms = {n: float(np.sqrt((ref[n] ** 2).sum())) for n in ref}
    over = sorted(n for n in norms if norms[n] > 10.0)
    assert over == ["embed_word_b", "lstm2_b"], norms
    assert all(abs(v - 10.0) > 0.5 for v in norms.values())                     # nobody sits on the threshold
    lr = 0.01
    m.xe_update(video, cap, mask, lr=lr, keep=1.0)
    slots = dict(zip(m.p, np.sqrt(m._sumsq.cpu().numpy().astype(np.float64))))
    for n in m.p:
        assert abs(slots[n] - norms[n]) <= 1e-3 * norms[n], (n, slots[n], norms[n])
        s = 10.0 / max(norms[n], 10.0)
        want = p[n].astype(np.float64) - lr * ref[n] * s
        got = m.p[n].cpu().numpy()
        assert np.allclose(got, want, rtol=2e-5, atol=lr * 2e-4 * np.abs(ref[n]).max() + 1e-7), n
        if n in over:                                                            # ... and the unclipped step would have been told apart
            unclipped = p[n].astype(np.float64) - lr * ref[n]
            assert np.abs(unclipped - want).max() > 100 * (lr * 2e-4 * np.abs(ref[n]).max() + 1e-7)
