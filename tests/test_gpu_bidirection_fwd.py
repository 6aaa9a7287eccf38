"""The bidirectional captioner's forward side on the GPU (s2vt_bidir_teacher_forced_fwd / s2vt_bidir_decode_greedy behind
s2vt_amd.bidirection, bidirection_tf_s2vt.py:85-216) against the CPU
restatement of tests/bidirection_cases.py, which test_bidirection_cases_cpu.py shows to tell the true model from four half-built ones:
teacher-forced logits (LSTM2's DropoutWrapper at keep 0.9 and 1.0) and greedy ids with both pick forms, bit for bit, at every case --
the 64- and 65-row shapes sit on the two sides of the row limit of the one-launch LSTM1 recurrence; build_generator on one video
equals its row of the batch; every form of the LSTM1 call gives the same logits."""
import numpy as np
import pytest

import bidirection_cases as BC

pytestmark = pytest.mark.gpu

_models = {}


def _model(oracle, name):
    import torch
    from s2vt_amd import bidirection
    if name not in _models:
        p, d, video, cap, vid, sid = BC.case(oracle, name)
        m = bidirection.Video_Caption_Generator(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, video.shape[0], d.n_video_lstm_step + d.n_caption_lstm_step,
                                                d.n_video_lstm_step, d.n_caption_lstm_step, params=p)
        _models[name] = (m, torch.as_tensor(video).cuda(), torch.as_tensor(cap).cuda())
    return _models[name]


def _time_major(logits):
    B, Tc, V = logits.shape
    return np.ascontiguousarray(logits.transpose(1, 0, 2)).reshape(Tc * B, V)


@pytest.mark.parametrize("keep", BC.KEEPS)
@pytest.mark.parametrize("name", list(BC.SHAPES))
def test_teacher_forced_logits(gpu, oracle, name, keep):
    import torch
    m, video, cap = _model(oracle, name)
    _, d, _, _, vid, sid = BC.case(oracle, name)
    got = m.teacher_forced_logits(video, cap, keep=keep, seed=BC.DROP_SEED, video_id=torch.as_tensor(vid).cuda(), sample_id=torch.as_tensor(sid).cuda())
    assert gpu.chain_timeouts() == 0
    assert np.array_equal(got.cpu().numpy(), _time_major(BC.reference(oracle, name)[("tf", keep)]))


@pytest.mark.parametrize("unshifted", [False, True])
@pytest.mark.parametrize("name", list(BC.SHAPES))
def test_greedy_ids(gpu, oracle, name, unshifted):
    m, video, _ = _model(oracle, name)
    ref = BC.reference(oracle, name)
    ids, logits = m.build_sampler(video, unshifted_softmax=unshifted, want_logits=True)
    assert gpu.chain_timeouts() == 0
    if not unshifted:                                                         # (the other pick may feed other words on)
        assert np.array_equal(logits.cpu().numpy(), ref["logits_greedy"])
    assert np.array_equal(ids.cpu().numpy(), ref["ids_unshifted" if unshifted else "ids"])
    assert ids.dtype.is_floating_point is False and tuple(ids.shape) == ref["ids"].shape


@pytest.mark.parametrize("name", ["small-odd", "chain-range"])
def test_build_generator_is_its_row_of_the_batch(gpu, oracle, name):
    m, video, _ = _model(oracle, name)
    batch = m.build_sampler(video, unshifted_softmax=True)
    for b in (0, video.shape[0] - 1):
        v, sentence, probs = m.build_generator(video[b:b + 1].contiguous())
        assert probs == [] and tuple(sentence.shape) == (m.n_caption_lstm_step,)
        assert np.array_equal(sentence.cpu().numpy(), batch[b].cpu().numpy())


@pytest.mark.parametrize("name,forms", [("one-tile", (1, 2, 0)), ("rows-65", (2, 0))])
def test_every_form_of_the_lstm1_call_gives_the_same_logits(gpu, oracle, name, forms):
    m, video, cap = _model(oracle, name)
    ref = _time_major(BC.reference(oracle, name)[("tf", 1.0)])
    for persistent in forms:
        got = m.teacher_forced_logits(video, cap, keep=1.0, persistent=persistent)
        assert np.array_equal(got.cpu().numpy(), ref), persistent


@pytest.mark.parametrize("name", ["small-odd", "rows-65"])
def test_driver_outputs_stay_inside_guard_bands(gpu, oracle, name):
    """s2vt_bidir_teacher_forced_fwd's logits and s2vt_bidir_decode_greedy's ids and logits written into guarded windows (tests/guardband.py),
    the video and the caption read from guarded windows: equal to the restatement, nothing outside the windows touched"""
    import torch
    from guardband import Guarded
    m, video, cap = _model(oracle, name)
    _, d, v_np, c_np, vid, sid = BC.case(oracle, name)
    ref = BC.reference(oracle, name)
    B, Tc, V = v_np.shape[0], d.n_caption_lstm_step, d.n_words
    gv = Guarded.of(v_np.reshape(B, -1), name="video")
    gc = Guarded.of(c_np, dtype=torch.int32, fill=2, name="caption")
    gl = Guarded(Tc * B, V, name="logits")
    gpu.bidir_teacher_forced_fwd(m._dims(), m._params(), gv.view.view(v_np.shape), gc.view, m._workspace(B, "cuda"), keep=1.0, out=gl.view)
    assert np.array_equal(gl.numpy(), _time_major(ref[("tf", 1.0)]))
    for unshifted in (False, True):
        gi = Guarded(B, Tc, dtype=torch.int32, name="ids")
        gg = Guarded(B, Tc * V, name="decode logits")
        gpu.bidir_decode_greedy(m._dims(), m._params(), gv.view.view(v_np.shape), unshifted, want_logits=True, ids=gi.view, logits=gg.view)
        assert np.array_equal(gi.numpy(), ref["ids_unshifted" if unshifted else "ids"])
        if not unshifted:
            assert np.array_equal(gg.numpy().reshape(B, Tc, V), ref["logits_greedy"])
        for g in (gi, gg):
            g.assert_intact()
    for g in (gv, gc, gl):
        g.assert_intact()
    assert gpu.chain_timeouts() == 0


def test_what_the_script_has_no_graph_for_is_refused(gpu, oracle):
    m, video, cap = _model(oracle, "small-odd")
    for fn in (m.sample, m.reinforce_update, m.build_mix_sample, m.scheduled_update, m.beam_search):
        with pytest.raises(ValueError, match="no graph"):
            fn(video)
