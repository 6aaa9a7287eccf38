"""The residual cases (tests/residual_cases.py) on the CPU: every case the GPU tests compare against discriminates between the plain and
the residual model, and the float64 restatement the gradients are checked against computes what the fp32 one does."""
import numpy as np
import pytest

import residual_cases as RC


@pytest.mark.parametrize("name,K,seed,video_base", RC.SAMPLE_CASES)
def test_cases_discriminate(oracle, name, K, seed, video_base):
    res, plain = RC.decodes(oracle, name, seed, K, video_base=video_base)
    RC.assert_visible(name, res, plain)


def test_every_shape_has_a_case():
    assert {c[0] for c in RC.SAMPLE_CASES} == set(RC.SHAPES)


@pytest.mark.parametrize("name", list(RC.EOS_BIAS))
def test_eos_cases_end_rows_early_and_keep_some(oracle, name):
    (s, g), _ = RC.decodes(oracle, name, RC.SAMPLER_SEEDS[0], eos=True)
    first = RC.first_eos(np.concatenate([s, g]))
    Tc = s.shape[1]
    assert (first < Tc - 1).any() and (first == Tc).any()


def test_restatement_with_the_flag_off_is_the_oracle(oracle):
    p, d, video = RC.case(oracle, "small-odd")
    ref_s, ref_g = oracle.sample_captions(p, d, video, K=2, seed=11)
    s, g = RC.residual_sample(oracle, p, d, video, 2, 11, residual=False)
    assert np.array_equal(s, ref_s) and np.array_equal(g, ref_g)
    cap = np.random.default_rng(0).integers(0, d.n_words, (video.shape[0], d.n_caption_lstm_step)).astype(np.int32)
    assert np.array_equal(RC.residual_teacher_forced(oracle, p, d, video, cap, residual=False), oracle.teacher_forced(p, d, video, cap))


@pytest.mark.parametrize("keep", [1.0, 0.9])
@pytest.mark.parametrize("name", ["small-odd", "one-tile"])
def test_float64_restatement_agrees_with_the_fp32_one(oracle, name, keep):
    import torch
    from oracle import s2vt_torch as T
    p, d, video = RC.case(oracle, name)
    B = video.shape[0]
    cap = np.random.default_rng(2).integers(0, d.n_words, (B, d.n_caption_lstm_step)).astype(np.int32)
    vid = np.arange(B, dtype=np.int32); sid = np.zeros(B, np.int32)
    drop = None if keep >= 1 else oracle.dropout_masks(RC.DROP_SEED, vid, sid, keep, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step)
    ref = RC.residual_teacher_forced(oracle, p, d, video, cap, drop, keep)
    with torch.no_grad():
        got = RC.torch_teacher_forced(T.to_torch(p, torch.float64, False), video, cap, drop, keep).numpy()
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()
    plain = RC.residual_teacher_forced(oracle, p, d, video, cap, drop, keep, residual=False)
    assert np.abs(plain - ref).max() > 1e-2 * np.abs(ref).max()          # (and the sum is not a rounding-size effect)
