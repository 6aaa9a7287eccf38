"""The bidirection cases (tests/bidirection_cases.py) on the CPU: every case the GPU tests compare against tells the true model from
four wrong ones a half-built driver would compute (the backward direction run in forward order, its outputs not re-reversed, left at
zero, or started behind the padding prefix).  A condition, not a measurement: a case that did not meet it would pass with the feature
half built."""
import numpy as np
import pytest

import bidirection_cases as BC


@pytest.mark.parametrize("variant", BC.VARIANTS)
@pytest.mark.parametrize("name", BC.DECODING)
def test_greedy_ids_discriminate(oracle, name, variant):
    p, d, video, cap, vid, sid = BC.case(oracle, name)
    ref = BC.reference(oracle, name)["ids"]
    ids, _ = BC.greedy(oracle, p, d, video, vid, variant=variant)
    differ = int((ids != ref).any(1).sum())
    B = video.shape[0]
    print(f"{name} {variant}: {differ}/{B} rows differ, {len(np.unique(ref))} distinct ids")
    assert 2 * differ >= B, (differ, B)
    assert len(np.unique(ref)) > 1                                            # (the decode has not collapsed to one token)


@pytest.mark.parametrize("variant", BC.VARIANTS)
@pytest.mark.parametrize("name", list(BC.SHAPES))
def test_teacher_forced_logits_discriminate(oracle, name, variant):
    p, d, video, cap, vid, sid = BC.case(oracle, name)
    ref = BC.reference(oracle, name)[("tf", 1.0)]
    got = BC.teacher_forced(oracle, p, d, video, cap, vid, sid, 1.0, variant=variant)
    assert not np.array_equal(got, ref)
    assert (got != ref).any((1, 2)).all()                                     # every row


def test_biases_are_not_zero_and_small(oracle):
    p = BC.case(oracle, "small-odd")[0]
    for n in ("lstm1_fw_b", "lstm1_bw_b", "lstm2_b"):
        assert np.abs(p[n]).max() <= BC.BIAS_A and np.count_nonzero(p[n]) == p[n].size


def test_backward_direction_moves_through_the_padding(oracle):
    """what the non-zero biases are for: after the Tc padding steps the backward cell's state is not zero, so skipping them shows"""
    p, d, video, *_ = BC.case(oracle, "small-odd")
    o1 = BC.output1(oracle, p, d, video)
    H = d.lstm_dim
    assert np.abs(o1[d.n_video_lstm_step][:, H:]).max() > 1e-3
