"""The CPU restatement of the scheduled-sampling unroll (tests/scheduled_cases.py) against the oracle's own unrolls at the two ends of the
coin's range, and the visibility conditions of every case the GPU tests use."""
import numpy as np
import pytest

import scheduled_cases as sc


@pytest.mark.parametrize("keep", [1.0, 0.9])
@pytest.mark.parametrize("name", ["small-odd", "one-tile", "one-step"])
def test_always_truth_is_the_teacher_forced_unroll(oracle, name, keep):
    p, d, video, gt, vid, sid = sc.case(oracle, name)
    r = sc.scheduled_unroll(oracle, p, d, video, gt, np.float32(1.0), 5, vid, sid, keep=keep)
    want = oracle.teacher_forced(p, d, video, gt, r["drop"], keep)                     # [N, Tc, V]
    N, Tc = gt.shape
    assert np.array_equal(r["logits"].reshape(Tc, N, -1), want.transpose(1, 0, 2))
    assert np.array_equal(r["fed"][:, 1:], gt[:, :-1]) and (r["fed"][:, 0] == 1).all()
    assert np.array_equal(r["generated"], want.argmax(-1).astype(np.int32))
    if keep < 1.0:
        assert not np.array_equal(want, oracle.teacher_forced(p, d, video, gt))       # (the masks took effect)


@pytest.mark.parametrize("name", ["small-odd", "one-tile", "many-rows"])
def test_never_truth_is_the_greedy_sampler(oracle, name):
    p, d, video, gt, vid, sid = sc.case(oracle, name)
    r = sc.scheduled_unroll(oracle, p, d, video, gt, np.float32(0.0), 5, vid, sid, keep=1.0)
    _, greedy = oracle.sample_captions(p, d, video, 0, 9, 0, True)
    assert np.array_equal(r["generated"], greedy)
    assert np.array_equal(r["fed"][:, 1:], greedy[:, :-1])
    assert not r["coin"].any()


def test_mask_is_sq1(oracle):
    """Quirk SQ1: the mask of step t already reflects step t's own pick, and stays 0 behind it."""
    p, d, video, gt, vid, sid = sc.case(oracle, "one-tile")
    r = sc.scheduled_unroll(oracle, p, d, video, gt, sc.p_gt_of(0.5), sc.SEEDS[0], vid, sid)
    alive = np.cumprod(r["generated"] != 0, axis=1).astype(np.float32)
    assert np.array_equal(r["mask"], alive)
    first = (r["generated"] == 0).argmax(1)
    rows = np.flatnonzero((r["generated"] == 0).any(1))
    assert rows.size and all(r["mask"][n, first[n]] == 0 for n in rows)                # the <eos> position itself is masked
    assert np.array_equal(r["coef_tm"].reshape(gt.shape[1], -1), r["mask"].T)


@pytest.mark.parametrize("keep", sc.KEEPS)
@pytest.mark.parametrize("prob", sc.PROBS)
@pytest.mark.parametrize("name", list(sc.SHAPES))
def test_every_case_is_visible(oracle, name, prob, keep):
    p, d, video, gt, vid, sid = sc.case(oracle, name)
    for seed in sc.SEEDS:
        sc.assert_visible(sc.scheduled_unroll(oracle, p, d, video, gt, sc.p_gt_of(prob), seed, vid, sid, keep=keep))
