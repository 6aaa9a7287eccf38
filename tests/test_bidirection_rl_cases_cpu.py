"""The REINFORCE cases of the bidirectional captioner (tests/bidirection_rl_cases.py) on the CPU: the conditions under which equality with
the restated sampler shows that the row -> video map, the noise counters and the ragged mask are honoured.  Conditions, not
measurements: a case that did not meet them would pass with the feature half built."""
import numpy as np
import pytest

import bidirection_rl_cases as RC


@pytest.mark.parametrize("name", RC.MULTI_STEP)
def test_a_quarter_of_the_sampled_rows_end_early_and_one_does_not(oracle, name):
    ref = RC.reference(oracle, name)
    ids, mask = ref["sampled"], ref["mask"]
    N, Tc = ids.shape
    early = int((mask.sum(1) < Tc).sum())
    print(f"{name}: {early} of {N} sampled rows end before Tc = {Tc}")
    assert 4 * early >= N, (early, N)
    assert early < N                                                          # at least one row runs to the end
    assert (mask[:, 0] == 1).all()


@pytest.mark.parametrize("name", list(RC.SAMPLES))
def test_the_samples_of_a_video_are_not_all_equal(oracle, name):
    p, d, video, S = RC.case(oracle, name)
    B = video.shape[0]
    ids = RC.reference(oracle, name)["sampled"].reshape(S, B, -1)
    for j in range(B):
        assert any(not np.array_equal(ids[0, j], ids[s, j]) for s in range(1, S)), j


@pytest.mark.parametrize("name", RC.MULTI_STEP)
def test_a_wrong_row_to_video_map_changes_half_the_rows(oracle, name):
    p, d, video, S = RC.case(oracle, name)
    ref = RC.reference(oracle, name)["sampled"]
    wrong, _, _ = RC.sample(oracle, p, d, video, S, row_video="wrong")
    differ = int((wrong != ref).any(1).sum())
    ops_only, g_wrong, _ = RC.sample(oracle, p, d, video, S, row_video="wrong-operands")
    print(f"{name}: {differ} of {ref.shape[0]} rows differ under n // S ({int((ops_only != ref).any(1).sum())} with the right noise counters; "
          f"greedy block: {int((g_wrong != RC.reference(oracle, name)['greedy']).any(1).sum())} of {g_wrong.shape[0]})")
    assert 2 * differ >= ref.shape[0], (differ, ref.shape[0])


def test_the_mask_restatement_is_hostglues(oracle):
    from s2vt_amd import hostglue
    ids = RC.reference(oracle, "small-odd")["sampled"]
    assert np.array_equal(RC.mask_from_ids(ids), hostglue.masks_from_ids(ids))


def test_the_eos_bias_is_a_copy(oracle):
    import bidirection_cases as BC
    p = RC.case(oracle, "small-odd")[0]
    q = BC.case(oracle, "small-odd")[0]
    assert p["embed_word_b"] is not q["embed_word_b"] and p["embed_word_b"][0] == q["embed_word_b"][0] + np.float32(RC.EOS_BIAS["small-odd"]) and RC.EOS_BIAS["small-odd"] == 3.0
    assert np.array_equal(p["embed_word_b"][1:], q["embed_word_b"][1:])
