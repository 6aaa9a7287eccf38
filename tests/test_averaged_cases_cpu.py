"""tests/averaged_cases.py on the CPU: every case shows what the averaged-embedding parity tests rely on, and the restatement is told
apart from each half-built variant of the rule (average_generate_words_tf_s2vt.py:124-133)."""
import numpy as np
import pytest

import averaged_cases as ac

_refs = {}


def _ref(oracle, name, keep=1.0, variant=None):
    key = (name, keep, variant)
    if key not in _refs:
        p, d, video, gt, mask, vid, sid = ac.case(oracle, name)
        _refs[key] = ac.averaged_unroll(oracle, p, d, video, gt, mask, vid, sid, keep=keep, variant=variant)
    return _refs[key]


@pytest.mark.parametrize("keep", ac.KEEPS)
@pytest.mark.parametrize("name", [n for n in ac.SHAPES if n != "chain-range"])
def test_cases_are_visible(oracle, name, keep):
    r = _ref(oracle, name, keep)
    ac.assert_visible(r)
    if r["generated"].shape[1] > 1:
        assert ac.only_picked_rows(r)


def test_chain_range_is_visible(oracle):
    ac.assert_visible(_ref(oracle, "chain-range"))


def test_masks_are_ragged(oracle):
    for name in ac.SHAPES:
        mask = ac.case(oracle, name)[4]
        assert (mask[0] == 0).all() and (mask[1] == 1).all()
        if mask.shape[1] > 1:
            assert len(set(mask.sum(1).tolist())) > 2
        assert ac.mask_sum_fixed_order(mask) == float(mask.astype(np.float64).sum())


def test_equal_ids_give_the_row_itself(oracle):
    W = ac.case(oracle, "small-odd")[0]["Wemb"]
    ids = np.arange(W.shape[0])
    assert np.array_equal(ac.mean_rows(W, ids, ids), W)


@pytest.mark.parametrize("variant", ac.VARIANTS)
@pytest.mark.parametrize("name", ["small-odd", "odd-width"])
def test_restatement_differs_from_the_half_built_rule(oracle, name, variant):
    a, b = _ref(oracle, name), _ref(oracle, name, variant=variant)
    assert not np.array_equal(a["logits"], b["logits"])
    if variant == "mean-at-step-0":
        assert not np.array_equal(a["logits"][:a["generated"].shape[0]], b["logits"][:a["generated"].shape[0]])      # step 0 already
    else:
        N = a["generated"].shape[0]
        assert np.array_equal(a["logits"][:N], b["logits"][:N])                                                    # step 0 feeds <bos> alone
        assert not np.array_equal(a["logits"][N:2 * N], b["logits"][N:2 * N])


def test_one_step_forms_no_mean(oracle):
    """Tc = 1: the variants that change the mean of step t >= 1 cannot show."""
    a = _ref(oracle, "one-step")
    for variant in ("truth-only", "argmax-only", "sum", "caption-t"):
        assert np.array_equal(a["logits"], _ref(oracle, "one-step", variant=variant)["logits"])
