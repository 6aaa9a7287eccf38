"""tests/topk_feed_cases.py on the CPU: every case shows what the top-k feed parity and gradient tests rely on (sum_generate_words_tf_s2vt.py
:163-174), and the restatement is told apart from each half-built variant of the rule.

(a) min |S| >= 0.25 over every (step, row): the division by the raw sum of the scores is well conditioned;
(b) the fp32 restatement's gradients are within 2e-5 of float64's, per tensor, relative to its largest entry;
(c) the weights-detached gradient differs from the full one by >= 2e-3 on every tensor -- ten times the GPU tests' bound, so a backward
    without the score edge cannot pass them;
(d) a selected word occurs in no caption; (e) some row's top-k ids change between steps; (f) five half-built rules give other logits."""
import numpy as np
import pytest

import topk_feed_cases as tc

_refs = {}


def _ref(oracle, name, keep=1.0, variant=None):
    key = (name, keep, variant)
    if key not in _refs:
        p, d, video, gt, mask, vid, sid = tc.case(oracle, name)
        _refs[key] = tc.unroll(oracle, p, d, video, gt, mask, vid, sid, keep=keep, variant=variant)
    return _refs[key]


@pytest.mark.parametrize("keep", tc.KEEPS)
@pytest.mark.parametrize("name", [n for n in tc.SHAPES if n != "chain-range"])
def test_cases_are_visible(oracle, name, keep):
    r = _ref(oracle, name, keep)
    print({k: v for k, v in tc.visibility(r).items()}, "min |S| =", float(np.abs(r["S"]).min()))
    tc.assert_visible(r)


def test_chain_range_is_visible(oracle):
    tc.assert_visible(_ref(oracle, "chain-range"))


def test_masks_are_ragged_and_captions_even(oracle):
    for name in tc.SHAPES:
        _, _, _, gt, mask, _, _ = tc.case(oracle, name)
        assert (mask[0] == 0).all() and (mask[1] == 1).all()
        assert not (gt % 2).any()


def test_top_k_order_and_the_chain():
    """Value descending, index ascending on exact ties -- also across the k-th place; a +0 / -0 pair is a tie; k = 1 gives weight 1."""
    s = np.array([[1.0, 3.0, 3.0, -2.0, 1.0, 1.0, 0.5], [0.0, -0.0, -1.0, -0.0, 0.0, -5.0, -1.0]], np.float32)
    v, ids = tc.top_k(s, 4)
    assert ids.tolist() == [[1, 2, 0, 4], [0, 1, 3, 4]]
    W = np.arange(14, dtype=np.float32).reshape(7, 2) / 8
    i1, w1, S1, x1 = tc.mix(s[:1], W, 1)
    assert w1.tolist() == [[1.0]] and np.array_equal(x1, W[[1]]) and S1.tolist() == [3.0]
    i3, w3, S3, x3 = tc.mix(s[:1], W, 3)
    assert S3.tolist() == [7.0] and np.array_equal(w3, (np.array([[3, 3, 1]], np.float32) / np.float32(7)))
    acc = np.zeros(2, np.float32)
    for j in range(3):
        acc = (acc + w3[0, j] * W[i3[0, j]]).astype(np.float32)
    assert np.array_equal(x3[0], acc)


@pytest.mark.parametrize("name", ["small-odd", "odd-width"])
def test_gradient_conditions(oracle, name):
    """(b) and (c), keep 0.9: float32 against float64 autograd of the same graph, and the weights-detached graph against the full one."""
    p, d, video, gt, mask, vid, sid = tc.case(oracle, name)
    r = _ref(oracle, name, 0.9)
    tc.assert_visible(r)
    _, full, dl_full = tc.autograd(p, video, gt, mask, r, 0.9, 20.0, 0.0)
    f32 = tc.fp32_gradients(p, video, gt, mask, r, 0.9, 20.0)
    err = tc.rel_err(f32, full)
    print("fp32 against float64:", err)
    assert max(err.values()) <= 2e-5, err
    _, det, dl_det = tc.autograd(p, video, gt, mask, r, 0.9, 20.0, 0.0, detach_weights=True)
    gap = tc.rel_err(det, full)
    print("detached against full:", gap)
    assert min(gap.values()) >= 2e-3, gap
    assert np.abs(dl_det - dl_full).max() >= 2e-3 * np.abs(dl_full).max()
    # a selected word outside every caption receives gradient through the mix alone
    rows = tc.selected_outside_captions(r)
    assert rows and any(np.abs(full["Wemb"][k]).max() > 0 for k in rows)


@pytest.mark.parametrize("variant", tc.VARIANTS)
@pytest.mark.parametrize("name", ["small-odd", "odd-width"])
def test_restatement_differs_from_the_half_built_rule(oracle, name, variant):
    a, b = _ref(oracle, name), _ref(oracle, name, variant=variant)
    N = a["generated"].shape[0]
    assert np.array_equal(a["logits"][:N], b["logits"][:N])                                                        # step 0 feeds <bos> alone
    assert not np.array_equal(a["logits"][N:2 * N], b["logits"][N:2 * N])


def test_one_step_forms_no_mix(oracle):
    a = _ref(oracle, "one-step")
    for variant in tc.VARIANTS:
        assert np.array_equal(a["logits"], _ref(oracle, "one-step", variant=variant)["logits"])


def test_generator_rules_differ(oracle):
    """build_generator mixes from the unshifted softmax's probabilities, training from the raw logits: other operands from step 1 on."""
    p, d, video, *_ = tc.case(oracle, "small-odd")
    ids1, l1 = tc.generate(oracle, p, d, video, weights_mode=1)
    ids0, l0 = tc.generate(oracle, p, d, video, weights_mode=0)
    B = video.shape[0]
    assert np.array_equal(l1[:B], l0[:B]) and not np.array_equal(l1[B:2 * B], l0[B:2 * B])
    one, _ = tc.generate(oracle, p, d, video[2:3], weights_mode=1)
    assert np.array_equal(one[0], ids1[2])
