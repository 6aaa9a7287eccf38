"""The cases of tests/pick_margin_cases.py have the properties that make tests/test_gpu_pick_margins.py discriminate -- conditions on the
INPUTS, checked with numpy and the CPU oracle alone: the adversarial product operands are what they are said to be, the H lines select the
resolve_listed instantiations they name, the overflow cases' survivor sets under the kernel's own margin formula are the stated ones, the
huge column overflows the norm and no logit, and the shifted-bias case does contain near-ties and an exact tie."""
import numpy as np
import pytest

import pick_margin_cases as pm


def _case(oracle, dims, nB, pseed=1):
    """tests/test_gpu_pick_screen.py::_case (that module is GPU-marked as a whole; the same inputs, restated)."""
    d = oracle.Dims(*dims, label_dim=0)
    p = oracle.init_params(d, seed=pseed)
    rng = np.random.default_rng(100 + nB)
    video = np.abs(rng.standard_normal((nB, d.n_video_lstm_step, d.dim_image)) * 0.5).astype(np.float32)
    return d, p, video


def test_constants_are_read_from_the_sources():
    assert 0.0 < pm.gumbel_screen_margin() < 0.1
    assert pm.resolve_list_capacity() == (2048, 4096, 12288)
    w = pm.gumbel_words()
    assert w.dtype == np.uint32 and len(w) == 1 << 23 and w[-1] == 0xFFFFFE00 and len(np.unique(w >> 9)) == 1 << 23
    ref = pm.gumbel_float64()
    assert np.isfinite(ref).all() and np.all(np.diff(ref) > 0)          # u in (0, 1) strictly: both logs finite, noise increasing in k
    assert abs(ref[0] + np.log(24 * np.log(2.0))) < 1e-12 and abs(ref[-1] - 24 * np.log(2.0)) < 1e-6


@pytest.mark.parametrize("R,H,V", pm.PRODUCT_SHAPES)
def test_product_families(R, H, V):
    assert pm.product_bound_C(H) == 2.0 ** -10 * (1 if H <= 1024 else 2)
    share = {}
    for fam in ("uniform", "all-ones", "split-worst"):
        h, W = pm.product_inputs(fam, R, H, V)
        assert h.shape == (R, H) and W.shape == (H, V) and h.dtype == W.dtype == np.float32
        share[fam] = float((np.abs(h.astype(np.float64)) @ np.abs(W.astype(np.float64)) / pm.product_scale(h, W)).min())
        if fam == "uniform":
            continue
        assert (h > 0).all() and (W > 0).all()
        frac = {int(x) for x in np.unique(h.view(np.uint32) & 0x7FFFFF)} | {int(x) for x in np.unique(W.view(np.uint32) & 0x7FFFFF)}
        assert frac == ({0x7FFFFF} if fam == "all-ones" else {pm.SPLIT_WORST_FRACTION})
        assert len(np.unique(np.frexp(h)[1])) == 3 and len(np.unique(np.frexp(W)[1])) == 3        # adjacent exponents, all drawn
        # what the three kept products miss of each term, relative to the term: h w - (hh wh + hh wl + hl wh), float64 (exact: 48 bits)
        (hh, hl), (wh, wl) = pm.bf16_split(h[0]), pm.bf16_split(W[:, 0])
        f = np.float64
        miss = (f(h[0]) * f(W[:, 0]) - (f(hh) * f(wh) + f(hh) * f(wl) + f(hl) * f(wh))) / (f(h[0]) * f(W[:, 0]))
        if fam == "all-ones":
            assert np.all(hh + hl == h[0]) and np.all(np.abs(miss) <= 2.0 ** -44)                 # the split is exact: only lo x lo is missing
        else:
            assert np.all(miss > 2.0 ** -15 * 0.95) and np.all(miss <= 2.0 ** -15)                # 2^-16 (lo x lo) + 2 x 2^-17, one sign
    # nothing cancels in the positive families: the product itself is sum |h_k w_k|, and that stays near |h| |w| (three equally likely
    # exponents: (7/3)^2 / 7 = 0.78 in expectation); the uniform family's product is a zero-mean sum, far below both
    assert share["all-ones"] > 0.7 and share["split-worst"] > 0.7
    h, W = pm.product_inputs("uniform", R, H, V)
    assert float((np.abs(h.astype(np.float64) @ W.astype(np.float64)) / pm.product_scale(h, W)).mean()) < 0.05


def test_h_lines_select_the_instantiations():
    assert [pm.resolve_form(H) for H in pm.H_LINES] == [(4, 35, 140, 192, 1), (8, 33, 260, 320, 1), (16, 33, 516, 576, 1),
                                                       (16, 64, 1024, 1024, 1), (32, 33, 1028, 1088, 2)]
    assert (pm.V_LINES + 3) // 4 * 4 == 304
    assert pm.H_LINES[0] % 4 != 0 and {pm.resolve_form(H)[0] for H in pm.H_LINES} == {4, 8, 16, 32}


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_overflow_survivor_sets(case):
    chunk, cap, regs = pm.resolve_list_capacity()
    V, Tc, bias = pm.overflow_bias(case)
    alive = pm.greedy_survivors(bias)
    count, winner = pm.OVERFLOW_EXPECT[case]
    assert len(alive) == count and int(np.argmax(bias)) == winner and Tc <= 4
    rounds = pm.overflow_flushes(case)
    if case == "a":
        assert V == 6148 <= regs and np.array_equal(alive, np.arange(cap)) and rounds is None      # the one list, full
    elif case == "d":
        assert V == 12292 > regs and len(alive) == V
        assert [len(r) for r in rounds] == [cap, cap, cap, 4] and sum(rounds, []) == list(range(V))
    else:
        assert V == 6148 and np.array_equal(alive, np.r_[np.arange(cap), V - 1])                   # one more than the list holds
        assert rounds == [list(range(cap)), [V - 1]] and (V - 1) // chunk * chunk == V - 4         # the last flush: a chunk of 4 columns
        assert [i for i, r in enumerate(rounds) if winner in r] == ([1] if case == "b" else [0])   # the flush that holds the winner
    # the margin that decides it: 2 (1e-3 + (rabs + 1) 2^-20); a column 2^-10 below the maximum survives, one at -10 does not
    mg = float(pm.screen_margin(np.abs(bias).max()))
    assert 2.0 ** -10 < mg < 1.0 and abs(mg - 2 * (pm.gumbel_screen_margin() + (float(np.abs(bias).max()) + 1) * 2.0 ** -20)) < 1e-8


def test_masked_token_case(oracle):
    d, p, video = _case(oracle, pm.SMALL, pm.B)
    pm.apply_masked_token(p)
    ids_s, ids_g, logits = oracle.sample_captions(p, d, video, K=pm.K, seed=7, return_logits=True)
    assert np.all(np.isneginf(logits[:, :, pm.MASKED])) and np.isfinite(np.delete(logits, pm.MASKED, axis=2)).all()
    assert (ids_s != pm.MASKED).all() and (ids_g != pm.MASKED).all()


def test_huge_column_overflows_the_norm_and_no_logit(oracle):
    d, p, video = _case(oracle, pm.SMALL, pm.B)
    pm.apply_huge_column(p)
    w = p["embed_word_W"][:, pm.HUGE_COLUMN]
    fmax = float(np.finfo(np.float32).max)
    assert np.isfinite(w).all()
    # pick_screen_prepare_kernel sums the squares of rows k = w (mod 4) per wave: each of the four partial sums overflows by itself
    assert all(float((w[q::4].astype(np.float64) ** 2).sum()) > 2 * fmax for q in range(4))
    assert np.isfinite(p["embed_word_b"]).all()
    ids_s, ids_g, logits = oracle.sample_captions(p, d, video, K=pm.K, seed=7, return_logits=True)
    assert np.isfinite(logits).all()
    assert np.abs(logits[:, :, pm.HUGE_COLUMN]).min() > 1e10                                    # that column decides every row, either way
    took = np.r_[ids_s.ravel(), ids_g.ravel()] == pm.HUGE_COLUMN
    assert took.any() and not took.all()


def test_shifted_bias_case_has_near_ties_and_a_tie(oracle):
    d, p, video = _case(oracle, pm.SMALL, pm.SLACK_B)
    pm.apply_bias_shift(p)
    near, ties, lo, hi, ids, want = pm.near_ties(oracle, p, d, video, pm.SLACK_K, pm.SLACK_SEED)
    print(f"{(pm.SLACK_K + 1) * pm.SLACK_B} rows, seed {pm.SLACK_SEED}: {near} sampled (row, step) pairs within 2 ulp, {ties} exact ties; winning keys in [{lo}, {hi}]")
    assert (pm.SLACK_K + 1) * pm.SLACK_B <= 195
    assert 8192.0 <= lo and hi < 16384.0 and np.spacing(np.float32(lo)) == 2.0 ** -10               # one ulp = 2^-10 <= kGumbelScreenMargin
    assert 2.0 ** -10 <= pm.gumbel_screen_margin()
    assert near >= 3 and ties >= 1
    assert np.array_equal(ids, want)                                                               # the oracle's rule: the lowest column of equal keys
