"""The operand families of tests/pick_screen1_cases.py do what the GPU tests of the one-product pick screen need them to do, shown with a
numpy emulation of the bf16 product (no GPU): the worst-cast family reaches the per-term bound the margin constant C1 is built on, the
uniform family stays far inside it, and the three-product constant 2^-10 would NOT cover the one-product error -- a build that switched the
product but not the constant is caught by the GPU test that asserts C1."""
import numpy as np
import pytest

import pick_screen1_cases as ps

R, V = 9, 40                                      # the property is per term: a few outputs show it


@pytest.mark.parametrize("K", ps.PRODUCT_K)
def test_worst_cast_family_reaches_the_cast_bound(K):
    h, W = ps.product_inputs("worst-cast", R, K, V)
    assert ((h.view(np.uint32) & 0xFFFF) == 0x7FFF).all() and ((W.view(np.uint32) & 0x7FFFFF) == 0x7FFF).all() and (h > 0).all() and (W > 0).all()
    over_norms, over_mass = ps.ratios(ps.product_emulated(h, W), h, W)
    print(f"K={K}: emulated |L1 - L| max {over_mass / 2.0 ** -7:.4f} x 2^-7 of sum |h_k w_k|, {over_norms / ps.bound(K):.4f} of C1 ceil(K / 1024) over |h||w|")
    assert over_mass >= 0.9 * 2.0 ** -7, "the family does not stress the two casts"
    assert over_mass < 2.0 ** -7, "two RNE casts of a term miss by less than 2^-7 of it"
    assert over_norms <= ps.bound(K)


@pytest.mark.parametrize("K", ps.PRODUCT_K)
def test_three_product_constant_would_not_cover_one_product(K):
    h, W = ps.product_inputs("worst-cast", R, K, V)
    over_norms, _ = ps.ratios(ps.product_emulated(h, W), h, W)
    assert over_norms > ps.C3 * ((K + 1023) // 1024), "a margin built on 2^-10 would still hold: the family cannot tell the constants apart"


@pytest.mark.parametrize("K", ps.PRODUCT_K)
def test_uniform_family_stays_below_half_the_constant(K):
    h, W = ps.product_inputs("uniform", R, K, V)
    over_norms, _ = ps.ratios(ps.product_emulated(h, W), h, W)
    print(f"K={K}: uniform, emulated max |L1 - L| / (|h||w|) = {over_norms:.3e} = {over_norms / ps.c1():.4f} of C1")
    assert over_norms <= ps.c1() / 2


def test_all_ones_family_casts_up_by_an_fp32_ulp():
    h, W = ps.product_inputs("all-ones", R, 1024, V)
    assert ((h.view(np.uint32) & 0x7FFFFF) == 0x7FFFFF).all() and ((W.view(np.uint32) & 0x7FFFFF) == 0x7FFFFF).all()
    _, over_mass = ps.ratios(ps.product_emulated(h, W), h, W)
    assert over_mass < 2.0 ** -22


def test_accumulation_share_is_the_derived_one():
    """2^-11 per 1024 steps holds the K-proportional terms: K 2^-24 of the fp32 chain + K 2^-22 (1 + 2^-8)^2 of the accumulation = 3.1e-4 at K = 1024."""
    assert ps.acc1() == 2.0 ** -11
    assert 1024 * 2.0 ** -24 + 1024 * 2.0 ** -22 * (1 + 2.0 ** -8) ** 2 < 2.0 ** -11


@pytest.mark.parametrize("family", ps.FAMILIES)
@pytest.mark.parametrize("K", ps.PRODUCT_K)
def test_measured_margin_covers_the_casts_and_is_tighter_on_ordinary_operands(K, family):
    h, W = ps.product_inputs(family, R, K, V)
    true = h.astype(np.float64) @ W.astype(np.float64)
    err = np.abs(ps.product_emulated(h, W) - true)
    m1 = ps.margin_m1(h, W)
    share = float((m1 / (ps.bound(K) * ps.product_scale(h, W))).max())
    print(f"{family} K={K}: emulated |L1 - L| max {float((err / m1).max()):.3f} of m1; m1 max {share:.3f} of C1 ceil(K / 1024) |h||w|")
    assert (err <= m1).all()
    if family == "uniform":
        assert share < 0.5, "on ordinary operands the measured margin is less than half the a-priori one"
    if family == "worst-cast":
        assert float((err / m1).max()) > 0.7, "the family does not come near the measured margin"


def test_worst_cast_sampler_case_keeps_sign_and_bf16_mantissa():
    rng = np.random.default_rng(3)
    W = rng.uniform(-0.1, 0.1, (17, 23)).astype(np.float32)
    p = {"embed_word_W": W.copy()}
    ps.apply_worst_cast(p)
    got = p["embed_word_W"]
    assert (np.sign(got) == np.sign(W)).all() and ((got.view(np.uint32) >> 16) == (W.view(np.uint32) >> 16)).all()
    assert ((got.view(np.uint32) & 0xFFFF) == 0x7FFF).all()
    assert (np.abs(ps.bf16_rne(got)) < np.abs(got)).all(), "every cast rounds towards zero"
