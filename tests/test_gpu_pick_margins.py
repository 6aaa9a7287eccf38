"""The two bounds the sampler's pick screens are exact under, and the resolve kernel's paths no other test reaches (cases:
tests/pick_margin_cases.py, their discriminating properties: tests/test_pick_margin_cases_cpu.py).

1. kGumbelScreenMargin (csrc/detmath.h): both Gumbel forms over all 2^23 noise words against float64.
2. m = C |h| max|w| (csrc/pick_screen.hip): the split-bf16 product against the fp32 chain on operands whose errors add up, and above K = 1024.
3. resolve_listed<4 / 8 / 16 / 32>, ldt != H, C x 2: ids at the H lines.
4. The overflow path: the list at capacity, one survivor more, the winner in the first and in the last flush, the memory form.
5. The every-column path: a -inf bias, a column norm that overflows.
6. The magnitude slack: keys in [8192, 16384), with near-ties and an exact tie.

Every sampler call runs on tests/test_gpu_pick_screen.py's guarded, dirtied, exact-size scratch blocks."""
import ctypes as C

import numpy as np
import pytest

import pick_margin_cases as pm
from test_gpu_pick_screen import _Sampler, _case, _dev

pytestmark = pytest.mark.gpu


def _both_against_the_oracle(oracle, s, p, d, video, nK, seed):
    """Screened ids == s2vt_sample's == the oracle's; returns (sampled, greedy, (total, most, every))."""
    got_s, got_g = s.screened(seed)
    counters = s.counters()
    ref_s, ref_g = s.plain(seed)
    assert np.array_equal(got_g, ref_g), "greedy ids differ from s2vt_sample's"
    assert np.array_equal(got_s, ref_s), "sampled ids differ from s2vt_sample's"
    orc_s, orc_g = oracle.sample_captions(p, d, video, K=nK, seed=seed)
    assert np.array_equal(ref_g, orc_g), "s2vt_sample's greedy ids differ from the oracle's"
    assert np.array_equal(ref_s, orc_s), "s2vt_sample's sampled ids differ from the oracle's"
    return got_s, got_g, counters


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
def test_gumbel_forms_over_the_whole_domain(gpu):
    """All 2^23 words.  Asserted: both forms finite, max |fast - exact| <= kGumbelScreenMargin / 50 (the header's claim).  Printed: the worst
    |fast - exact| and |exact - float64| with their k, and the worst of the last 2^10 words (u -> 1, the largest noise) on their own."""
    import torch
    L = __import__("s2vt_amd").lib()
    z = torch.zeros(4, dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    assert L.s2vt_gumbel_words_eval(None, P(z), P(z), 4, None) == -1 and L.s2vt_gumbel_words_eval(P(z), None, P(z), 4, None) == -1
    assert L.s2vt_gumbel_words_eval(P(z), P(z), None, 4, None) == -1 and L.s2vt_gumbel_words_eval(P(z), P(z), P(z), -1, None) == -1
    assert L.s2vt_gumbel_words_eval(P(z), P(z), P(z), 0, None) == 0
    words = pm.gumbel_words()
    exact, fast = (t.cpu().numpy() for t in gpu.gumbel_words_eval(_dev(words.view(np.int32))))
    assert np.isfinite(exact).all() and np.isfinite(fast).all()
    ref = pm.gumbel_float64()
    d_fast, d_ref = np.abs(fast.astype(np.float64) - exact), np.abs(exact - ref)
    kf, kr = int(d_fast.argmax()), int(d_ref.argmax())
    margin = pm.gumbel_screen_margin()
    print(f"max |fast - exact| = {d_fast[kf]:.3e} at k = {kf} (exact {exact[kf]!r}, fast {fast[kf]!r}): margin / {margin / d_fast[kf]:.1f}")
    print(f"max |exact - float64| = {d_ref[kr]:.3e} at k = {kr} (exact {exact[kr]!r}, float64 {ref[kr]!r})")
    tail = slice(pm.GUMBEL_WORDS - 1024, None)
    print(f"last 1024 words (u -> 1): max |fast - exact| = {d_fast[tail].max():.3e}, max |exact - float64| = {d_ref[tail].max():.3e}; "
          f"first 1024: {d_fast[:1024].max():.3e}, {d_ref[:1024].max():.3e}")
    assert d_fast[kf] <= margin / 50


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["uniform", "all-ones", "split-worst"])
@pytest.mark.parametrize("R,H,V", pm.PRODUCT_SHAPES)
def test_split_product_stays_inside_the_margin(gpu, R, H, V, family):
    """max |L~ - L| / (|h| |w|) <= C = 2^-10 ceil(H / 1024) (uniform operands: C / 8), L~ the split-bf16 product, L the fp32 chain: what m
    has to cover.  Printed: that share of C, and both products' own error against the float64 product, over |h| |w| and over sum |h_k w_k|."""
    import torch
    import s2vt_amd
    from s2vt_amd import _lib
    L = s2vt_amd.lib()
    h, W = pm.product_inputs(family, R, H, V)
    hd, Wd = _dev(h), _dev(W)
    Hp = (H + 63) // 64 * 64
    P = lambda t: C.c_void_p(t.data_ptr())
    hh, hl = (torch.empty((R, Hp), dtype=torch.int16, device="cuda") for _ in range(2))
    Wh, Wl = (torch.empty((V, Hp), dtype=torch.int16, device="cuda") for _ in range(2))
    assert L.s2vt_cast_bf16_split(P(hd), H, None, R, H, 0, P(hh), P(hl), Hp, 0, None, None, None, 0, None, 0, None) == 0
    assert L.s2vt_cast_bf16_split(P(Wd), V, None, H, V, 1, P(Wh), P(Wl), Hp, Hp, None, None, None, 0, None, 0, None) == 0
    approx = torch.empty((R, V), dtype=torch.float32, device="cuda")
    assert L.s2vt_gemm_bf16x3_nt(P(hh), P(hl), Hp, P(Wh), P(Wl), Hp, P(approx), V, R, V, Hp, 0, None, 0, None) == 0
    chain = torch.empty((R, V), dtype=torch.float32, device="cuda")
    seg = _lib.Operand(hd.data_ptr(), None, H, H, 0, 0)
    assert L.s2vt_gemm(C.byref(seg), 1, P(Wd), V, None, None, 0, P(chain), V, R, V, 0, -1, None) == 0
    torch.cuda.synchronize()
    approx, chain = approx.cpu().numpy().astype(np.float64), chain.cpu().numpy().astype(np.float64)
    true = h.astype(np.float64) @ W.astype(np.float64)
    scale, mass = pm.product_scale(h, W), np.abs(h.astype(np.float64)) @ np.abs(W.astype(np.float64))
    Cb = pm.product_bound_C(H)
    ratio = float((np.abs(approx - chain) / scale).max())
    print(f"{family} R={R} H={H} V={V}: max |L~ - L| / (|h||w|) = {ratio:.3e} = {ratio / Cb:.3e} of C; against float64, over |h||w|: "
          f"split {float((np.abs(approx - true) / scale).max()):.3e}, chain {float((np.abs(chain - true) / scale).max()):.3e}; over sum|h_k w_k|: "
          f"split {float((np.abs(approx - true) / mass).max()):.3e}, chain {float((np.abs(chain - true) / mass).max()):.3e}")
    assert ratio <= (Cb / 8 if family == "uniform" else Cb)


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", pm.H_LINES)
def test_ids_at_the_h_lines(gpu, oracle, H):
    """resolve_listed<CH> at H = 137 (CH 4, ldt = 140 != H, ldl = 304 != V), 260 (CH 8), 516 and 1024 (CH 16: 33 and all 64 lanes),
    1028 (CH 32, C x 2, Hp = 1088).  Every one of these H is accepted as it is."""
    d, p, video = _case(oracle, pm.dims(pm.V_LINES, H, 3), pm.B)
    s = _Sampler(gpu, d, p, video, pm.B, pm.K)
    assert s.rows == 65
    _, _, (total, most, every) = _both_against_the_oracle(oracle, s, p, d, video, pm.K, 7)
    print(f"H={H}: survivors per row: mean {total / (s.rows * s.Tc):.3f}, most {most}; rows that took every column: {every}")
    assert every == 0 and most < s.V and total >= s.rows * s.Tc


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_overflow_path_capacity_and_flush_order(gpu, oracle, case):
    """Zero weights, so an argmax row's survivors are set by the biases alone: a. exactly kResList of them (the one list, full); b. one
    more, the winner alone in the final flush of a 4-column chunk; c. the winner in the first flush; d. every column, memory form."""
    V, Tc, _ = pm.overflow_bias(case)
    d, p, video = _case(oracle, pm.dims(V, 136, Tc), pm.B)
    pm.apply_overflow(p, case)
    s = _Sampler(gpu, d, p, video, pm.B, pm.K)
    _, got_g, (total, most, every) = _both_against_the_oracle(oracle, s, p, d, video, pm.K, 2)
    count, winner = pm.OVERFLOW_EXPECT[case]
    print(f"case {case}: V={V}, survivors total {total}, most {most}; rows that took every column: {every}")
    assert (got_g == winner).all(), f"an argmax row did not take column {winner}"
    assert most == count and every == 0
    assert total >= pm.B * s.Tc * count


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["masked-token", "huge-column"])
def test_every_column_path(gpu, oracle, case):
    """A -inf bias (a masked token: every fast key row holds a non-finite key) and a column of embed_word_W whose squared norm overflows fp32
    (nwmax = inf, so the margin is; every logit finite): each row of each step resolves all V columns exactly."""
    d, p, video = _case(oracle, pm.SMALL, pm.B)
    (pm.apply_masked_token if case == "masked-token" else pm.apply_huge_column)(p)
    s = _Sampler(gpu, d, p, video, pm.B, pm.K)
    got_s, got_g, (total, most, every) = _both_against_the_oracle(oracle, s, p, d, video, pm.K, 7)
    print(f"{case}: survivors total {total}, most {most}; rows that took every column: {every} of {s.rows * s.Tc}")
    if case == "masked-token":
        assert (got_s != pm.MASKED).all() and (got_g != pm.MASKED).all()
    assert every == s.rows * s.Tc and most == s.V and total == s.rows * s.Tc * s.V


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
def test_keys_in_the_last_binade_the_margin_covers(gpu, oracle):
    """embed_word_b + 12000: keys in [8192, 16384), one ulp = 2^-10, the largest that kGumbelScreenMargin still covers.  The case holds sampled
    rows whose two best exact keys lie within 2 ulp, one pair equal (asserted on the CPU); both samplers give the oracle's ids, the lowest column on a tie."""
    d, p, video = _case(oracle, pm.SMALL, pm.SLACK_B)
    pm.apply_bias_shift(p)
    s = _Sampler(gpu, d, p, video, pm.SLACK_B, pm.SLACK_K)
    _, _, (total, most, every) = _both_against_the_oracle(oracle, s, p, d, video, pm.SLACK_K, pm.SLACK_SEED)
    print(f"survivors per row: mean {total / (s.rows * s.Tc):.3f}, most {most}; rows that took every column: {every}")
    assert every == 0          # (rabs ~ 12000 widens the margin to 2 (m + 1e-3 + 0.0114): a row whose logits all lie within it keeps all V columns)
