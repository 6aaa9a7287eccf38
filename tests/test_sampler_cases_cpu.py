"""The sampler cases of tests/sampler_cases.py discriminate -- a condition on the INPUTS of tests/test_gpu_decode_loop_edges.py, checked on the
CPU oracle alone: every mutant (a dropped K tail, hidden unit, embedding column: what a subtly wrong decode kernel would compute) changes
at least one of the oracle's ids, the greedy rows differ between videos, the draws are not all equal.  The same counts are printed, not
asserted, for SAMPLE_CASES of tests/test_gpu_fwd.py (default-scale weights): there most of them are zero.

Ids changed per mutant, in the order of sampler_cases.MUTANTS (embed_word_W tail group, embed_word_W last row, lstm2_W recurrent tail group,
lstm2_W last recurrent row, Wemb last column, gate columns of unit H - 1), of the (K + g) B Tc ids of the case (run with -s to print them):

    V8-E1-H132-Tc1-B16-K1-g1 (tiny)     11  10   6   6  12  10  of  32
    V16-E1-H132-Tc2-B16-K0-g1 (tiny)    10  15   8   5  22  15  of  32
    V52-E5-H136-Tc3-B16-K3-g1           41  14  22   3  81  15  of 192
    V48-E16-H140-Tc4-B32-K1-g1         127  15  95   5 128  16  of 256
    V100-E17-H144-Tc3-B48-K0-g1         99  31  52   8  66  28  of 144
    V200-E7-H260-Tc3-B64-K0-g1          32   7  13  10  45  27  of 192
    V12288-E3-H132-Tc2-B16-K1-g1        17   9  12   6  14  15  of  64
    V12284-E129-H260-Tc3-B32-K1-g1     102  38  41  14 117  36  of 192
    V1000-E33-H1004-Tc3-B16-K2-g1       33   3  34   5  51   9  of 144
    V1000-E128-H1008-Tc2-B32-K1-g1      82   3  24   5  95   6  of 128
    V300-E12-H500-Tc3-B16-K3-g0         12   6  17   6  28   9  of 144
    V300-E12-H500-Tc3-B32-K2-g0         36   7  13   4  51  15  of 192
    V200-E5-H132-Tc2-B16-K16-g1        108  23  58  10 209  21  of 544
    V200-E9-H260-Tc2-B48-K6-g1         105  57  55  19 178  32  of 672
    V200-E5-H136-Tc2-B100-K2-g1        191  82  82  24 280  68  of 600
  not asserted -- test_gpu_fwd.SAMPLE_CASES, oracle.init_params as it is:
    V97-E12-H20-Tc6-B3-K2                0   0   0   0   0   0  of  54   (one greedy id)
    V260-E32-H64-Tc8-B4-K3              31   1   1   1   0   1  of 128   (two greedy ids)
    V12000-E500-H1000-Tc20-B2-K2        13  12  17   1   4  13  of 120
"""
import numpy as np
import pytest

import sampler_cases as sc

ALL = sc.CASES + sc.BIG_CASES + sc.DEC4_ONLY_CASES


def test_at_most_two_tiny_cases_and_every_case_in_its_window():
    assert sum(c.tiny for c in ALL) <= 2
    for c in sc.CASES:
        assert sc.rows(c) <= 64 and c.B in (16, 32, 48, 64)
    for c in sc.BIG_CASES:
        assert 256 < sc.rows(c) <= 384 and c.B % 16 == 0
    for c in sc.DEC4_ONLY_CASES:
        assert 256 < sc.rows(c) <= 384
    for c in ALL:           # decode_loop_eligible / decode4_eligible
        assert c.H % 4 == 0 and 132 <= c.H <= 1008 and c.E >= 1 and c.V % 4 == 0 and c.V <= 12288


@pytest.mark.parametrize("case", ALL, ids=sc.case_id)
def test_every_mutant_changes_the_oracle_ids(oracle, case):
    base = sc.run_oracle(case, oracle)
    counts = [sc.ids_changed(base, sc.run_oracle(case, oracle, m)) for m in sc.MUTANTS]
    print(f"\n{sc.case_id(case)}: ids changed per mutant {counts} of {sc.rows(case) * case.Tc}")
    if case.tiny:
        assert sum(n > 0 for n in counts) >= 3, counts
    else:
        assert all(n > 0 for n in counts), counts
    s, g = base
    if case.with_greedy and not case.tiny:
        assert len({tuple(r) for r in g}) >= 2 and len(np.unique(g)) >= 3
    if case.K > 0:
        assert len(np.unique(s)) > 1


def test_print_mutant_counts_of_the_default_initialisation(oracle):
    """On record, not asserted: the same mutants on the inputs of test_gpu_fwd.py::test_sampler_token_ids_bit_exact."""
    from test_gpu_fwd import SAMPLE_CASES
    for case in SAMPLE_CASES:
        d = oracle.Dims(label_dim=0, **case["dims"])
        p = oracle.init_params(d, seed=3)
        rng = np.random.default_rng(9)
        for k in ("lstm1_b", "lstm2_b", "encode_image_b", "embed_word_b"):
            p[k] = rng.uniform(-.1, .1, p[k].shape).astype(np.float32)
        B, K = case["B"], case["K"]
        video = np.abs(rng.standard_normal((B, d.n_video_lstm_step, d.dim_image)) * 0.5).astype(np.float32)
        base = oracle.sample_captions(p, d, video, K, seed=2024, video_base=10)
        counts = [sc.ids_changed(base, oracle.sample_captions(m(p), d, video, K, seed=2024, video_base=10)) for m in sc.MUTANTS]
        print(f"\nSAMPLE_CASES V{d.n_words}-E{d.word_dim}-H{d.lstm_dim}-Tc{d.n_caption_lstm_step}-B{B}-K{K}: ids changed per mutant {counts} of "
              f"{(K + 1) * B * d.n_caption_lstm_step}; distinct greedy ids {len(np.unique(base[1]))}")
