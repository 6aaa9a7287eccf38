"""pick_resolve_kernel on both sides of its 12288-column line (csrc/pick_screen.hip): up to 6 chunks of 2048 columns a thread keeps its
fast keys in registers, above that they go through memory as before.  Token ids against s2vt_sample and the oracle at |V| = 12288 (register
path, the last chunk full), 12292 (memory path) and 300 (register path, one partial chunk); at 12288 also the zero-weights construction of
tests/test_gpu_pick_screen.py -- every column of an argmax row survives, so the chunk-by-chunk overflow path runs on the registers --
and its near-tie construction.  H = 136, 65 rows, at most 4 caption steps throughout."""
import numpy as np
import pytest

from test_gpu_pick_screen import _Sampler, _case

pytestmark = pytest.mark.gpu

B, K = 13, 4                                  # 65 rows: 52 sampled, 13 greedy


def _dims(V, Tc):
    return (32, V, 16, 136, 2, Tc)            # (D, V, E, H, Tv, Tc)


@pytest.mark.parametrize("V,Tc", [(12288, 3), (12292, 3), (300, 4)], ids=["V12288-regs", "V12292-memory", "V300-regs"])
def test_ids_on_both_sides_of_the_line(gpu, oracle, V, Tc):
    d, p, video = _case(oracle, _dims(V, Tc), B)
    s = _Sampler(gpu, d, p, video, B, K)
    got_s, got_g = s.screened(7)
    total, most, every = s.counters()
    ref_s, ref_g = s.plain(7)
    assert np.array_equal(got_g, ref_g), "greedy ids differ from s2vt_sample's"
    assert np.array_equal(got_s, ref_s), "sampled ids differ from s2vt_sample's"
    orc_s, orc_g = oracle.sample_captions(p, d, video, K=K, seed=7, video_base=0)
    assert np.array_equal(got_g, orc_g), "greedy ids differ from the oracle's"
    assert np.array_equal(got_s, orc_s), "sampled ids differ from the oracle's"
    print(f"V={V}: survivors per row: mean {total / (s.rows * s.Tc):.3f}, most {most}; rows that took every column: {every}")
    assert total >= s.rows * s.Tc and most < V and every == 0          # the screen is live, and every row kept its fast winner


def test_zero_weights_overflow_path_on_registers(gpu, oracle):
    d, p, video = _case(oracle, _dims(12288, 2), B)
    p["embed_word_W"][:] = 0.0
    p["embed_word_b"][:] = 0.25
    s = _Sampler(gpu, d, p, video, B, K)
    got_s, got_g = s.screened(2)
    total, most, every = s.counters()
    ref_s, ref_g = s.plain(2)
    assert np.array_equal(got_g, ref_g) and np.array_equal(got_s, ref_s)
    assert (got_g == 0).all()
    assert most == s.V and every == 0                                   # an argmax row: all V keys are equal, none may be dropped
    assert total >= B * s.Tc * s.V


def test_near_ties_on_registers(gpu, oracle):
    d, p, video = _case(oracle, _dims(12288, 2), B)
    W = p["embed_word_W"]
    for j in range(1, 4):                                               # groups of four columns, 2^-20 apart: all of the winning group survive
        W[:, j::4] = W[:, 0::4] * np.float32(1.0 + j * 2.0 ** -20)
    s = _Sampler(gpu, d, p, video, B, K)
    got_s, got_g = s.screened(9)
    _, most, every = s.counters()
    ref_s, ref_g = s.plain(9)
    assert np.array_equal(got_g, ref_g) and np.array_equal(got_s, ref_s)
    assert most >= 4 and every == 0
