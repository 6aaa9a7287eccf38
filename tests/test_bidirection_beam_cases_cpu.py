"""tests/bidirection_beam_cases.py on the CPU: the sharpened case gives a beam search something to decide, so a GPU search that equals
an independent driver on it has been through a changed caption, both exits of the loop and a shared parent; and the helpers the GPU tests
lean on restate what they say they restate."""
import numpy as np

import bidirection_beam_cases as C
import bidirection_cases as BC


def test_the_sharpened_case_discriminates_at_beam_3(oracle):
    p, d, video = C.case(oracle)
    differ, early, full, shared = C.figures(oracle, p, d, video, 3)
    print(f"\nbeam 3 at the sharpened case: {differ} of {video.shape[0]} captions differ from greedy, {early} end on <eos> before Tc, "
          f"{full} run all {d.n_caption_lstm_step} steps, {shared} steps with a shared parent")
    assert (differ, early, full, shared) == (5, 2, 3, 29)         # the scan's row (module docstring of bidirection_beam_cases)
    assert differ >= 1 and early >= 1 and full >= 1 and shared >= 1


def test_the_sharpened_case_is_peaked(oracle):
    """why the case is sharpened: at bidirection_cases' own parameters the first step's best word has about 1 / V of the mass"""
    q, d, v, *_ = BC.case(oracle, C.BASE)
    p, _, video = C.case(oracle)
    flat = np.exp(C.topk(C.cpu_step(oracle, q, d, v[2])(0, [[]]), 1)[1][0, 0])
    sharp = np.exp(C.topk(C.cpu_step(oracle, p, d, video[2])(0, [[]]), 1)[1][0, 0])
    assert flat < 2.0 / d.n_words and sharp > 20.0 / d.n_words


def test_beam_1_of_the_cpu_search_is_the_greedy_restatement(oracle):
    p, d, video = C.case(oracle)
    ids, _ = BC.greedy(oracle, p, d, video, np.arange(video.shape[0], dtype=np.int32))
    beam, _ = C.cpu_beam(oracle, p, d, video, 1)
    Tc = d.n_caption_lstm_step
    for j, (s, lp, sc) in enumerate(beam):
        g = ids[j].tolist()
        n = g.index(0, 1) + 1 if 0 in g[1:] else Tc               # up to and including the first <eos> behind the first word
        assert s == g[:n], j


def test_topk_order_and_normaliser():
    l = np.array([[0.5, 2.0, 2.0, -1.0, 2.0], [3.0, 3.0, 1.0, 0.0, 3.5]], np.float32)
    ids, lp = C.topk(l, 3)
    assert ids.tolist() == [[1, 2, 4], [4, 0, 1]]                 # value descending, index ascending on ties
    assert np.allclose(np.exp(C.topk(l, 5)[1].astype(np.float64)).sum(1), 1.0, atol=1e-6)
    assert lp[0, 0] == lp[0, 1] == lp[0, 2]


def test_helpers_restate_bidirection_cases(oracle):
    dims, B = BC.SHAPES["small-odd"]
    p, d, video = C.make(oracle, dims, B)
    q, _, v, cap, vid, sid = BC.case(oracle, "small-odd")
    assert all(np.array_equal(p[n], q[n]) for n in q) and np.array_equal(video, v)
    full = BC.teacher_forced(oracle, q, d, v, cap, vid, sid)
    assert np.array_equal(C.first_steps(oracle, q, d, v, cap, 4), full[:, :4])
