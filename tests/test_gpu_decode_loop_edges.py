"""The sampler's persistent decode loop (csrc/decode_loop.hip) against the CPU oracle at the edges of the window it admits -- H 132 / 260 / 1008,
E below one k-group and one past one, V 8 .. 12288 (one column tile, a workgroup boundary, a partial last tile, every workgroup full), one
decode step, B = 48, no greedy rows -- on inputs whose ids REACT to the decode state (tests/sampler_cases.py; tests/test_sampler_cases_cpu.py
shows that dropping a K tail, a hidden unit or an embedding column changes the oracle's ids at every case).  Every comparison is np.array_equal on
token ids, and the launch profiler must have seen the persistent form: a fall-back to per-step launches cannot make a test pass.
Also: exact ties between columns owned by different workgroups (the 64-bit atomic-max key) incl. all-negative logits, stale state on the shared
workspace, a busy second stream, and the opt-in 257-384-row forms (S2VT_DECLOOP=2, S2VT_DEC4=1) at small widths."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import sampler_cases as sc

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(sampled, greedy) ids of the oracle: computed once per case, shared by the tests, never written to."""
    from oracle import s2vt_oracle
    s, g = sc.run_oracle(case, s2vt_oracle)
    s.setflags(write=False)
    if g is not None:
        g.setflags(write=False)
    return s, g


def _sample(gpu, d, p, video, K, seed, base, with_greedy=True):
    """ops.sample with the launch profiler on -> (sampled, greedy | None, names of the profiled launches)."""
    import torch
    dims = gpu.make_dims(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step)
    dp = {k: _dev(v) for k, v in p.items()}
    gpu.prof_filter(-1, -1); gpu.prof_enable(True)
    try:
        s, g = gpu.sample(dims, gpu.make_params(dp), _dev(video), K, seed=seed, video_base=base, with_greedy=with_greedy)
        torch.cuda.synchronize()
    finally:
        gpu.prof_enable(False)
    names = {r["name"] for r in gpu.prof_collect()}
    return s.cpu().numpy(), (None if g is None else g.cpu().numpy()), names


def _check_case(gpu, oracle, case, tag=""):
    ref_s, ref_g = _reference(case)
    d, p, video, seed, base = sc.build(case, oracle)
    s, g, names = _sample(gpu, d, p, video, case.K, seed, base, case.with_greedy)
    assert "decloop(m64)" in names, (tag, names)                       # the persistent launch, not 2 Tc launches
    assert gpu.chain_timeouts() == 0, tag
    assert s.shape == ref_s.shape and np.array_equal(s, ref_s), (tag, "sampled", int((s != ref_s).sum()))
    if case.with_greedy:
        assert np.array_equal(g, ref_g), (tag, "greedy", int((g != ref_g).sum()))
    else:
        assert g is None
    return s, g


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_decode_loop_ids_equal_oracle_at_window_edges(gpu, oracle, case):
    for rep in range(2):                                               # back to back: nothing stale from the first call
        _check_case(gpu, oracle, case, rep)


TIE_SETS = [(40, 41, 47, 48, 95, 96, 299), (47, 48), (96, 299)]       # 48 columns per workgroup: 47 | 48 and 95 | 96 are boundaries, 299 is in the seventh


def test_decode_loop_cross_workgroup_ties_and_negative_keys(gpu, oracle):
    """Identical columns of embed_word_W with the same bias have identical logits in every row and step; the argmax rows must take the
    lowest one although the candidates reach the pick word through atomic max operations of different workgroups, in any order -- also
    when every logit, hence the float half of every key, is negative."""
    V, E, H, Tc, B, K = 300, 5, 132, 4, 16, 1
    d = oracle.Dims(sc.D_IMAGE, V, E, H, sc.TV, Tc, 0)
    p0 = oracle.init_params(d, seed=3)                                 # default-scale weights: |h . W| stays far below the bias step of 3
    rng = np.random.default_rng(4)
    for k in ("lstm1_b", "lstm2_b", "encode_image_b", "embed_word_b"):
        p0[k] = rng.uniform(-.1, .1, p0[k].shape).astype(np.float32)
    video = np.abs(rng.standard_normal((B, sc.TV, sc.D_IMAGE)) * 0.5).astype(np.float32)

    def run(p, expect):
        ref_s, ref_g = oracle.sample_captions(p, d, video, K, seed=77, video_base=5)
        assert (ref_g == expect).all(), (expect, np.unique(ref_g))     # on the oracle first
        s, g, names = _sample(gpu, d, p, video, K, 77, 5)
        assert "decloop(m64)" in names, names
        assert np.array_equal(g, ref_g), (expect, np.unique(g))
        assert np.array_equal(s, ref_s)
        return ref_s, ref_g

    for cols in TIE_SETS:
        p = {k: v.copy() for k, v in p0.items()}
        for c in cols[1:]:
            p["embed_word_W"][:, c] = p["embed_word_W"][:, cols[0]]
        p["embed_word_b"][list(cols)] = 3.0
        _, ref_g = run(p, min(cols))
        # every logit negative: the same order through the keys of negative floats
        q = {k: v.copy() for k, v in p.items()}
        q["embed_word_b"] = (q["embed_word_b"] - np.float32(100.0)).astype(np.float32)
        logits = oracle.sample_captions(q, d, video, K, seed=77, video_base=5, return_logits=True)[2]
        assert logits.max() < 0
        _, neg_g = run(q, min(cols))
        assert np.array_equal(neg_g, ref_g)
    # one column far above the rest, in the last workgroup that owns any: every id, drawn or argmax, is V - 1
    p = {k: v.copy() for k, v in p0.items()}
    p["embed_word_b"][V - 1] = 50.0
    ref_s, _ = run(p, V - 1)
    assert (ref_s == V - 1).all()
    assert gpu.chain_timeouts() == 0


def test_decode_loop_stale_state_and_load(gpu, oracle):
    """The sampler workspace is shared by every call (ops.workspace: it only grows): a case, a smaller one with other strides, the first
    again -- every result its oracle's.  Then one case three times beside a stream of unrelated products: the same bits, no timeout."""
    import torch
    by_id = {sc.case_id(c): c for c in sc.CASES}
    a, b = by_id["V52-E5-H136-Tc3-B16-K3-g1"], by_id["V16-E1-H132-Tc2-B16-K0-g1"]
    for tag, case in (("first", a), ("smaller", b), ("again", a)):
        _check_case(gpu, oracle, case, tag)
    case = by_id["V200-E7-H260-Tc3-B64-K0-g1"]
    side = torch.cuda.Stream()
    x = torch.randn(2048, 2048, device="cuda")
    for rep in range(3):
        with torch.cuda.stream(side):
            for _ in range(3 + rep):
                x = torch.tanh(x @ x * 1e-3)                           # uneven load beside the loop's hand-offs
        _check_case(gpu, oracle, case, f"load{rep}")                   # (bits equal to one reference: equal to each other)
    torch.cuda.synchronize()
    assert gpu.chain_timeouts() == 0


# ---- the opt-in forms at 257-384 rows: the switches are read once per process, so each runs in a child
CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["S2VT_ROOT"]); sys.path.insert(0, os.path.join(os.environ["S2VT_ROOT"], "tests"))
import numpy as np, torch
import s2vt_amd
from s2vt_amd import ops
from oracle import s2vt_oracle as orc
import sampler_cases as sc
cases = sc.BIG_CASES + (sc.DEC4_ONLY_CASES if sys.argv[2] == "dec4" else [])
out, names = {}, set()
for i, c in enumerate(cases):
    d, p, video, seed, base = sc.build(c, orc)
    dims = ops.make_dims(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step)
    dp = {k: torch.as_tensor(v).cuda() for k, v in p.items()}
    ops.prof_filter(-1, -1); ops.prof_enable(True)
    s, g = ops.sample(dims, ops.make_params(dp), torch.as_tensor(video).cuda(), c.K, seed=seed, video_base=base)
    torch.cuda.synchronize()
    ops.prof_enable(False)
    names |= {r["name"] for r in ops.prof_collect()}
    out[f"s{i}"] = s.cpu().numpy(); out[f"g{i}"] = g.cpu().numpy()
out["timeouts"] = np.asarray(ops.chain_timeouts())
out["names"] = np.asarray(sorted(names))
np.savez(sys.argv[1], **out)
print("child ok")
'''


def test_optin_big_forms_equal_oracle_at_small_width(gpu, oracle):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env0 = {k: v for k, v in os.environ.items() if k not in ("S2VT_DECLOOP", "S2VT_DEC4")}
    with tempfile.TemporaryDirectory() as td:
        for mode, knob, want in (("loop", {"S2VT_DECLOOP": "2"}, ("decloop(m320)", "decloop(m384)")),
                                 ("dec4", {"S2VT_DEC4": "1"}, ("dec4(m320)", "dec4(m384)"))):
            f = os.path.join(td, f"{mode}.npz")
            # a child that faults or runs out of time ends the test here (TimeoutExpired / the assertion): the next one is not started
            r = subprocess.run([sys.executable, "-c", CHILD, f, mode], env=dict(env0, S2VT_ROOT=root, **knob), capture_output=True, text=True,
                               timeout=180)
            assert r.returncode == 0 and "child ok" in r.stdout, (mode, r.returncode, r.stderr[-3000:])
            res = dict(np.load(f))
            assert int(res["timeouts"]) == 0
            names = set(res["names"].tolist())
            for w in want:
                assert w in names, (mode, names)
            cases = sc.BIG_CASES + (sc.DEC4_ONLY_CASES if mode == "dec4" else [])
            for i, c in enumerate(cases):
                ref_s, ref_g = _reference(c)
                assert np.array_equal(res[f"s{i}"], ref_s), (mode, sc.case_id(c), "sampled")
                assert np.array_equal(res[f"g{i}"], ref_g), (mode, sc.case_id(c), "greedy")
