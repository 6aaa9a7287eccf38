"""The host ROUGE-L scorer (csrc_host/rouge.cpp through reward.RougeL.score_ids) against the string restatement of tests/rouge_cases.py,
bit for bit; its argument checks; the argument checks of the device entry, which answer without a GPU; and the host file under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program (nothing preloaded, nothing loaded into the interpreter)."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import rouge_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scorer(name, **kw):
    from s2vt_amd import reward
    c = RC.case(name)
    return c, reward.RougeL(c["refs_by_video"], c["wordtoix"], **kw)


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("name", RC.CASES)
def test_host_scores_equal_the_restatement_bit_for_bit(name, threads):
    c, sc = _scorer(name, n_threads=threads)
    got = sc.score_ids(c["ids"], c["video_of_row"])
    assert got.dtype == np.float32 and got.shape == (len(c["ids"]),)
    assert np.array_equal(got.view(np.uint32), RC.expected(name)["f32"].view(np.uint32))


def test_other_beta_follows_the_restatement():
    for beta in (0.5, 2.0):
        c, sc = _scorer("ragged", beta=beta)
        want = RC.score_rows(c, beta=beta)[0].astype(np.float32)
        assert np.array_equal(sc.score_ids(c["ids"], c["video_of_row"]).view(np.uint32), want.view(np.uint32))
        assert (want != RC.expected("ragged")["f32"]).any()


def test_bad_arguments():
    from s2vt_amd import reward
    c, sc = _scorer("ragged")
    for bad in (-1, 7):
        v = c["video_of_row"].copy()
        v[5] = bad
        with pytest.raises(ValueError):
            sc.score_ids(c["ids"], v)
    with pytest.raises(ValueError):                                 # a video without references: at construction
        reward.RougeL([["w1 w2"], [], ["w3"]], c["wordtoix"])
    with pytest.raises(RuntimeError):                               # built without `device`: no corpus on the GPU
        sc.score_ids_device(None, None)
    with pytest.raises(ValueError):
        reward.make_scorer("bleu", c["refs_by_video"], c["wordtoix"])
    assert isinstance(reward.make_scorer("rouge", c["refs_by_video"], c["wordtoix"]), reward.RougeL)
    assert isinstance(reward.make_scorer("cider", c["refs_by_video"], c["wordtoix"]), reward.CiderD)


def test_same_signature_as_ciderd():
    """greedy_eval / beam_eval call scorer.score_ids(ids, rows): duck typing."""
    from s2vt_amd import reward
    assert inspect.signature(reward.RougeL.score_ids) == inspect.signature(reward.CiderD.score_ids)
    c, sc = _scorer("tiny")
    rows = [int(v) for v in c["video_of_row"]]                      # a list of rows, as greedy_eval passes it
    assert np.array_equal(sc.score_ids(c["ids"], rows), RC.expected("tiny")["f32"])


def test_device_entry_checks_its_arguments_without_a_gpu():
    import s2vt_amd
    from s2vt_amd import _lib
    L = s2vt_amd.lib()
    buf = (ctypes.c_int32 * 64)()
    here = ctypes.cast(buf, ctypes.c_void_p)

    def refs(tokens=here, offs=here, vrefs=here, n_videos=1, n_refs=1):
        return ctypes.byref(_lib.RougeRefs(tokens, offs, vrefs, n_videos, n_refs))

    def call(r=None, ids=here, ld=8, N=4, Tc=8, vrow=here, beta2=1.44, out=here, pr=None):
        return L.s2vt_rouge_l_score(refs() if r is None else r, ids, ld, N, Tc, 0, vrow, beta2, out, pr, None)
    bad = _lib.lib().s2vt_error_string(-1)
    assert bad == b"bad argument"
    assert L.s2vt_rouge_l_score(None, here, 8, 4, 8, 0, here, 1.44, here, None, None) == -1
    assert call(r=refs(tokens=None)) == -1 and call(r=refs(offs=None)) == -1 and call(r=refs(vrefs=None)) == -1
    assert call(ids=None) == -1 and call(vrow=None) == -1 and call(out=None) == -1
    assert call(ld=7) == -1                                          # ld < Tc
    assert call(Tc=0, ld=8) == -1 and call(Tc=129, ld=200) == -1
    assert call(N=-1) == -1 and call(r=refs(n_videos=0)) == -1
    assert call(beta2=-0.5) == -1 and call(beta2=float("nan")) == -1 and call(beta2=float("inf")) == -1
    assert call(N=0) == 0 and call(N=0, Tc=128, ld=128) == 0         # nothing is launched


def _dump(c, d):
    from s2vt_amd import reward
    toks, offs, vids = reward.tokenize_refs(c["refs_by_video"], c["wordtoix"])
    toks.astype("<i4").tofile(os.path.join(d, "tokens.i32")); offs.astype("<i8").tofile(os.path.join(d, "offsets.i64"))
    vids.astype("<i4").tofile(os.path.join(d, "video_of_ref.i32"))
    c["ids"].astype("<i4").tofile(os.path.join(d, "ids.i32")); c["video_of_row"].astype("<i4").tofile(os.path.join(d, "video_of_row.i32"))
    return len(vids), len(c["refs_by_video"])


def test_host_file_under_sanitizers_as_a_program(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "rouge_san")
    src = [os.path.join(ROOT, "multitask-end-to-end-video-captioning_amd", "csrc_host", "rouge.cpp"), os.path.join(ROOT, "tests", "rouge_san_main.cpp")]
    b = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", *src, "-o", exe], capture_output=True, text=True)
    # (the runtimes are linked INTO the program: the sanitizers' link-order check has nothing to object to, whatever the environment preloads)
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("the compiler cannot link the sanitizer runtimes")
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for name in RC.CASES:
        c = RC.case(name)
        d = tmp_path / name
        d.mkdir()
        n_refs, n_videos = _dump(c, str(d))
        N, Tc = c["ids"].shape
        r = subprocess.run([exe, str(d), str(n_refs), str(n_videos), str(N), str(Tc), "0", float(RC.BETA ** 2).hex(), "1"], capture_output=True, text=True,
                           env=env, timeout=120)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (name, r.stderr[-2000:])
        got = np.asarray([int(x, 16) for x in r.stdout.split()], np.uint32)
        assert np.array_equal(got, RC.expected(name)["f32"].view(np.uint32)), name
