"""The caller-owned workspace of every driver (`void* workspace, size_t bytes`, or a scratch sized by a *_scratch_bytes function) under the
four checks of tests/workspace_contract.py: A exact and dirty, B shrink, C containment inside a larger window, D refusal.  The window is a
tests/guardband.py::GuardedWorkspace of exactly the bytes the size function declares; it is never pre-filled: the same entry point, run on
other inputs (another noise seed and video_base, other captions, the video scaled by 3), dirties it before the call under test.

A alone cannot see a store past the declared end that stays inside the last region's rounding up to 256 bytes -- those bytes are part of
the window.  C can: the declared end then lies inside a larger window whose bytes behind it must keep their bits.

How a driver gets its window: the entry points are called through s2vt_amd.ops (or straight through s2vt_amd.lib() where ops has no
wrapper for that symbol) while ops.workspace -- and the torch.empty(n, dtype=uint8) of the wrappers that allocate a workspace themselves --
is answered by the test's Provider, so the byte count a wrapper passes is the window's.  Outputs the wrappers allocate are filled with
sentinel bits first.  Nothing else of ops is touched, and the patch is undone after every stage.

Entries, and the existing test each oracle / bound comes from (ids, logits, states: np.array_equal; gradients: max |g - ref| over the
tensor's largest reference entry):
  1 S2VT sampler   s2vt_sample, s2vt_sample_ex (flags 0, STOP_AT_EOS), s2vt_sample_mix, s2vt_sample + s2vt_teacher_forced_fwd_reuse
                   oracle.sample_captions on sampler_cases.build (test_gpu_decode_loop_edges.py); ids behind the first <eos> zero
                   (test_gpu_stop_at_eos.py); _encode / _mix_decode of test_gpu_sample_mix.py; oracle.teacher_forced (test_gpu_train.py)
                   opt-in forms S2VT_DECLOOP=2 / S2VT_DEC4=1: one child process each, checks A and C (test_gpu_decode_loop_edges.py)
  2 S2VT beam      s2vt_beam_encode + s2vt_beam_step over a whole search, on the model and videos of tests/golden/beam_search.json: the
                   per-video BeamSearchGenerator within 2e-4 (test_gpu_beam_batched.py::test_batched_equals_per_video_configs2)
  3 S2VT training  s2vt_teacher_forced_fwd / _steps / _live, s2vt_bptt_bwd / _phase (1, 2) / _steps / _live / _bf16 / _split,
                   s2vt_bptt_dvideo, s2vt_scheduled_fwd: logits oracle.teacher_forced bit for bit, gradients float64 autograd of
                   oracle/s2vt_torch.py within 2e-4 (test_gpu_train.py::test_gradients_vs_float64_autograd), bf16 1e-2
                   (test_gpu_bf16_grads.py GRAD_TOL), d_video 2e-4 (test_gpu_e2e.py); scheduled_cases.scheduled_unroll (test_gpu_scheduled.py);
                   the residual captioner: residual_cases (test_gpu_residual_train.py); 320 rows: BIG of test_gpu_bchain_split.py, Tc = 3
  4 attention      s2vt_attn_teacher_forced_fwd + s2vt_attn_bptt_bwd, s2vt_attn_decode_greedy, s2vt_attn_sample / _ex,
                   s2vt_attn_teacher_forced_fwd_rows + s2vt_attn_bptt_bwd_rows, s2vt_attn_beam_encode + _step: oracle.attention_forward,
                   float64 autograd of attention_xe_loss within 2e-4 (test_gpu_attention_model.py), the per-video search (test_gpu_attn_beam.py)
  5 bidirectional  s2vt_bidir_teacher_forced_fwd + s2vt_bidir_bptt_bwd, s2vt_bidir_decode_greedy, s2vt_bidir_sample,
                   s2vt_bidir_teacher_forced_fwd_rows + s2vt_bidir_bptt_bwd_rows, s2vt_bidir_beam_encode + _step: bidirection_cases,
                   bidirection_rl_cases, bidirection_beam_cases; gradients 2e-4 (test_gpu_bidirection_train.py GRAD_BOUND)
  6 recurrences    s2vt_lstm_recurrence_fwd, s2vt_lstm_birecurrence_fwd, s2vt_lstm_recurrence_bwd, s2vt_lstm_recurrence_bwd_split: the oracle's
                   steps (test_gpu_chain.py, test_gpu_bidirection_chain.py), float64 within 2e-5 of the step's largest entry
                   (test_gpu_chain.py::test_persistent_backward_recurrence), split within 2 x its CPU emulation (test_gpu_bchain_split.py)

Two things the drivers' own contract decides:
  * A scratch the header documents as unused in one form of a call -- the per-step launches (persistent = 0) of s2vt_lstm_recurrence_fwd
    and s2vt_lstm_birecurrence_fwd, which accept a NULL scratch -- is not refused when it is short.  Check D then requires that the call
    succeeds and that not one byte of the short buffer changes (Family.unused).
  * A size function need not grow with the shape: 16 videos x 4 blocks = 64 rows take the persistent decode loop, whose operands are carved
    from the workspace, and need more bytes than 32 videos.  Checks B and C then run the smaller shape on a new window of its own exact
    size that holds the larger call's stale bytes, repeated to its length (what a grow-only cache hands out from reused memory)."""
import contextlib
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile
from collections import namedtuple

import numpy as np
import pytest

import sampler_cases as sc
import workspace_contract as wc

pytestmark = pytest.mark.gpu

GRAD_BOUND = 2e-4            # test_gpu_train.py::test_gradients_vs_float64_autograd, test_gpu_bidirection_train.py, test_gpu_attention_model.py
BF16_BOUND = 1e-2            # test_gpu_bf16_grads.py GRAD_TOL
DVIDEO_BOUND = 2e-4          # test_gpu_e2e.py
CHAIN_BWD_BOUND = 2e-5       # test_gpu_chain.py::test_persistent_backward_recurrence


def _dev(a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _orc():
    from oracle import s2vt_oracle
    return s2vt_oracle


# ---- the Provider behind ops
class _TorchProxy:
    """torch as ops sees it during a stage: outputs come from the Provider (sentinel bits, remembered), and a flat uint8 allocation
    -- a wrapper allocating its own workspace -- is a window, tagged by the allocating function or class."""

    def __init__(self, env):
        self._env = env

    def __getattr__(self, name):
        import torch
        return getattr(torch, name)

    def empty(self, *size, **kw):
        import torch
        if kw.get("dtype") is torch.uint8 and len(size) == 1 and isinstance(size[0], int):
            f = sys._getframe(1)
            owner = f.f_locals.get("self")
            return self._env.ws(size[0], type(owner).__name__ if owner is not None else f.f_code.co_name)
        return self._env.empty(*size, **kw)

    def empty_like(self, t, **kw):
        return self._env.empty(tuple(t.shape), dtype=kw.get("dtype", t.dtype))


@contextlib.contextmanager
def _through(env):
    from s2vt_amd import ops
    orig_ws, orig_torch = ops.workspace, ops.torch

    def workspace(nbytes, device, tag="default"):
        if nbytes <= 0 or nbytes % 256:                                # not a *_workspace_bytes value (a helper's own scratch)
            return orig_ws(nbytes, device, tag)
        return env.ws(nbytes, tag)
    ops.workspace, ops.torch = workspace, _TorchProxy(env)
    try:
        yield ops
    finally:
        ops.workspace, ops.torch = orig_ws, orig_torch


def _stage(fn):
    @functools.wraps(fn)
    def stage(self, env, shape, inp, state):
        with _through(env) as ops:
            return fn(self, ops, env, shape, inp, state)
    return stage


class _Family:
    stage_names = ("run",)

    @property
    def stages(self):
        return [getattr(self, n) for n in self.stage_names]

    def refused(self, e):
        from s2vt_amd._lib import S2VTLibraryError
        return isinstance(e, S2VTLibraryError) and "(code -3)" in str(e)


def _finish(env):
    from s2vt_amd import ops
    assert ops.chain_timeouts() == 0 and not ops.chain_fault()


def _check_A(fam, shape):
    _finish(wc.exact_and_dirty(fam, shape, "cuda"))


def _check_B(fam, small, large):
    _finish(wc.shrink(fam, small, large, "cuda"))


def _check_C(fam, small, large, same_size_ok=False):
    _finish(wc.containment(fam, small, large, "cuda", same_size_ok))


def _check_D(fam, shape):
    _finish(wc.refusal(fam, shape, "cuda"))


def _rel(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (np.abs(ref).max() + 1e-30))


def _assert_grads(got, ref, bound, what):
    for n in sorted(ref):
        e = _rel(got[n].cpu().numpy(), ref[n])
        print(f"{what} {n}: {e:.2e} of {bound:.0e}")
        assert e <= bound, (what, n, e, bound)


# =================================================================================================== 6. stand-alone recurrences
RecShape = namedtuple("RecShape", "M E H T persistent")


class RecurrenceFwd(_Family):
    refusal_checks_new_outputs = False                                 # the wrapper writes slot 0 of the histories itself

    def unused(self, s):                                               # include/s2vt.h: "scratch: ... (persistent form only)"
        return {"chain"} if s.persistent == 0 else ()

    def inputs(self, s, variant):
        import test_gpu_chain as CH
        return CH._case(s.M, s.E, s.H, s.T, s.T, seed=s.M + s.H + 1000 * variant)

    @_stage
    def run(self, ops, env, s, inp, state):
        W, b, h0, c0, cinit, vid, sid = inp
        state["out"] = ops.lstm_recurrence_fwd(_dev(W), s.E, _dev(b), _dev(h0), _dev(c0), T=s.T, cinit=_dev(cinit), cinit_steps=s.T, keep=0.9,
                                               seed=77, video_id=_dev(vid), sample_id=_dev(sid), drop_code0=512, want_gates=True, want_out=True,
                                               persistent=s.persistent)

    def check(self, s, inp, state):
        """the oracle's own steps, as test_gpu_chain.py::test_persistent_recurrence_equals_per_step_launches takes them"""
        oracle = _orc()
        W, b, h0, c0, cinit, vid, sid = inp
        got = [t.cpu().numpy() for t in state["out"]]
        c, h = c0, h0
        for t in range(s.T):
            mask = oracle.dropout_mask(77, vid, sid, 512 + t, 0.9, s.H)
            z = cinit[t].copy()
            oracle.gemm_chain(np.ascontiguousarray(h), np.ascontiguousarray(W[s.E:]), z)
            oracle.bias_add(z, b)
            rc, rh, rout, rg = oracle.lstm_pointwise(z, c, mask, 0.9, want_gates=True)
            assert np.array_equal(got[0][t + 1], rc) and np.array_equal(got[1][t + 1], rh), t
            assert np.array_equal(got[2][t], rg) and np.array_equal(got[3][t], rout), t
            c, h = rc, rh


class BirecurrenceFwd(_Family):
    refusal_checks_new_outputs = False

    def unused(self, s):                                               # per-step launches of the fused cell kernel: no scratch (csrc/bidir.hip)
        return {"bichain"} if s.persistent == 0 else ()

    def _windows(self, s):
        return (0, 1, False), (s.T - 1, 1, True)

    def inputs(self, s, variant):
        import test_gpu_bidirection_chain as BCH
        rng = np.random.default_rng(1000 * s.M + s.H + s.T + 77 * variant)
        return [BCH._dir_case(rng, s.M, s.E, s.H, s.T, w) for w in self._windows(s)]

    @_stage
    def run(self, ops, env, s, dirs, state):
        desc = [ops.lstm_dir(_dev(W), s.E, _dev(b), _dev(h0), _dev(c0), s.T, cinit=_dev(ci), cinit_t0=w[0], reverse=w[2])
                for (W, b, h0, c0, ci), w in zip(dirs, self._windows(s))]
        state["out"] = ops.lstm_birecurrence_fwd(desc[0], desc[1], persistent=s.persistent)

    def check(self, s, dirs, state):
        import test_gpu_bidirection_chain as BCH
        for which, d, w, g in zip(("fw", "bw"), dirs, self._windows(s), state["out"]):
            for name, rr, gg in zip(("C", "H", "gates"), BCH._oracle_dir(_orc(), d, s.E, s.T, w), g):
                assert np.array_equal(rr, gg.cpu().numpy()), (which, name)


class RecurrenceBwd(_Family):
    """s2vt_lstm_recurrence_bwd (precision fp32) / s2vt_lstm_recurrence_bwd_split: the forward products come from per-step launches of the
    forward recurrence on a workspace of their own, outside the stage."""
    refusal_checks_new_outputs = True

    def __init__(self, precision):
        self.precision = precision

    def inputs(self, s, variant):
        import test_gpu_chain as CH
        from s2vt_amd import ops
        W, b, h0, c0, cinit, vid, sid = CH._case(s.M, s.E, s.H, s.T, s.T, seed=s.M + s.H + 1 + 1000 * variant)
        Cc, _, gates, _ = ops.lstm_recurrence_fwd(_dev(W), s.E, _dev(b), _dev(h0), _dev(c0), T=s.T, cinit=_dev(cinit), cinit_steps=s.T,
                                                  want_gates=True, persistent=0)
        dext = (np.random.default_rng(s.M * 7 + s.H + variant).standard_normal((s.T, s.M, s.H)) * 0.1).astype(np.float32)
        return W, gates, Cc, dext, vid, sid

    @_stage
    def run(self, ops, env, s, inp, state):
        W, gates, Cc, dext, vid, sid = inp
        state["dZ"] = ops.lstm_recurrence_bwd(_dev(W), s.E, gates, Cc, dext=_dev(dext), dext_t0=0, keep=1.0, seed=99, video_id=_dev(vid),
                                              sample_id=_dev(sid), drop_code0=512, persistent=s.persistent, precision=self.precision)

    def check(self, s, inp, state):
        import torch
        import test_gpu_bchain_split as BS
        from s2vt_amd import ops
        W, gates, Cc, dext, vid, sid = inp
        ref, emu = BS._float64_and_emulation(ops, W, s.E, gates, Cc, dext, 0, 1.0, vid, sid)
        got = state["dZ"].cpu()
        assert torch.isfinite(got).all()
        e = BS._worst(got, ref)
        bound = 2 * BS._worst(emu, ref) if self.precision == "split" else CHAIN_BWD_BOUND
        print(f"recurrence bwd {self.precision} {s}: {e:.3e} of {bound:.3e}")
        assert e <= bound, (e, bound)


REC_FWD = [RecShape(16, 8, 132, 2, 0), RecShape(16, 8, 132, 2, 1), RecShape(64, 8, 264, 3, 0), RecShape(64, 8, 264, 3, 1)]


@pytest.mark.parametrize("s", REC_FWD, ids=str)
@pytest.mark.parametrize("fam", [RecurrenceFwd(), BirecurrenceFwd()], ids=["s2vt_lstm_recurrence_fwd", "s2vt_lstm_birecurrence_fwd"])
def test_recurrence_fwd_exact_dirty_and_refusal(gpu, fam, s):
    _check_A(fam, s)
    _check_D(fam, s)


@pytest.mark.parametrize("persistent", [0, 1])
@pytest.mark.parametrize("fam", [RecurrenceFwd(), BirecurrenceFwd()], ids=["s2vt_lstm_recurrence_fwd", "s2vt_lstm_birecurrence_fwd"])
def test_recurrence_fwd_containment_between_H_264_and_132(gpu, fam, persistent):
    """(both scratch sizes are the same at these widths -- the state exchange buffer is sized for the widest H -- so what this adds to A is the
    stale data of the other shape; the backward's scratch below does shrink with H)"""
    _check_C(fam, RecShape(16, 8, 132, 2, persistent), RecShape(64, 8, 264, 3, persistent), same_size_ok=True)


REC_BWD = [("fp32", RecShape(64, 8, 264, 3, 0), RecShape(64, 8, 132, 3, 0)), ("fp32", RecShape(64, 8, 264, 3, 1), RecShape(64, 8, 132, 3, 1)),
           ("split", RecShape(257, 8, 264, 3, 1), RecShape(257, 8, 136, 3, 1))]


@pytest.mark.parametrize("precision,s,smaller", REC_BWD, ids=lambda v: str(v))
def test_recurrence_bwd_all_checks(gpu, precision, s, smaller):
    """s2vt_lstm_recurrence_bwd / s2vt_lstm_recurrence_bwd_split: A and D at the issue's shape, C against the same rows at a smaller H (the
    scratch depends on M and H only: there is no shrink case)."""
    fam = RecurrenceBwd(precision)
    _check_A(fam, s)
    _check_C(fam, smaller, s)
    _check_D(fam, s)


# =================================================================================================== 1. S2VT sampler
Tiny = namedtuple("Tiny", "dims B K with_greedy")                      # H < 132: the per-step path
BY_ID = {sc.case_id(c): c for c in sc.CASES}
SAMPLER_SHAPES = [BY_ID["V8-E1-H132-Tc1-B16-K1-g1"], BY_ID["V52-E5-H136-Tc3-B16-K3-g1"], Tiny((16, 11, 3, 4, 2, 3), 4, 2, True)]


def _shape_id(s):
    return sc.case_id(s) if isinstance(s, sc.Case) else f"dims{'-'.join(map(str, s.dims))}-B{s.B}-K{s.K}"


def _larger(s):
    return s._replace(B=2 * s.B)                                       # 16 -> 32 rows of videos (the tiny shape: 4 -> 8)


@functools.lru_cache(maxsize=None)
def _sampler_case(s):
    """(oracle dims, parameters, video, seed, video_base) of a sampler shape: built once, never written to."""
    oracle = _orc()
    if isinstance(s, sc.Case):
        return sc.build(s, oracle)
    d = oracle.Dims(*s.dims, 0)
    p = oracle.init_params(d, seed=3)
    rng = np.random.default_rng(9)
    for k in ("lstm1_b", "lstm2_b", "encode_image_b"):
        p[k] = rng.uniform(-.1, .1, p[k].shape).astype(np.float32)
    p["embed_word_b"] = rng.uniform(-.5, .5, d.n_words).astype(np.float32)
    p["embed_word_W"] = (p["embed_word_W"] * np.float32(30.0)).astype(np.float32)
    video = (np.abs(rng.standard_normal((s.B, d.n_video_lstm_step, d.dim_image)) * 0.5) * np.linspace(0.2, 10.0, s.B)[:, None, None]).astype(np.float32)
    return d, p, video, 2035, 10


def _sampler_inputs(s, variant):
    d, p, video, seed, base = _sampler_case(s)
    rng = np.random.default_rng(5 + variant)
    cap = rng.integers(2, d.n_words, (s.B, d.n_caption_lstm_step)).astype(np.int32)
    if variant:
        video, seed, base = (video * np.float32(3)).astype(np.float32), seed + 1, base + 7
    return dict(d=d, p=p, video=video, seed=seed, base=base, cap=cap)


def _gpu_model(ops, i, residual=False):
    d = i["d"]
    dims = ops.make_dims(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step, residual=residual)
    dp = {k: _dev(v) for k, v in i["p"].items() if v is not None}
    params = ops.make_params(dp)
    params._keep = dp
    return dims, params


class Sampler(_Family):
    """s2vt_sample / s2vt_sample_ex through the C ABI on (ptr, bytes)"""

    def __init__(self, entry, flags=0):
        self.entry, self.flags = entry, flags

    def inputs(self, s, variant):
        return _sampler_inputs(s, variant)

    @_stage
    def run(self, ops, env, s, i, state):
        import torch
        import s2vt_amd
        L = s2vt_amd.lib()
        dims, params = _gpu_model(ops, i)
        g = int(s.with_greedy)
        ws = env.ws(L.s2vt_sample_workspace_bytes(C.byref(dims), s.B, s.K, g), "sample")
        ids = env.empty(((s.K + g) * s.B, dims.n_caption_lstm_step), dtype=torch.int32)
        video = _dev(i["video"])
        head = (C.byref(dims), C.byref(params), _p(video), s.B, s.K, g, i["seed"], i["base"])
        tail = (_p(ids), _p(ws), ws.numel(), _stream())
        rc = L.s2vt_sample(*head, *tail) if self.entry == "s2vt_sample" else L.s2vt_sample_ex(*head, self.flags, *tail)
        s2vt_amd._lib.check(rc, self.entry)
        state["ids"], state["ws"] = ids, ws

    def check(self, s, i, state):
        import bidirection_rl_cases as RC
        ref_s, ref_g = _orc().sample_captions(i["p"], i["d"], i["video"], s.K, seed=i["seed"], video_base=i["base"], with_greedy=s.with_greedy)
        ref = np.concatenate([r for r in (ref_s, ref_g) if r is not None and len(r)])
        if self.flags & 1:                                             # ids behind the first <eos> are 0 (include/s2vt.h, test_gpu_stop_at_eos.py)
            ref = ref * RC.mask_from_ids(ref).astype(np.int32)
        got = state["ids"].cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got, ref), int((got != ref).sum())


class SamplerThenReuse(Sampler):
    """s2vt_sample, then s2vt_teacher_forced_fwd_reuse of the K * B sampled rows on the training workspace, LSTM1's trajectory taken from the
    sampler's workspace (a residual model's is the enlarged one: the plain regions and one [R, H] block)."""
    stage_names = ("run", "reuse")

    def __init__(self, residual=False):
        super().__init__("s2vt_sample")
        self.residual = residual

    def inputs(self, s, variant):
        i = _sampler_inputs(s, variant)
        N = s.K * s.B
        i["cap_rows"] = np.random.default_rng(17 + variant).integers(0, i["d"].n_words, (N, i["d"].n_caption_lstm_step)).astype(np.int32)
        i["vid"] = np.tile(np.arange(s.B, dtype=np.int32) + i["base"], s.K)
        i["sid"] = np.repeat(np.arange(s.K, dtype=np.int32), s.B)
        return i

    @_stage
    def run(self, ops, env, s, i, state):
        import torch
        import s2vt_amd
        L = s2vt_amd.lib()
        dims, params = _gpu_model(ops, i, self.residual)
        g = int(s.with_greedy)
        ws = env.ws(L.s2vt_sample_workspace_bytes(C.byref(dims), s.B, s.K, g), "sample")
        ids = env.empty(((s.K + g) * s.B, dims.n_caption_lstm_step), dtype=torch.int32)
        state["video"] = _dev(i["video"])
        s2vt_amd._lib.check(L.s2vt_sample(C.byref(dims), C.byref(params), _p(state["video"]), s.B, s.K, g, i["seed"], i["base"], _p(ids), _p(ws),
                                          ws.numel(), _stream()), "s2vt_sample")
        state["ids"], state["ws"] = ids, ws

    @_stage
    def reuse(self, ops, env, s, i, state):
        import s2vt_amd
        L = s2vt_amd.lib()
        dims, params = _gpu_model(ops, i, self.residual)
        N, g = s.K * s.B, int(s.with_greedy)
        tws = env.ws(L.s2vt_train_workspace_bytes(C.byref(dims), s.B, N), "train")
        logits = env.empty((dims.n_caption_lstm_step * N, dims.n_words))
        cap, vid, sid = _dev(i["cap_rows"]), _dev(i["vid"]), _dev(i["sid"])
        sws = state["ws"]
        s2vt_amd._lib.check(L.s2vt_teacher_forced_fwd_reuse(C.byref(dims), C.byref(params), _p(state["video"]), s.B, N, _p(cap), 0.9, 99, _p(vid), _p(sid),
                                                            _p(logits), _p(tws), tws.numel(), _p(sws), sws.numel(), (s.K + g) * s.B, _stream()),
                            "s2vt_teacher_forced_fwd_reuse")
        state["logits"] = logits

    def check(self, s, i, state):
        import residual_cases as RES
        oracle, d = _orc(), i["d"]
        if not self.residual:
            super().check(s, i, state)
        drop = oracle.dropout_masks(99, i["vid"], i["sid"], 0.9, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step)
        rows = np.ascontiguousarray(np.tile(i["video"], (s.K, 1, 1)))
        if self.residual:
            ref = RES.residual_teacher_forced(oracle, i["p"], d, rows, i["cap_rows"], drop, 0.9)
        else:
            ref = oracle.teacher_forced(i["p"], d, rows, i["cap_rows"], drop, 0.9)
        got = state["logits"].view(d.n_caption_lstm_step, s.K * s.B, d.n_words).permute(1, 0, 2).cpu().numpy()
        assert np.array_equal(got, ref)


class SamplerMix(_Family):
    def inputs(self, s, variant):
        return _sampler_inputs(s, variant)

    @_stage
    def run(self, ops, env, s, i, state):
        dims, params = _gpu_model(ops, i)
        state["out"] = ops.sample_mix(dims, params, _dev(i["video"]), _dev(i["cap"]), float(np.float32(0.5 / 1.00001)), i["seed"], i["base"], s.with_greedy)

    def check(self, s, i, state):
        import test_gpu_sample_mix as SM
        oracle = _orc()
        enc = SM._encode(oracle, i["p"], i["d"], i["video"])
        ref_m, ref_g, _, _ = SM._mix_decode(oracle, i["p"], i["d"], enc, i["cap"], np.float32(0.5 / 1.00001), i["seed"], i["base"], s.with_greedy)
        m, g = state["out"]
        assert np.array_equal(m.cpu().numpy(), ref_m)
        assert np.array_equal(g.cpu().numpy(), ref_g)


SAMPLER_FAMILIES = [Sampler("s2vt_sample"), Sampler("s2vt_sample_ex", 0), Sampler("s2vt_sample_ex", 1), SamplerMix(), SamplerThenReuse()]
SAMPLER_IDS = ["s2vt_sample", "s2vt_sample_ex-flags0", "s2vt_sample_ex-stop_at_eos", "s2vt_sample_mix", "s2vt_sample+s2vt_teacher_forced_fwd_reuse"]


@pytest.mark.parametrize("s", SAMPLER_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("fam", SAMPLER_FAMILIES, ids=SAMPLER_IDS)
def test_sampler_all_checks(gpu, fam, s):
    _check_A(fam, s)
    _check_B(fam, s, _larger(s))
    _check_C(fam, s, _larger(s))
    _check_D(fam, s)


def test_residual_sampler_workspace_feeds_the_reuse_forward(gpu):
    """the enlarged sampler workspace of a residual model (the plain regions + one [R, H] block) and the reuse forward reading it"""
    import residual_cases as RES
    fam = SamplerThenReuse(residual=True)
    p, d, video = RES.case(_orc(), "small-odd")
    small = Tiny((d.dim_image, d.n_words, d.word_dim, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step), video.shape[0], 2, True)
    for check in (lambda: _check_A(fam, small), lambda: _check_B(fam, small, _larger(small)), lambda: _check_C(fam, small, _larger(small)),
                  lambda: _check_D(fam, small)):
        check()


# ---- the opt-in forms at 257-384 rows: the switches are read once per process, so one child per switch runs checks A and C
CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["S2VT_ROOT"]); sys.path.insert(0, os.path.join(os.environ["S2VT_ROOT"], "tests"))
import numpy as np, torch
import s2vt_amd
from s2vt_amd import ops
import sampler_cases as sc
import test_gpu_workspace_contract as T
cases = [sc.BIG_CASES[0]] + ([sc.DEC4_ONLY_CASES[0]] if sys.argv[2] == "dec4" else [])
fam = T.Sampler("s2vt_sample")
ops.prof_filter(-1, -1); ops.prof_enable(True)
for c in cases:
    T._check_A(fam, c)                      # the workspace size is asked for here, under the switch
    T._check_C(fam, c, c._replace(K=c.K + 4))
torch.cuda.synchronize()
ops.prof_enable(False)
names = sorted({r["name"] for r in ops.prof_collect()})
np.savez(sys.argv[1], names=np.asarray(names), timeouts=np.asarray(ops.chain_timeouts()))
print("child ok")
'''


def test_optin_big_forms_exact_dirty_and_containment(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env0 = {k: v for k, v in os.environ.items() if k not in ("S2VT_DECLOOP", "S2VT_DEC4")}
    with tempfile.TemporaryDirectory() as td:
        for mode, knob, want in (("loop", {"S2VT_DECLOOP": "2"}, "decloop(m320)"), ("dec4", {"S2VT_DEC4": "1"}, "dec4(m320)")):
            f = os.path.join(td, f"{mode}.npz")
            # a child that faults or runs out of time ends the test here (TimeoutExpired / the assertion): the next one is not started
            r = subprocess.run([sys.executable, "-c", CHILD, f, mode], env=dict(env0, S2VT_ROOT=root, **knob), capture_output=True, text=True,
                               timeout=180)
            assert r.returncode == 0 and "child ok" in r.stdout, (mode, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
            res = dict(np.load(f))
            assert int(res["timeouts"]) == 0
            assert want in set(res["names"].tolist()), (mode, res["names"])


# =================================================================================================== 3. S2VT training
TrainShape = namedtuple("TrainShape", "kind B rep dims")              # kind: plain | residual; dims = (D, V, E, H, Tv, Tc)
DIM_NAMES = ("dim_image", "n_words", "word_dim", "lstm_dim", "n_video_lstm_step", "n_caption_lstm_step")


def _train_shapes():
    import residual_cases as RES
    import test_gpu_bchain_split as BS
    import test_gpu_train as TR
    c = TR.CASES[0]
    small = TrainShape("plain", c["B"], c["rep"], tuple(c["dims"][n] for n in DIM_NAMES))
    big = dict(BS.BIG, n_caption_lstm_step=3)
    rows320 = TrainShape("plain", 64, 5, tuple(big[n] for n in DIM_NAMES))                       # N = 320: above 256 rows
    rdims, rB = RES.SHAPES["small-odd"]
    residual = TrainShape("residual", rB, 2, tuple(rdims[n] for n in DIM_NAMES))
    return small, rows320, residual


def _train_larger(s):
    return s._replace(B=2 * s.B, rep=s.rep + 1) if s.B < 64 else s._replace(B=s.B + 16, rep=s.rep)   # 320 -> 400 rows


@functools.lru_cache(maxsize=None)
def _train_params(s):
    import residual_cases as RES
    import test_gpu_train as TR
    oracle = _orc()
    if s.kind == "residual":
        p, d, _ = RES.case(oracle, "small-odd")
        return d, p
    d, p, *_ = TR._setup(oracle, dict(B=s.B, rep=s.rep, dims=dict(zip(DIM_NAMES, s.dims))))
    return d, p


def _train_inputs(s, variant):
    d, p = _train_params(s._replace(B=3, rep=2) if s.kind == "plain" and s.B < 64 else s._replace(B=64, rep=5) if s.kind == "plain" else s)
    rng = np.random.default_rng(31 + variant + 7 * s.B)
    N, Tc = s.B * s.rep, d.n_caption_lstm_step
    video = (np.abs(rng.standard_normal((s.B, d.n_video_lstm_step, d.dim_image)) * 0.5) * (3 if variant else 1)).astype(np.float32)
    cap = rng.integers(0, d.n_words, (N, Tc)).astype(np.int32)
    lens = rng.integers(1, Tc, N) if Tc > 1 else np.ones(N, np.int64)
    lens[0] = max(Tc - 1, 1)
    mask = (np.arange(Tc)[None, :] < lens[:, None]).astype(np.float32)
    steps = int(lens.max())
    coef_tm = np.ascontiguousarray((mask * rng.standard_normal((N, Tc))).astype(np.float32).T).reshape(-1)
    live = np.flatnonzero(mask[:, :steps].T.reshape(-1)).astype(np.int32)
    vid = np.tile(np.arange(s.B, dtype=np.int32) + 5 + variant, s.rep)
    sid = np.repeat(np.arange(s.rep, dtype=np.int32), s.B)
    return dict(d=d, p=p, video=video, cap=cap, vid=vid, sid=sid, N=N, keep=0.9, seed=99 + variant, steps=steps, mask=mask, coef_tm=coef_tm, live=live)


@functools.lru_cache(maxsize=None)
def _train_reference(s):
    """(logits [N, Tc, V] of the oracle, float64 gradients of sum coef * nll incl. d_video) for the inputs under test: computed once."""
    import torch
    import residual_cases as RES
    from oracle import s2vt_torch as T
    oracle, i = _orc(), _train_inputs(s, 0)
    d, N = i["d"], i["N"]
    drop = oracle.dropout_masks(i["seed"], i["vid"], i["sid"], i["keep"], d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step)
    rows = np.ascontiguousarray(np.tile(i["video"], (s.rep, 1, 1)))
    if s.kind == "residual":
        logits = RES.residual_teacher_forced(oracle, i["p"], d, rows, i["cap"], drop, i["keep"])
    else:
        logits = oracle.teacher_forced(i["p"], d, rows, i["cap"], drop, i["keep"])
    pt = T.to_torch({k: v for k, v in i["p"].items() if v is not None}, torch.float64, True)
    vt = torch.tensor(i["video"], dtype=torch.float64, requires_grad=True)
    lg = RES.torch_teacher_forced(pt, vt.repeat(s.rep, 1, 1), i["cap"], drop, i["keep"], residual=s.kind == "residual")
    lp = torch.log_softmax(lg, -1).gather(2, torch.as_tensor(i["cap"]).long().unsqueeze(-1)).squeeze(-1)
    coef = torch.as_tensor(i["coef_tm"].reshape(d.n_caption_lstm_step, N).T.copy()).double()
    (-(lp * coef).sum()).backward()
    g = {k: v.grad.numpy() for k, v in pt.items() if v.grad is not None}
    g["d_video"] = vt.grad.numpy()
    return logits, g


class Train(_Family):
    """fwd: s2vt_teacher_forced_fwd | _steps | _live;  bwd: s2vt_bptt_bwd | _phase (1 then 2) | _steps | _live | _bf16 | _split;
    then s2vt_bptt_dvideo.  All through the C ABI on (ptr, bytes); the objective is sum coef * nll with coef zero behind a row's length."""
    stage_names = ("fwd", "bwd", "dvideo")

    def __init__(self, fwd, bwd):
        self.f, self.b = fwd, bwd

    def inputs(self, s, variant):
        return _train_inputs(s, variant)

    def _setup(self, ops, s, i, state):
        if "dims" not in state:
            state["dims"], state["params"] = _gpu_model(ops, i, s.kind == "residual")
            for k in ("video", "cap", "vid", "sid", "live", "coef_tm"):
                state[k] = _dev(i[k])
        return state["dims"], state["params"]

    def _rows(self, i):
        Tc = i["d"].n_caption_lstm_step
        return {"plain": Tc * i["N"], "steps": i["steps"] * i["N"], "live": len(i["live"])}[self.f]

    @_stage
    def fwd(self, ops, env, s, i, state):
        import s2vt_amd
        L = s2vt_amd.lib()
        dims, params = self._setup(ops, s, i, state)
        N = i["N"]
        tws = env.ws(L.s2vt_train_workspace_bytes(C.byref(dims), s.B, N), "train")
        logits = env.empty((self._rows(i), dims.n_words))
        head = (C.byref(dims), C.byref(params), _p(state["video"]), s.B, N, _p(state["cap"]))
        noise = (i["keep"], i["seed"], _p(state["vid"]), _p(state["sid"]), _p(logits), _p(tws), tws.numel())
        if self.f == "plain":
            rc = L.s2vt_teacher_forced_fwd(*head, *noise, _stream())
        elif self.f == "steps":
            rc = L.s2vt_teacher_forced_fwd_steps(*head, i["steps"], *noise, None, 0, 0, _stream())
        else:
            rc = L.s2vt_teacher_forced_fwd_live(*head, i["steps"], _p(state["live"]), len(i["live"]), *noise, None, 0, 0, _stream())
        s2vt_amd._lib.check(rc, "s2vt_teacher_forced_fwd_" + self.f)
        state["logits"] = logits

    @_stage
    def bwd(self, ops, env, s, i, state):
        import torch
        import s2vt_amd
        L = s2vt_amd.lib()
        dims, params = self._setup(ops, s, i, state)
        N, rows = i["N"], self._rows(i)
        sel = state["live"].long() if self.f == "live" else slice(0, rows)
        dl = state["logits"].clone()                                   # (softmax in place on a copy: the forward's output stays as it is)
        target = state["cap"].t().contiguous().view(-1)[sel].contiguous()
        nll = torch.empty(rows, device="cuda"); lp = torch.empty(rows, device="cuda")
        s2vt_amd._lib.check(L.s2vt_softmax_nll_fwd_bwd(_p(dl), dl.stride(0), rows, dims.n_words, _p(target), _p(state["coef_tm"][sel].contiguous()), 0.0,
                                                       _p(nll), _p(lp), _stream()), "s2vt_softmax_nll_fwd_bwd")
        g = {k: torch.zeros_like(v) for k, v in params._keep.items()}
        grads = ops.make_params(g)
        tws = env.ws(L.s2vt_train_workspace_bytes(C.byref(dims), s.B, N), "train")
        head = (C.byref(dims), C.byref(params), C.byref(grads), _p(state["video"]), s.B, N, _p(dl))
        noise = (i["keep"], i["seed"], _p(state["vid"]), _p(state["sid"]), _p(tws), tws.numel())
        lv = (i["steps"], _p(state["live"]) if self.f == "live" else None, len(i["live"]) if self.f == "live" else 0)
        assert self.f != "plain" or i["steps"] <= dims.n_caption_lstm_step
        if self.b == "plain":
            rcs = [L.s2vt_bptt_bwd(*head, *noise, _stream())]
        elif self.b == "phase":
            rcs = [L.s2vt_bptt_bwd_phase(*head, *noise, ph, _stream()) for ph in (1, 2)]
        elif self.b == "steps":
            rcs = [L.s2vt_bptt_bwd_steps(*head, i["steps"], *noise, 0, _stream())]
        elif self.b == "live":
            rcs = [L.s2vt_bptt_bwd_live(*head, *lv, *noise, 0, _stream())]
        else:
            size, fn, tag = {"bf16": (L.s2vt_bf16_grad_workspace_bytes, L.s2vt_bptt_bwd_bf16, "bf16_grad"),
                             "split": (L.s2vt_split_grad_workspace_bytes, L.s2vt_bptt_bwd_split, "split_grad")}[self.b]
            scratch = env.ws(size(C.byref(dims), s.B, N), tag)
            steps = i["steps"] if self.f != "plain" else dims.n_caption_lstm_step
            rcs = [fn(*head, steps, lv[1], lv[2], *noise, 0, _p(scratch), scratch.numel(), _stream())]
        for rc in rcs:
            s2vt_amd._lib.check(rc, "s2vt_bptt_bwd_" + self.b)
        state["grads"] = g

    @_stage
    def dvideo(self, ops, env, s, i, state):
        import s2vt_amd
        L = s2vt_amd.lib()
        dims, params = self._setup(ops, s, i, state)
        tws = env.ws(L.s2vt_train_workspace_bytes(C.byref(dims), s.B, i["N"]), "train")
        dv = env.empty((s.B, dims.n_video_lstm_step, dims.dim_image))
        s2vt_amd._lib.check(L.s2vt_bptt_dvideo(C.byref(dims), C.byref(params), s.B, i["N"], _p(dv), _p(tws), tws.numel(), _stream()), "s2vt_bptt_dvideo")
        state["grads"]["d_video"] = dv

    def check(self, s, i, state):
        d, N = i["d"], i["N"]
        ref_logits, ref_g = _train_reference(s)
        tm = np.ascontiguousarray(ref_logits.transpose(1, 0, 2)).reshape(-1, d.n_words)        # time-major [Tc * N, V]
        want = tm[i["live"]] if self.f == "live" else tm[:self._rows(i)]
        assert np.array_equal(state["logits"].cpu().numpy(), want)
        dv = state["grads"].pop("d_video")
        _assert_grads(state["grads"], {k: v for k, v in ref_g.items() if k != "d_video"}, BF16_BOUND if self.b == "bf16" else GRAD_BOUND,
                      f"{self.f}+{self.b}")
        e = _rel(dv.cpu().numpy(), ref_g["d_video"])
        print(f"d_video: {e:.2e}")
        assert e <= (BF16_BOUND if self.b == "bf16" else DVIDEO_BOUND), e


TRAIN_MODES = [("plain", "plain"), ("plain", "phase"), ("steps", "steps"), ("live", "live"), ("live", "bf16"), ("live", "split"), ("plain", "split")]
TRAIN_IDS = ["s2vt_teacher_forced_fwd+s2vt_bptt_bwd+s2vt_bptt_dvideo", "s2vt_teacher_forced_fwd+s2vt_bptt_bwd_phase",
             "s2vt_teacher_forced_fwd_steps+s2vt_bptt_bwd_steps", "s2vt_teacher_forced_fwd_live+s2vt_bptt_bwd_live",
             "s2vt_teacher_forced_fwd_live+s2vt_bptt_bwd_bf16", "s2vt_teacher_forced_fwd_live+s2vt_bptt_bwd_split", "dense+s2vt_bptt_bwd_split"]


@pytest.mark.parametrize("mode", TRAIN_MODES, ids=TRAIN_IDS)
def test_training_all_checks_at_the_smallest_shape(gpu, mode):
    fam, (small, _, _) = Train(*mode), _train_shapes()
    _check_A(fam, small)
    _check_B(fam, small, _train_larger(small))
    _check_C(fam, small, _train_larger(small))
    _check_D(fam, small)


@pytest.mark.parametrize("mode", [("live", "live"), ("live", "split"), ("live", "bf16")], ids=["s2vt_bptt_bwd_live", "s2vt_bptt_bwd_split", "s2vt_bptt_bwd_bf16"])
def test_training_above_256_rows(gpu, mode):
    """N = 320: LSTM2's recurrences take the register-weights and split forms"""
    fam, (_, rows320, _) = Train(*mode), _train_shapes()
    _check_A(fam, rows320)
    _check_B(fam, rows320, _train_larger(rows320))
    _check_C(fam, rows320, _train_larger(rows320))
    _check_D(fam, rows320)


@pytest.mark.parametrize("mode", [("plain", "plain"), ("live", "split")], ids=["s2vt_bptt_bwd", "s2vt_bptt_bwd_split"])
def test_training_residual_captioner(gpu, mode):
    fam, (_, _, residual) = Train(*mode), _train_shapes()
    _check_A(fam, residual)
    _check_B(fam, residual, _train_larger(residual))
    _check_C(fam, residual, _train_larger(residual))
    _check_D(fam, residual)


SchedShape = namedtuple("SchedShape", "name B")


class Scheduled(_Family):
    """s2vt_scheduled_fwd on the training workspace and its own scratch (s2vt_scheduled_scratch_bytes), both guarded"""

    def inputs(self, s, variant):
        import scheduled_cases as SCH
        p, d, *_ = SCH.case(_orc(), s.name)
        rng = np.random.default_rng(3 + variant + s.B)
        video = (np.abs(rng.standard_normal((s.B, d.n_video_lstm_step, d.dim_image)) * 0.5) * (3 if variant else 1)).astype(np.float32)
        gt = rng.integers(2, d.n_words, (s.B, d.n_caption_lstm_step)).astype(np.int32)
        return dict(d=d, p=p, video=video, gt=gt, vid=np.arange(s.B, dtype=np.int32) + 3 * variant, sid=np.zeros(s.B, np.int32), coin=11 + variant)

    @_stage
    def run(self, ops, env, s, i, state):
        import scheduled_cases as SCH
        dims, params = _gpu_model(ops, i)
        state["out"] = ops.scheduled_fwd(dims, params, _dev(i["video"]), _dev(i["gt"]), s.B, float(SCH.p_gt_of(0.5)), i["coin"], 1.0, 0.9, SCH.DROP_SEED,
                                         _dev(i["vid"]), _dev(i["sid"]))

    def check(self, s, i, state):
        import scheduled_cases as SCH
        r = SCH.scheduled_unroll(_orc(), i["p"], i["d"], i["video"], i["gt"], SCH.p_gt_of(0.5), i["coin"], i["vid"], i["sid"], keep=0.9)
        f = state["out"]
        for k in ("generated", "fed", "mask", "coef_tm", "target_tm", "logits"):      # test_gpu_scheduled.py::test_forward_equals_the_restatement
            assert np.array_equal(f[k].cpu().numpy(), r[k]), k
        assert float(f["mask_sum"]) == r["mask_sum"]


def test_scheduled_fwd_all_checks(gpu):
    fam, small, large = Scheduled(), SchedShape("small-odd", 5), SchedShape("small-odd", 12)
    _check_A(fam, small)
    _check_B(fam, small, large)
    _check_C(fam, small, large)
    _check_D(fam, small)


# ---- shared by the attention and bidirectional training pairs: the objective sum coef * nll and its float64 gradients
def _lengths_and_coef(rng, N, Tc):
    lens = rng.integers(1, Tc + 1, N)
    lens[0], lens[-1] = Tc, 1
    mask = (np.arange(Tc)[None, :] < lens[:, None]).astype(np.float32)
    coef = (mask * rng.uniform(0.5, 1.5, (N, Tc)) / mask.sum()).astype(np.float32)
    return np.ascontiguousarray(coef.T).reshape(-1)                      # time-major [Tc * N]


def _float64_grads(p, logits_fn, cap, coef_tm):
    """d(sum coef * nll)/d(every variable) by float64 autograd; logits_fn(pt) -> logits [N, Tc, V]"""
    import torch
    from oracle import s2vt_torch as T
    pt = T.to_torch(p, torch.float64, True)
    lg = logits_fn(pt)
    N, Tc = cap.shape
    lp = torch.log_softmax(lg, -1).gather(2, torch.as_tensor(cap).long().unsqueeze(-1)).squeeze(-1)
    (-(lp * torch.as_tensor(coef_tm.reshape(Tc, N).T.copy()).double()).sum()).backward()
    return {k: v.grad.numpy() for k, v in pt.items()}


def _dlogits(state, logits, cap_dev, coef_tm):
    """coef * (softmax - onehot) of a copy of the forward's logits (s2vt_softmax_nll_fwd_bwd, no workspace)"""
    import torch
    import s2vt_amd
    dl = logits.clone()
    R, V = dl.shape
    target = cap_dev.t().contiguous().view(-1)
    nll = torch.empty(R, device="cuda"); lp = torch.empty(R, device="cuda")
    coef = _dev(coef_tm)
    s2vt_amd._lib.check(s2vt_amd.lib().s2vt_softmax_nll_fwd_bwd(_p(dl), dl.stride(0), R, V, _p(target), _p(coef), 0.0, _p(nll), _p(lp), _stream()),
                        "s2vt_softmax_nll_fwd_bwd")
    state["_keep_dl"] = (dl, target, coef, nll, lp)
    return dl


# =================================================================================================== 4. attention captioner
AttnShape = namedtuple("AttnShape", "D V H Tv Tc B K")
ATTN_SMALL = AttnShape(48, 131, 32, 5, 6, 5, 3)                          # test_gpu_attention_model.py / test_gpu_attn_reinforce.py SHAPES[0]; B <= 64: persistent
ATTN_LARGE = ATTN_SMALL._replace(B=10, K=4)
ATTN_STEPWISE = ATTN_SMALL._replace(B=66, K=1)                           # above 64 rows: per-step launches


@functools.lru_cache(maxsize=None)
def _attn_params(D, V, H, Tv, Tc):
    import test_gpu_attn_reinforce as AR
    d, p, _ = AR._params((D, V, H, Tv, Tc, 1, 1))                          # embed_word_b[0] = 3: sampled rows end early
    rng = np.random.default_rng(2)
    for k in ("lstm3_b", "embed_att_ba", "embed_nn_bp", "encode_image_b"):
        p[k] = rng.uniform(-.1, .1, p[k].shape).astype(np.float32)
    return d, p


def _attn_inputs(s, variant, rows=False):
    d, p = _attn_params(s.D, s.V, s.H, s.Tv, s.Tc)
    rng = np.random.default_rng(40 + variant + s.B)
    video = (np.abs(rng.standard_normal((s.B, s.Tv, s.D)) * 0.5) * (3 if variant else 1)).astype(np.float32)
    S = s.K if rows else 1
    N = S * s.B
    cap = rng.integers(0, s.V, (N, s.Tc)).astype(np.int32)
    base = 10 + 7 * variant
    vid = np.tile(np.arange(s.B, dtype=np.int32) + base, S)
    sid = np.repeat(np.arange(S, dtype=np.int32), s.B)
    return dict(d=d, p=p, video=video, cap=cap, vid=vid, sid=sid, N=N, S=S, base=base, keep=0.9, seed=321 + variant, sample_seed=11 + variant,
                coef_tm=_lengths_and_coef(rng, N, s.Tc))


def _attn_model(ops, s, i, state):
    if "dims" not in state:
        import torch
        state["dims"] = ops.make_dims(s.D, s.V, s.H, s.H, s.Tv, s.Tc)
        state["dp"] = {k: _dev(v) for k, v in i["p"].items()}
        state["params"] = ops.make_attn_params(state["dp"])
        for k in ("video", "cap", "vid", "sid"):
            state[k] = _dev(i[k])
    return state["dims"], state["params"]


def _attn_drop(i, s):
    return [_orc().dropout_mask(i["seed"], i["vid"], i["sid"], 768 + t, i["keep"], s.H) for t in range(s.Tc)]


class AttnTrain(_Family):
    """s2vt_attn_teacher_forced_fwd + s2vt_attn_bptt_bwd, or the _rows pair on N = K * B rows that share the B image blocks"""
    stage_names = ("fwd", "bwd")

    def __init__(self, rows):
        self.rows = rows

    def inputs(self, s, variant):
        return _attn_inputs(s, variant, self.rows)

    def _ws(self, ops, s, i, dims):
        return ops.attn_rows_workspace(dims, s.B, i["S"], "cuda") if self.rows else ops.attn_workspace(dims, s.B, "cuda")

    @_stage
    def fwd(self, ops, env, s, i, state):
        dims, params = _attn_model(ops, s, i, state)
        f = ops.attn_teacher_forced_fwd_rows if self.rows else ops.attn_teacher_forced_fwd
        state["logits"], state["alphas"], _ = f(dims, params, state["video"], state["cap"], i["keep"], i["seed"], state["vid"], state["sid"],
                                                ws=self._ws(ops, s, i, dims), want_alphas=True)

    @_stage
    def bwd(self, ops, env, s, i, state):
        import torch
        dims, params = _attn_model(ops, s, i, state)
        dl = _dlogits(state, state["logits"], state["cap"], i["coef_tm"])
        g = {k: torch.zeros_like(v) for k, v in state["dp"].items()}
        kw = dict(keep=i["keep"], seed=i["seed"], video_id=state["vid"], sample_id=state["sid"])
        if self.rows:
            ops.attn_bptt_bwd_rows(dims, params, ops.make_attn_params(g), state["video"], i["S"], dl, self._ws(ops, s, i, dims), **kw)
        else:
            ops.attn_bptt_bwd(dims, params, ops.make_attn_params(g), state["video"], dl, self._ws(ops, s, i, dims), **kw)
        state["grads"] = g

    def check(self, s, i, state):
        import torch
        from oracle import s2vt_torch as T
        drop = _attn_drop(i, s)
        tiled = np.ascontiguousarray(np.tile(i["video"], (i["S"], 1, 1)))
        ref_l, ref_a, _ = _orc().attention_forward(i["p"], i["d"], tiled, i["cap"], drop, i["keep"])
        assert np.array_equal(state["alphas"].cpu().numpy(), ref_a)
        assert np.array_equal(state["logits"].view(s.Tc, i["N"], s.V).transpose(0, 1).cpu().numpy(), ref_l)
        ref = _float64_grads(i["p"], lambda pt: T.attention_teacher_forced(pt, torch.as_tensor(tiled).double(), i["cap"], drop, i["keep"])[0], i["cap"],
                             i["coef_tm"])
        _assert_grads({k: v.reshape(ref[k].shape) for k, v in state["grads"].items()}, ref, GRAD_BOUND, "attn rows" if self.rows else "attn")


class AttnGreedy(_Family):
    def inputs(self, s, variant):
        return _attn_inputs(s, variant)

    @_stage
    def run(self, ops, env, s, i, state):
        dims, params = _attn_model(ops, s, i, state)
        state["ids"], state["alphas"] = ops.attn_decode_greedy(dims, params, state["video"], i["base"], want_alphas=True)

    def check(self, s, i, state):
        _, ref_a, ref_ids = _orc().attention_forward(i["p"], i["d"], i["video"], None, greedy=True)
        assert np.array_equal(state["ids"].cpu().numpy(), ref_ids) and np.array_equal(state["alphas"].cpu().numpy(), ref_a)


class AttnSample(_Family):
    def __init__(self, stop_at_eos):
        self.stop = stop_at_eos

    def inputs(self, s, variant):
        return _attn_inputs(s, variant)

    @_stage
    def run(self, ops, env, s, i, state):
        dims, params = _attn_model(ops, s, i, state)
        state["out"] = ops.attn_sample(dims, params, state["video"], s.K, i["sample_seed"], i["base"], True, stop_at_eos=self.stop)

    def check(self, s, i, state):
        """test_gpu_attn_reinforce.py::test_sampler_ids_bit_exact_vs_oracle: by induction over t, the ids up to t - 1 are the oracle's, so the
        oracle's logits of step t are what the device picked from.  Early exit: equal up to and including the first <eos>, zeros behind it."""
        import bidirection_rl_cases as RC
        oracle = _orc()
        rows = np.concatenate([t.cpu().numpy() for t in state["out"]])
        mask = RC.mask_from_ids(rows) > 0
        if self.stop:
            assert (rows[~mask] == 0).all()
        logits, _, _ = oracle.attention_forward(i["p"], i["d"], np.ascontiguousarray(np.tile(i["video"], (s.K + 1, 1, 1))), rows, None, 1.0)
        vid = np.tile(np.arange(s.B, dtype=np.int32) + i["base"], s.K + 1)
        sid = np.concatenate([np.repeat(np.arange(s.K, dtype=np.int32), s.B), np.full(s.B, -1, np.int32)])
        assert mask.sum() < mask.size                                  # some row ends early: the early exit has something to skip
        for t in range(s.Tc):
            want = oracle.pick_tokens(np.ascontiguousarray(logits[:, t]), vid, sid, t, i["sample_seed"])
            live = mask[:, t] if self.stop else slice(None)
            assert np.array_equal(want[live], rows[:, t][live]), t


ATTN_FAMILIES = [AttnTrain(False), AttnTrain(True), AttnGreedy(), AttnSample(False), AttnSample(True)]
ATTN_IDS = ["s2vt_attn_teacher_forced_fwd+s2vt_attn_bptt_bwd", "s2vt_attn_teacher_forced_fwd_rows+s2vt_attn_bptt_bwd_rows", "s2vt_attn_decode_greedy",
            "s2vt_attn_sample", "s2vt_attn_sample_ex"]


@pytest.mark.parametrize("fam", ATTN_FAMILIES, ids=ATTN_IDS)
def test_attention_all_checks(gpu, fam):
    _check_A(fam, ATTN_SMALL)
    _check_B(fam, ATTN_SMALL, ATTN_LARGE)
    _check_C(fam, ATTN_SMALL, ATTN_LARGE)
    _check_D(fam, ATTN_SMALL)


@pytest.mark.parametrize("fam", ATTN_FAMILIES, ids=ATTN_IDS)
def test_attention_stepwise_path_exact_and_dirty(gpu, fam):
    _check_A(fam, ATTN_STEPWISE)


# =================================================================================================== 5. bidirectional captioner
BidirShape = namedtuple("BidirShape", "name B S")
BIDIR_SMALL, BIDIR_LARGE = BidirShape("small-odd", 5, 3), BidirShape("small-odd", 10, 4)


def _bidir_inputs(s, variant, rows=False, eos_bias=False):
    import bidirection_cases as BC
    import bidirection_rl_cases as RC
    oracle = _orc()
    p, d = (RC.case(oracle, s.name)[:2] if eos_bias else BC.case(oracle, s.name)[:2])
    rng = np.random.default_rng(50 + variant + s.B)
    video = (np.abs(rng.standard_normal((s.B, d.n_video_lstm_step, d.dim_image)) * 0.5) * (3 if variant else 1)).astype(np.float32)
    S = s.S if rows else 1
    N = S * s.B
    cap = rng.integers(2, d.n_words, (N, d.n_caption_lstm_step)).astype(np.int32)
    base = 7 * variant
    vid = np.tile(np.arange(s.B, dtype=np.int32) + base, S)
    sid = np.repeat(np.arange(S, dtype=np.int32), s.B)
    return dict(d=d, p=p, video=video, cap=cap, vid=vid, sid=sid, N=N, S=S, base=base, keep=0.9, seed=BC.DROP_SEED + variant, sample_seed=RC.SAMPLE_SEED + variant,
                coef_tm=_lengths_and_coef(rng, N, d.n_caption_lstm_step))


def _bidir_model(ops, i, state):
    if "dims" not in state:
        d = i["d"]
        state["dims"] = ops.make_dims(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step)
        state["dp"] = {k: _dev(v) for k, v in i["p"].items()}
        state["params"] = ops.make_bidir_params(state["dp"])
        for k in ("video", "cap", "vid", "sid"):
            state[k] = _dev(i[k])
    return state["dims"], state["params"]


class BidirTrain(_Family):
    """s2vt_bidir_teacher_forced_fwd + s2vt_bidir_bptt_bwd, or the _rows pair"""
    stage_names = ("fwd", "bwd")

    def __init__(self, rows):
        self.rows = rows

    def inputs(self, s, variant):
        return _bidir_inputs(s, variant, self.rows)

    def _ws(self, ops, s, i, dims):
        return ops.bidir_rows_workspace(dims, s.B, i["S"], "cuda") if self.rows else ops.bidir_workspace(dims, s.B, "cuda")

    @_stage
    def fwd(self, ops, env, s, i, state):
        dims, params = _bidir_model(ops, i, state)
        f = ops.bidir_teacher_forced_fwd_rows if self.rows else ops.bidir_teacher_forced_fwd
        state["logits"] = f(dims, params, state["video"], state["cap"], self._ws(ops, s, i, dims), i["keep"], i["seed"], state["vid"], state["sid"])

    @_stage
    def bwd(self, ops, env, s, i, state):
        import torch
        dims, params = _bidir_model(ops, i, state)
        dl = _dlogits(state, state["logits"], state["cap"], i["coef_tm"])
        g = {k: torch.zeros_like(v) for k, v in state["dp"].items()}
        args = (dl, self._ws(ops, s, i, dims), i["keep"], i["seed"], state["vid"], state["sid"])
        if self.rows:
            ops.bidir_bptt_bwd_rows(dims, params, ops.make_bidir_params(g), state["video"], i["S"], *args)
        else:
            ops.bidir_bptt_bwd(dims, params, ops.make_bidir_params(g), state["video"], *args)
        state["grads"] = g

    def _torch_logits(self, pt, d, video, cap, drop, keep):
        """the unroll of bidirection_cases.torch_loss / bidirection_rl_cases.torch_objective, up to the logits [N, Tc, V]"""
        import torch
        from oracle import s2vt_torch as T
        dt = pt["Wemb"].dtype
        video = torch.as_tensor(video).to(dt)
        caption = torch.as_tensor(cap).long()
        N, Tv, D = video.shape
        Tc, E, H = caption.shape[1], d.word_dim, d.lstm_dim
        Tt = Tv + Tc
        emb = (video.reshape(N * Tv, D) @ pt["encode_image_W"] + pt["encode_image_b"]).reshape(N, Tv, E)
        pad = torch.zeros(N, E, dtype=dt)
        x = lambda t: emb[:, t] if t < Tv else pad

        def run(name, order):
            c = torch.zeros(N, H, dtype=dt); h = torch.zeros(N, H, dtype=dt)
            out = {}
            for t in order:
                _, c, h = T.lstm_cell(x(t), c, h, pt[name + "_W"], pt[name + "_b"])
                out[t] = h
            return out
        fw = run("lstm1_fw", range(Tt))
        bw = run("lstm1_bw", range(Tt - 1, -1, -1))
        c = torch.zeros(N, H, dtype=dt); h = torch.zeros(N, H, dtype=dt)
        g = lambda k, t: torch.as_tensor(drop[k][t]).to(dt)
        for t in range(Tv):
            _, c, h = T.lstm_cell(torch.cat([fw[t], bw[t], pad], 1), c, h, pt["lstm2_W"], pt["lstm2_b"], g("enc2", t), keep)
        logits = []
        for t in range(Tc):
            prev = torch.ones(N, dtype=torch.long) if t == 0 else caption[:, t - 1]
            out, c, h = T.lstm_cell(torch.cat([fw[Tv + t], bw[Tv + t], pt["Wemb"][prev]], 1), c, h, pt["lstm2_W"], pt["lstm2_b"], g("dec2", t), keep)
            logits.append(out @ pt["embed_word_W"] + pt["embed_word_b"])
        return torch.stack(logits, 1)

    def check(self, s, i, state):
        import bidirection_cases as BC
        oracle, d = _orc(), i["d"]
        tiled = np.ascontiguousarray(np.tile(i["video"], (i["S"], 1, 1)))
        ref = BC.teacher_forced(oracle, i["p"], d, tiled, i["cap"], i["vid"], i["sid"], i["keep"], drop_seed=i["seed"])
        tm = np.ascontiguousarray(ref.transpose(1, 0, 2)).reshape(-1, d.n_words)
        assert np.array_equal(state["logits"].cpu().numpy(), tm)
        drop = oracle.dropout_masks(i["seed"], i["vid"], i["sid"], i["keep"], d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step)
        ref_g = _float64_grads(i["p"], lambda pt: self._torch_logits(pt, d, tiled, i["cap"], drop, i["keep"]), i["cap"], i["coef_tm"])
        _assert_grads(state["grads"], ref_g, GRAD_BOUND, "bidir rows" if self.rows else "bidir")


class BidirGreedy(_Family):
    def __init__(self, unshifted, want_logits):
        self.unshifted, self.want_logits = unshifted, want_logits

    def inputs(self, s, variant):
        return _bidir_inputs(s, variant)

    @_stage
    def run(self, ops, env, s, i, state):
        dims, params = _bidir_model(ops, i, state)
        state["out"] = ops.bidir_decode_greedy(dims, params, state["video"], self.unshifted, i["base"], self.want_logits)

    def check(self, s, i, state):
        import bidirection_cases as BC
        ids, logits = BC.greedy(_orc(), i["p"], i["d"], i["video"], i["vid"], unshifted=self.unshifted)
        got = state["out"] if self.want_logits else (state["out"], None)
        assert np.array_equal(got[0].cpu().numpy(), ids), int((got[0].cpu().numpy() != ids).sum())
        if self.want_logits and not self.unshifted:                    # (the other pick may feed other words on: test_gpu_bidirection_fwd.py)
            assert np.array_equal(got[1].cpu().numpy(), logits)


class BidirSample(_Family):
    def inputs(self, s, variant):
        return _bidir_inputs(s, variant, eos_bias=True)

    @_stage
    def run(self, ops, env, s, i, state):
        dims, params = _bidir_model(ops, i, state)
        state["out"] = ops.bidir_sample(dims, params, state["video"], s.S, i["sample_seed"], i["base"], True)

    def check(self, s, i, state):
        import bidirection_rl_cases as RC
        ref_s, ref_g, _ = RC.sample(_orc(), i["p"], i["d"], i["video"], s.S, seed=i["sample_seed"], video_base=i["base"])
        assert np.array_equal(state["out"][0].cpu().numpy(), ref_s) and np.array_equal(state["out"][1].cpu().numpy(), ref_g)


BIDIR_FAMILIES = [BidirTrain(False), BidirTrain(True), BidirGreedy(False, False), BidirGreedy(False, True), BidirGreedy(True, False), BidirGreedy(True, True),
                  BidirSample()]
BIDIR_IDS = ["s2vt_bidir_teacher_forced_fwd+s2vt_bidir_bptt_bwd", "s2vt_bidir_teacher_forced_fwd_rows+s2vt_bidir_bptt_bwd_rows",
             "s2vt_bidir_decode_greedy", "s2vt_bidir_decode_greedy-logits", "s2vt_bidir_decode_greedy-unshifted", "s2vt_bidir_decode_greedy-unshifted-logits",
             "s2vt_bidir_sample"]


@pytest.mark.parametrize("fam", BIDIR_FAMILIES, ids=BIDIR_IDS)
def test_bidirectional_all_checks(gpu, fam):
    _check_A(fam, BIDIR_SMALL)
    _check_B(fam, BIDIR_SMALL, BIDIR_LARGE)
    _check_C(fam, BIDIR_SMALL, BIDIR_LARGE)
    _check_D(fam, BIDIR_SMALL)


# =================================================================================================== 2. beam searches (S2VT, attention, bidirectional)
BeamShape = namedtuple("BeamShape", "B beam")


class Beam(_Family):
    """*_beam_encode + *_beam_step over a whole batched search (beam_generator.BatchedBeamSearch on the model's decoder, whose workspace the
    Provider hands out), then one more step 0 on the same workspace: the stage check D shortens."""
    stage_names = ("search", "one_step")
    LNF = 0.5

    def inputs(self, s, variant):
        m, video = self.model()
        v = video[:s.B] if not variant else np.ascontiguousarray(video[::-1][:s.B] * np.float32(3))
        return dict(m=m, video=np.ascontiguousarray(v, np.float32))

    @_stage
    def search(self, ops, env, s, i, state):
        from s2vt_amd.beam_generator import BatchedBeamSearch
        search = BatchedBeamSearch(i["m"], s.beam, self.LNF)
        state["res"] = search.generate(i["video"])
        state["dec"] = search._dec
        state["tag"] = type(search._dec).__name__
        state["nbytes"] = env.asked[state["tag"]]

    @_stage
    def one_step(self, ops, env, s, i, state):
        dec = state["dec"]
        dec.ws = env.ws(state["nbytes"], state["tag"])
        rows = np.zeros((3, s.B), np.int32)
        rows[0] = np.arange(s.B); rows[2] = 1
        state["step0"] = dec.step(i["m"].store.params, 0, rows, s.beam)

    def check(self, s, i, state):
        for j, (bs, blp, bsc) in enumerate(state["res"]):
            rs, rlp, rsc = self.reference(i["m"], i["video"], j, s.beam)
            assert bs == rs, (j, bs, rs)
            assert self.same(blp, rlp) and self.same(bsc, rsc), (j, blp, rlp, bsc, rsc)

    def same(self, a, b):                                              # test_gpu_attn_beam.py / test_gpu_bidirection_beam.py: the same bits
        return np.float64(a).tobytes() == np.float64(b).tobytes()


class S2VTBeam(Beam):
    """against the per-video BeamSearchGenerator, as test_gpu_beam_batched.py::test_batched_equals_per_video_configs2 (2e-4 on the scores),
    on the model and videos of tests/golden/beam_search.json"""
    _m = {}

    def model(self):
        if not self._m:
            import json
            import test_gpu_beam_batched as BB
            from s2vt_amd import model as M
            oracle = _orc()
            gold = json.load(open(BB.GOLD))
            dm = gold["dims"]
            d = oracle.Dims(label_dim=0, **dm)
            p = oracle.init_params(d, seed=3)
            p["embed_word_W"] *= np.float32(gold["scales"]["embed_word_W"])
            p["lstm1_W"] *= np.float32(gold["scales"]["lstm_W"]); p["lstm2_W"] *= np.float32(gold["scales"]["lstm_W"])
            p["Wemb"] *= np.float32(gold["scales"]["Wemb"])
            p["embed_word_b"][0] += np.float32(gold["eos_bias"]["3"])
            mdl = M.Video_Caption_Generator(dm["dim_image"], dm["n_words"], dm["word_dim"], dm["lstm_dim"], 1, 0, dm["n_video_lstm_step"], dm["n_caption_lstm_step"])
            mdl.store.load(p)
            seen, videos = set(), []
            for c in gold["cases"]:
                v = tuple(c["video"])
                if c["param_seed"] == 3 and v not in seen:
                    seen.add(v); videos.append(np.asarray(c["video"], np.float32).reshape(dm["n_video_lstm_step"], dm["dim_image"]))
            videos = np.stack(videos)                                  # the fixture's three videos, and the same at twice the strength
            self._m["m"] = (mdl, np.concatenate([videos, videos * np.float32(2)]))
        return self._m["m"]

    def reference(self, m, video, j, k):
        from s2vt_amd.beam_generator import BeamSearchGenerator
        return BeamSearchGenerator(m, k, self.LNF).generate(video[j:j + 1])

    def same(self, a, b):
        import test_gpu_beam_batched as BB
        return BB._close(a, b)


class AttnBeam(Beam):
    _m = {}

    def model(self):
        if not self._m:
            import torch
            import test_gpu_attn_beam as AB
            _, _, mdl, video, _ = AB._model(_orc(), 24, 60, 20, 5, 7, 6, 3, scaled=True)
            with torch.no_grad():
                mdl.p["embed_word_b"][0] += 20.0                      # (test_gpu_attn_beam.py::_sweep: captions of both kinds)
            self._m["m"] = (mdl, video)
        return self._m["m"]

    def reference(self, m, video, j, k):
        import test_gpu_attn_beam as AB
        from s2vt_amd import ops
        return AB._per_video_search(AB._teacher_forced_step(ops, m, video[j], k), m.n_caption_lstm_steps, k, self.LNF)


class BidirBeam(Beam):
    _m = {}

    def model(self):
        if not self._m:
            import bidirection_beam_cases as BBC
            import test_gpu_bidirection_beam as TB
            p, d, video = BBC.case(_orc())
            self._m["m"] = (TB._generator(p, d, video.shape[0]), video)
        return self._m["m"]

    def reference(self, m, video, j, k):
        """test_gpu_bidirection_beam.py's independent driver; its cache of teacher-forced rows is keyed by the video's index in ITS case, so
        the rows are computed here without it"""
        import torch
        import test_gpu_bidirection_beam as TB
        from s2vt_amd import ops
        Tc, V = m.n_caption_lstm_step, m.n_words
        vj = torch.as_tensor(np.ascontiguousarray(video[j:j + 1])).cuda()

        def step(t, prefixes):
            rows = []
            for sent in prefixes:
                cap = np.zeros((1, Tc), np.int32)
                cap[0, :len(sent)] = sent
                rows.append(m.teacher_forced_logits(vj, torch.as_tensor(cap).cuda(), keep=1.0).view(Tc, V)[t].clone())
            ids, lp = ops.vocab_topk(torch.stack(rows).contiguous(), k)
            return ids.cpu().numpy(), lp.cpu().numpy()
        return TB._per_video_search(step, Tc, k, self.LNF)


@pytest.mark.parametrize("fam,small,large", [(S2VTBeam(), BeamShape(3, 3), BeamShape(6, 5)), (AttnBeam(), BeamShape(3, 3), BeamShape(6, 5)),
                                             (BidirBeam(), BeamShape(3, 2), BeamShape(5, 3))],
                         ids=["s2vt_beam_encode+s2vt_beam_step", "s2vt_attn_beam_encode+s2vt_attn_beam_step", "s2vt_bidir_beam_encode+s2vt_bidir_beam_step"])
def test_beam_search_all_checks(gpu, fam, small, large):
    """shrink in B and in beam"""
    _check_A(fam, small)
    _check_B(fam, small, large)
    _check_C(fam, small, large)
    _check_D(fam, small)
