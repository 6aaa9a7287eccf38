"""Thin torch-tensor wrappers over the C ABI (include/s2vt.h).  torch is plumbing here: device
memory, the current HIP stream, dtype checks.  All compute happens in libs2vt_hip.so."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import AttnParams, Dims, Operand, Params, check, lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk_f32(*ts):
    for t in ts:
        if t is not None:
            assert t.is_cuda and t.dtype == torch.float32, "expected a CUDA float32 tensor"


def make_dims(dim_image, n_words, word_dim, lstm_dim, n_video_lstm_step, n_caption_lstm_step, label_dim=0, residual=False) -> Dims:
    """residual: the model bit S2VT_MODEL_RESIDUAL (residual_tf_s2vt.py: out1 + out2 into the vocabulary projection), carried in the
    struct's spare word into every call that takes the dims."""
    return Dims(dim_image, n_words, word_dim, lstm_dim, n_video_lstm_step, n_caption_lstm_step, label_dim,
                _lib.MODEL_RESIDUAL if residual else 0)


def make_params(tensors: dict) -> Params:
    """tensors: name -> CUDA fp32 tensor (names = _lib.PARAM_FIELDS; missing ones become NULL)."""
    p = Params()
    for n in _lib.PARAM_FIELDS:
        t = tensors.get(n)
        if t is not None:
            _chk_f32(t)
            assert t.is_contiguous()
        setattr(p, n, None if t is None else t.data_ptr())
    return p


def operand(t, k=None, rowidx=None, rowmod=0, ld=None) -> Operand:
    """A K-segment of a concatenated operand.  t=None -> zero input of width k."""
    if t is None:
        return Operand(None, None, 0, int(k), 0, 0)
    _chk_f32(t)
    assert t.dim() == 2 and t.stride(1) == 1
    if rowidx is not None:
        assert rowidx.is_cuda and rowidx.dtype == torch.int32 and rowidx.is_contiguous()
    op = Operand(t.data_ptr(), None if rowidx is None else rowidx.data_ptr(), int(ld if ld is not None else t.stride(0)),
                 int(k if k is not None else t.shape[1]), int(rowmod), 0)
    op._keep = (t, rowidx)          # the struct holds raw pointers: keep the tensors alive with it
    return op


def math_eval(fn: str, x):
    _chk_f32(x)
    y = torch.empty_like(x)
    code = {"exp": 0, "log": 1, "tanh": 2, "sigmoid": 3}[fn]
    check(lib().s2vt_math_eval(code, _ptr(x), _ptr(y), x.numel(), _stream()), "s2vt_math_eval")
    return y


def gumbel_eval(seed, video, sample, step, V, device="cuda"):
    out = torch.empty(V, dtype=torch.float32, device=device)
    check(lib().s2vt_gumbel_eval(seed, video, sample, step, _ptr(out), V, _stream()), "s2vt_gumbel_eval")
    return out


def gumbel_words_eval(words):
    """(exact, fast): gumbel_from_word and gumbel_fast_from_word of each Philox word (int32 / uint32 bits, a contiguous device tensor)."""
    assert words.is_cuda and words.is_contiguous() and words.element_size() == 4 and not words.dtype.is_floating_point
    exact = torch.empty(words.shape, dtype=torch.float32, device=words.device)
    fast = torch.empty_like(exact)
    check(lib().s2vt_gumbel_words_eval(_ptr(words), _ptr(exact), _ptr(fast), words.numel(), _stream()), "s2vt_gumbel_words_eval")
    return exact, fast


def gemm(segs, W, bias=None, M=None, cinit=None, act_tanh=False, tile_cfg=-1, out=None):
    """C = act([seg0 ; seg1 ; seg2] @ W + bias), continuing the chain from cinit if given."""
    _chk_f32(W, bias, cinit)
    assert W.dim() == 2 and W.stride(1) == 1
    N = W.shape[1]
    arr = (Operand * len(segs))(*segs)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=W.device)
    check(lib().s2vt_gemm(arr, len(segs), _ptr(W), W.stride(0), _ptr(bias), _ptr(cinit),
                          0 if cinit is None else cinit.stride(0), _ptr(out), out.stride(0), M, N, int(act_tanh), tile_cfg,
                          _stream()), "s2vt_gemm")
    return out


def gemm_nt(segs, Wt, bias=None, M=None, cinit=None, act_tanh=False, tile_cfg=-1, out=None):
    """C = act([seg0 ; seg1 ; seg2] @ Wt^T + bias) with Wt [N, K] (K contiguous): the weight matrix as the backward reads it."""
    _chk_f32(Wt, bias, cinit)
    assert Wt.dim() == 2 and Wt.stride(1) == 1
    N = Wt.shape[0]
    arr = (Operand * len(segs))(*segs)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=Wt.device)
    check(lib().s2vt_gemm_nt(arr, len(segs), _ptr(Wt), Wt.stride(0), _ptr(bias), _ptr(cinit),
                             0 if cinit is None else cinit.stride(0), _ptr(out), out.stride(0), M, N, int(act_tanh), tile_cfg,
                             _stream()), "s2vt_gemm_nt")
    return out


def gemm_nt_splitk(A, Wt, splits=0, tile_cfg=-1, out=None, slabs=None):
    """C = A @ Wt^T with the reduction cut into K slabs that are summed (order-free: gradients only).  splits = 0: the
    library's choice for the shape."""
    _chk_f32(A, Wt)
    M, K = A.shape
    N = Wt.shape[0]
    assert Wt.shape[1] == K and A.stride(1) == 1 and Wt.stride(1) == 1
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    if slabs is None:
        slabs = torch.empty((max(splits, 12) + 1) * M * N, dtype=torch.float32, device=A.device)
    check(lib().s2vt_gemm_nt_splitk(_ptr(A), A.stride(0), _ptr(Wt), Wt.stride(0), _ptr(out), out.stride(0), M, N, K, int(splits),
                                    int(tile_cfg), _ptr(slabs), slabs.numel(), _stream()), "s2vt_gemm_nt_splitk")
    return out


def lstm_cell_fwd(x0, x1, h_prev, c_prev, W, b, M, state_rowmod=0, keep=1.0, seed=0, video_id=None, sample_id=None,
                  drop_code=0, want_gates=False, tile_cfg=-1, res=None):
    """res (an Operand of width H): the residual form, out = dropout(h') + res[row(m)] (s2vt_lstm_cell_fwd_res)."""
    _chk_f32(h_prev, c_prev, W, b)
    H = W.shape[1] // 4
    dev = W.device
    c = torch.empty((M, H), dtype=torch.float32, device=dev)
    h = torch.empty_like(c)
    out = torch.empty_like(c)
    gates = torch.empty((M, 4 * H), dtype=torch.float32, device=dev) if want_gates else None
    if res is not None:
        check(lib().s2vt_lstm_cell_fwd_res(None if x0 is None else C.byref(x0), None if x1 is None else C.byref(x1), _ptr(h_prev),
                                           _ptr(c_prev), state_rowmod, _ptr(W), _ptr(b), C.byref(res), _ptr(c), _ptr(h), _ptr(out),
                                           _ptr(gates), M, H, float(keep), seed, _ptr(video_id), _ptr(sample_id), drop_code, tile_cfg,
                                           _stream()), "s2vt_lstm_cell_fwd_res")
        return c, h, out, gates
    check(lib().s2vt_lstm_cell_fwd(None if x0 is None else C.byref(x0), None if x1 is None else C.byref(x1), _ptr(h_prev),
                                   _ptr(c_prev), state_rowmod, _ptr(W), _ptr(b), _ptr(c), _ptr(h), _ptr(out), _ptr(gates),
                                   M, H, float(keep), seed, _ptr(video_id), _ptr(sample_id), drop_code, tile_cfg, _stream()),
          "s2vt_lstm_cell_fwd")
    return c, h, out, gates


def lstm_recurrence_fwd(W, kw0, b, h0, c0, T, cinit=None, cinit_steps=0, keep=1.0, seed=0, video_id=None, sample_id=None,
                        drop_code0=0, want_gates=True, want_out=False, persistent=-1, gates_in_cinit=False):
    """T steps of one BasicLSTMCell on the recurrent rows W[kw0:kw0+H] (+ the carried partials cinit [steps, M, 4H]).
    Returns (C_hist [T+1,M,H], H_hist [T+1,M,H], gates [T,M,4H] | None, out [T,M,H] | None).
    persistent: 1 = the one-launch persistent form, 0 = per-step launches, -1 = auto.  gates_in_cinit: write the gates over cinit."""
    _chk_f32(W, b, h0, c0, cinit)
    M, H = h0.shape
    dev = W.device
    Ch = torch.empty((T + 1, M, H), dtype=torch.float32, device=dev); Hh = torch.empty_like(Ch)
    Ch[0].copy_(c0); Hh[0].copy_(h0)
    if gates_in_cinit:
        assert cinit is not None and cinit.shape[0] == T
        gates = cinit
    else:
        gates = torch.empty((T, M, 4 * H), dtype=torch.float32, device=dev) if want_gates else None
    out = torch.empty((T, M, H), dtype=torch.float32, device=dev) if want_out else None
    nb = lib().s2vt_lstm_recurrence_scratch_bytes(H)
    ws = workspace(nb, dev, "chain")
    check(lib().s2vt_lstm_recurrence_fwd(_ptr(W), kw0, _ptr(b), _ptr(cinit), 0 if cinit is None else cinit.stride(0),
                                         0 if cinit is None else cinit.stride(1), cinit_steps, _ptr(Ch), _ptr(Hh), _ptr(gates), _ptr(out),
                                         M, H, T, float(keep), seed, _ptr(video_id), _ptr(sample_id), drop_code0, persistent, _ptr(ws),
                                         ws.numel(), _stream()), "s2vt_lstm_recurrence_fwd")
    return Ch, Hh, gates, out


def lstm_dir(W, kw0, b, h0, c0, T, cinit=None, cinit_t0=0, reverse=False, want_gates=True) -> _lib.LstmDir:
    """One direction of lstm_birecurrence_fwd, in chain-step order: histories [T+1, M, H] with slot 0 = (c0, h0); cinit
    [steps, M, 4H] is the carried partial of chain steps cinit_t0 .. cinit_t0 + steps - 1, consumed last slice first if
    `reverse` (the backward direction reads the frame products in descending time).  The tensors ride on the struct as
    .C / .H / .gates."""
    _chk_f32(W, b, h0, c0, cinit)
    M, H = h0.shape
    dev = W.device
    Ch = torch.empty((T + 1, M, H), dtype=torch.float32, device=dev); Hh = torch.empty_like(Ch)
    Ch[0].copy_(c0); Hh[0].copy_(h0)
    gates = torch.empty((T, M, 4 * H), dtype=torch.float32, device=dev) if want_gates else None
    d = _lib.LstmDir()
    d.W, d.kw0, d.b = W.data_ptr(), int(kw0), b.data_ptr()
    if cinit is not None:
        assert cinit.dim() == 3 and cinit.shape[1] == M and cinit.stride(2) == 1
        steps = cinit.shape[0]
        d.cinit = cinit.data_ptr() + (4 * (steps - 1) * cinit.stride(0) if reverse else 0)
        d.cinit_tstride = -cinit.stride(0) if reverse else cinit.stride(0)
        d.ldcinit, d.cinit_t0, d.cinit_steps = cinit.stride(1), int(cinit_t0), steps
    d.C_hist, d.H_hist, d.gates = Ch.data_ptr(), Hh.data_ptr(), None if gates is None else gates.data_ptr()
    d.C, d.H, d.gates_t = Ch, Hh, gates
    d._keep = (W, b, cinit)         # the struct holds raw pointers: keep the tensors alive with it
    return d


def lstm_birecurrence_fwd(fw: _lib.LstmDir, bw: _lib.LstmDir, persistent=-1):
    """Both LSTM1 directions of the bidirectional captioner (s2vt_lstm_birecurrence_fwd): fills the histories of the two
    lstm_dir() descriptions.  persistent: 1 = one persistent launch for both directions (M <= 64), 0 = per-step launches,
    2 = one persistent recurrence per direction, -1 = the library's choice.  Every form gives the bits of two lstm_recurrence_fwd calls."""
    T, M, H = fw.C.shape[0] - 1, fw.C.shape[1], fw.C.shape[2]
    assert bw.C.shape == fw.C.shape
    nb = lib().s2vt_lstm_birecurrence_scratch_bytes(H)
    ws = workspace(nb, fw.C.device, "bichain")
    check(lib().s2vt_lstm_birecurrence_fwd(C.byref(fw), C.byref(bw), M, H, T, persistent, _ptr(ws), ws.numel(), _stream()),
          "s2vt_lstm_birecurrence_fwd")
    return (fw.C, fw.H, fw.gates_t), (bw.C, bw.H, bw.gates_t)


def make_bidir_params(tensors: dict) -> _lib.BidirParams:
    """tensors: name -> contiguous CUDA fp32 tensor for every name in _lib.BIDIR_PARAM_FIELDS (s2vt_bidir_params)."""
    p = _lib.BidirParams()
    for n in _lib.BIDIR_PARAM_FIELDS:
        t = tensors[n]
        _chk_f32(t)
        assert t.is_contiguous()
        setattr(p, n, t.data_ptr())
    p._keep = tensors
    return p


def bidir_workspace(dims: Dims, B: int, device):
    nb = lib().s2vt_bidir_workspace_bytes(C.byref(dims), B)
    assert nb > 0
    return torch.empty(nb, dtype=torch.uint8, device=device)


def bidir_teacher_forced_fwd(dims: Dims, params, video, caption, ws, keep=1.0, seed=0, video_id=None, sample_id=None, lstm1_form=-1, out=None):
    """build_model's logits of the bidirectional captioner, time-major [Tc * B, V] (s2vt_bidir_teacher_forced_fwd); ws keeps the state
    bidir_bptt_bwd needs."""
    _chk_f32(video)
    B = video.shape[0]
    assert video.is_contiguous() and caption.is_cuda and caption.dtype == torch.int32 and caption.is_contiguous()
    if out is None:
        out = torch.empty((dims.n_caption_lstm_step * B, dims.n_words), dtype=torch.float32, device=video.device)
    check(lib().s2vt_bidir_teacher_forced_fwd(C.byref(dims), C.byref(params), _ptr(video), B, _ptr(caption), float(keep), seed, _ptr(video_id),
                                              _ptr(sample_id), lstm1_form, _ptr(out), _ptr(ws), ws.numel(), _stream()), "s2vt_bidir_teacher_forced_fwd")
    return out


def bidir_bptt_bwd(dims: Dims, params, grads, video, dlogits, ws, keep=1.0, seed=0, video_id=None, sample_id=None):
    """Adds the gradient products of all eleven variables into `grads` (a make_bidir_params of zeroed tensors)."""
    _chk_f32(video, dlogits)
    assert dlogits.is_contiguous()
    check(lib().s2vt_bidir_bptt_bwd(C.byref(dims), C.byref(params), C.byref(grads), _ptr(video), video.shape[0], _ptr(dlogits), float(keep), seed,
                                    _ptr(video_id), _ptr(sample_id), _ptr(ws), ws.numel(), _stream()), "s2vt_bidir_bptt_bwd")


def bidir_decode_greedy(dims: Dims, params, video, unshifted_softmax=False, video_base=0, want_logits=False, lstm1_form=-1, ids=None, logits=None):
    """Greedy decode of B videos (s2vt_bidir_decode_greedy): ids int32 [B, Tc] (and logits [B, Tc, V])."""
    _chk_f32(video)
    assert video.is_contiguous()
    B = video.shape[0]
    if ids is None:
        ids = torch.empty((B, dims.n_caption_lstm_step), dtype=torch.int32, device=video.device)
    if want_logits and logits is None:
        logits = torch.empty((B, dims.n_caption_lstm_step, dims.n_words), dtype=torch.float32, device=video.device)
    nb = lib().s2vt_bidir_decode_workspace_bytes(C.byref(dims), B)
    ws = workspace(nb, video.device, "bidir_decode")
    check(lib().s2vt_bidir_decode_greedy(C.byref(dims), C.byref(params), _ptr(video), B, int(bool(unshifted_softmax)), int(video_base), lstm1_form,
                                         _ptr(ids), _ptr(logits), _ptr(ws), ws.numel(), _stream()), "s2vt_bidir_decode_greedy")
    return (ids, logits) if want_logits else ids


def bidir_sample(dims: Dims, params, video, K: int, seed: int = 0, video_base: int = 0, with_greedy: bool = True, lstm1_form=-1, out=None, ids=None):
    """K multinomial captions per video (+ the greedy one) of the bidirectional captioner (s2vt_bidir_sample): (sampled [K * B, Tc] | None,
    greedy [B, Tc] | None) int32, sample-major rows.  out / ids: windows for the sampled / greedy block."""
    _chk_f32(video)
    assert video.is_contiguous() and K >= 0 and (K > 0 or with_greedy)
    B, Tc = video.shape[0], dims.n_caption_lstm_step
    if K > 0 and out is None:
        out = torch.empty((K * B, Tc), dtype=torch.int32, device=video.device)
    if with_greedy and ids is None:
        ids = torch.empty((B, Tc), dtype=torch.int32, device=video.device)
    nb = lib().s2vt_bidir_sample_workspace_bytes(C.byref(dims), B, int(K), int(bool(with_greedy)))
    assert nb > 0
    ws = workspace(nb, video.device, "bidir_sample")
    check(lib().s2vt_bidir_sample(C.byref(dims), C.byref(params), _ptr(video), B, int(K), int(bool(with_greedy)), int(seed), int(video_base), lstm1_form,
                                  _ptr(out if K > 0 else None), _ptr(ids if with_greedy else None), _ptr(ws), ws.numel(), _stream()), "s2vt_bidir_sample")
    return (out if K > 0 else None), (ids if with_greedy else None)


def bidir_sample_sum(dz, B: int, S: int, out=None):
    """dz [T, S * B, C] (sample-major rows) -> [T, B, C]: the sum over a video's S rows in ascending s, no atomics (s2vt_bidir_sample_sum)."""
    _chk_f32(dz, out)
    T, N, Cc = dz.shape
    assert N == S * B and dz.is_contiguous()
    if out is None:
        out = torch.empty((T, B, Cc), dtype=torch.float32, device=dz.device)
    check(lib().s2vt_bidir_sample_sum(_ptr(dz), _ptr(out), T, B, S, Cc, _stream()), "s2vt_bidir_sample_sum")
    return out


def bidir_rows_workspace(dims: Dims, B: int, S: int, device):
    nb = lib().s2vt_bidir_rows_workspace_bytes(C.byref(dims), B, S)
    assert nb > 0
    return torch.empty(nb, dtype=torch.uint8, device=device)


def bidir_teacher_forced_fwd_rows(dims: Dims, params, video, caption, ws, keep=1.0, seed=0, video_id=None, sample_id=None, lstm1_form=-1, out=None):
    """The teacher-forced logits of the N = S * B sample-major rows caption [N, Tc] on the B videos video [B, Tv, D], time-major [Tc * N, V]
    (s2vt_bidir_teacher_forced_fwd_rows): the bits of bidir_teacher_forced_fwd on the S-times tiled block; ws (bidir_rows_workspace) keeps
    the state bidir_bptt_bwd_rows needs."""
    _chk_f32(video)
    B, N = video.shape[0], caption.shape[0]
    assert video.is_contiguous() and caption.is_cuda and caption.dtype == torch.int32 and caption.is_contiguous() and N % B == 0 and N >= B
    if out is None:
        out = torch.empty((dims.n_caption_lstm_step * N, dims.n_words), dtype=torch.float32, device=video.device)
    check(lib().s2vt_bidir_teacher_forced_fwd_rows(C.byref(dims), C.byref(params), _ptr(video), B, N // B, _ptr(caption), float(keep), seed, _ptr(video_id),
                                                   _ptr(sample_id), lstm1_form, _ptr(out), _ptr(ws), ws.numel(), _stream()),
          "s2vt_bidir_teacher_forced_fwd_rows")
    return out


def bidir_bptt_bwd_rows(dims: Dims, params, grads, video, S, dlogits, ws, keep=1.0, seed=0, video_id=None, sample_id=None):
    """The backward of bidir_teacher_forced_fwd_rows on the same ws: adds the gradient products of all eleven variables into `grads`."""
    _chk_f32(video, dlogits)
    assert dlogits.is_contiguous() and video.is_contiguous()
    check(lib().s2vt_bidir_bptt_bwd_rows(C.byref(dims), C.byref(params), C.byref(grads), _ptr(video), video.shape[0], int(S), _ptr(dlogits), float(keep),
                                         seed, _ptr(video_id), _ptr(sample_id), _ptr(ws), ws.numel(), _stream()), "s2vt_bidir_bptt_bwd_rows")


def lstm_recurrence_bwd(W, kw0, gates, C_hist, dext=None, dext_t0=0, keep=1.0, seed=0, video_id=None, sample_id=None, drop_code0=0,
                        persistent=-1, precision="fp32"):
    """Back-propagation through lstm_recurrence_fwd's unroll: returns dZ [T, M, 4H].  gates [T, M, 4H] activated, C_hist
    [T+1, M, H], dext [T - dext_t0, M, H] = gradient w.r.t. the (dropped) outputs of steps dext_t0 .. T-1 or None.
    persistent: 1 = the one-launch form, 0 = per-step launches, -1 = auto.
    precision: "fp32", or "split" = dz @ Whh^T as three bf16 products on split operands (persistent = 1 above 256 rows only:
    S2VT_E_BADARG elsewhere)."""
    assert precision in ("fp32", "split")
    _chk_f32(W, gates, C_hist, dext)
    T, M, H4 = gates.shape
    H = H4 // 4
    assert gates.is_contiguous() and C_hist.is_contiguous() and C_hist.shape == (T + 1, M, H)
    if dext is not None:
        assert dext.is_contiguous() and dext.shape == (T - dext_t0, M, H)
    dZ = torch.empty((T, M, 4 * H), dtype=torch.float32, device=W.device)
    nb = lib().s2vt_lstm_recurrence_bwd_scratch_bytes(M, H)
    ws = workspace(nb, W.device, "bchain")
    name = "s2vt_lstm_recurrence_bwd_split" if precision == "split" else "s2vt_lstm_recurrence_bwd"
    check(getattr(lib(), name)(_ptr(W), kw0, _ptr(gates), _ptr(C_hist), _ptr(dext), M * H, H, dext_t0, _ptr(dZ), M, H, T, float(keep),
                               seed, _ptr(video_id), _ptr(sample_id), drop_code0, persistent, _ptr(ws), ws.numel(), _stream()), name)
    return dZ


def chain_timeouts() -> int:
    """Timed-out grid-wide waits of the persistent recurrence so far (0 = healthy); synchronises the device."""
    torch.cuda.synchronize()
    return int(lib().s2vt_chain_timeouts())


def vocab_pick(out2, W, b, video_id, sample_id, step, seed, want_logits=False, tile_cfg=-1):
    _chk_f32(out2, W, b)
    M, H = out2.shape
    V = W.shape[1]
    packed = torch.zeros(M, dtype=torch.int64, device=out2.device)
    tok = torch.empty(M, dtype=torch.int32, device=out2.device)
    logits = torch.empty((M, V), dtype=torch.float32, device=out2.device) if want_logits else None
    check(lib().s2vt_vocab_pick(_ptr(out2), out2.stride(0), _ptr(W), _ptr(b), M, H, V, _ptr(video_id), _ptr(sample_id),
                                step, seed, _ptr(packed), _ptr(tok), _ptr(logits), tile_cfg, _stream()), "s2vt_vocab_pick")
    return tok, logits, packed


def tile_count(kind: int) -> int:
    """Entries of a tile table (kind = the profiler's kernel_class: _lib.TILE_STORE / TILE_LSTM / TILE_PICK / TILE_STORE_NT)."""
    n = lib().s2vt_tile_count(kind)
    if n < 0:
        check(n, "s2vt_tile_count")
    return n


def tile_info(kind: int, tile_cfg: int) -> dict:
    """Entry tile_cfg of a tile table: rows, cols, name, fallback (-1: none), has_scalar, has_live."""
    d = _lib.TileDesc()
    check(lib().s2vt_tile_info(kind, tile_cfg, C.byref(d)), "s2vt_tile_info")
    return dict(rows=d.rows, cols=d.cols, name=d.name.decode(), fallback=d.fallback, has_scalar=bool(d.has_scalar), has_live=bool(d.has_live))


def _chk_live(live, n_live):
    for t in (live, n_live):
        if t is not None:
            assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()


def gemm_live(segs, W, out, live=None, n_live=None, bias=None, cinit=None, act_tanh=False, tile_cfg=-1):
    """s2vt_gemm on the rows live[0 .. n_live) of `out` ([M, N]: M is the capacity); the other rows of `out` are left as they are."""
    _chk_f32(W, bias, cinit, out)
    _chk_live(live, n_live)
    assert W.dim() == 2 and W.stride(1) == 1 and out.stride(1) == 1
    M, N = out.shape[0], W.shape[1]
    arr = (Operand * len(segs))(*segs)
    check(lib().s2vt_gemm_live(arr, len(segs), _ptr(W), W.stride(0), _ptr(bias), _ptr(cinit), 0 if cinit is None else cinit.stride(0),
                               _ptr(out), out.stride(0), M, N, int(act_tanh), _ptr(live), _ptr(n_live), tile_cfg, _stream()), "s2vt_gemm_live")
    return out


def lstm_cell_fwd_live(x0, x1, h_prev, c_prev, W, b, c_new, h_new, out, gates=None, live=None, n_live=None, state_rowmod=0, keep=1.0, seed=0,
                       video_id=None, sample_id=None, drop_code=0, tile_cfg=-1, res=None):
    """The cell step (plain, or residual when res is given) on the rows live[0 .. n_live) of c_new / h_new / out / gates ([M, .])."""
    _chk_f32(h_prev, c_prev, W, b, c_new, h_new, out, gates)
    _chk_live(live, n_live)
    M, H = c_new.shape[0], W.shape[1] // 4
    check(lib().s2vt_lstm_cell_fwd_live(None if x0 is None else C.byref(x0), None if x1 is None else C.byref(x1), _ptr(h_prev), _ptr(c_prev),
                                        state_rowmod, _ptr(W), _ptr(b), None if res is None else C.byref(res), _ptr(c_new), _ptr(h_new),
                                        _ptr(out), _ptr(gates), M, H, float(keep), seed, _ptr(video_id), _ptr(sample_id), drop_code,
                                        _ptr(live), _ptr(n_live), tile_cfg, _stream()), "s2vt_lstm_cell_fwd_live")
    return c_new, h_new, out, gates


def lstm_cell_fwd_gather(x0, x1, h_prev, c_prev, W, b, M, state_rowidx=None, cinit=None, cinit_rowidx=None, want_gates=False, tile_cfg=-1,
                         c_new=None, h_new=None, gates=None):
    """The gathered-state cell step (s2vt_lstm_cell_fwd_gather): launch row m continues h_prev / c_prev row state_rowidx[m] and the carried
    partial cinit row cinit_rowidx[m] (int32 device arrays of M entries; None: row m), no dropout.  Returns (c_new, h_new, gates | None),
    [M, H] / [M, 4H]; given outputs are written in place and must not overlap the state they are gathered from."""
    _chk_f32(h_prev, c_prev, W, b, cinit, c_new, h_new, gates)
    _chk_live(state_rowidx, cinit_rowidx)
    H = W.shape[1] // 4
    dev = W.device
    c_new = torch.empty((M, H), dtype=torch.float32, device=dev) if c_new is None else c_new
    h_new = torch.empty((M, H), dtype=torch.float32, device=dev) if h_new is None else h_new
    if gates is None and want_gates:
        gates = torch.empty((M, 4 * H), dtype=torch.float32, device=dev)
    assert cinit is None or (cinit.dim() == 2 and cinit.stride(1) == 1)
    check(lib().s2vt_lstm_cell_fwd_gather(None if x0 is None else C.byref(x0), None if x1 is None else C.byref(x1), _ptr(h_prev), _ptr(c_prev),
                                          _ptr(state_rowidx), _ptr(cinit), 0 if cinit is None else cinit.stride(0), _ptr(cinit_rowidx), _ptr(W),
                                          _ptr(b), _ptr(c_new), _ptr(h_new), _ptr(gates), int(M), H, tile_cfg, _stream()),
          "s2vt_lstm_cell_fwd_gather")
    return c_new, h_new, gates


def vocab_pick_live(out2, W, b, video_id, sample_id, step, seed, packed, live=None, n_live=None, pick_stride=1, logits=None, tile_cfg=-1):
    """s2vt_vocab_pick on the rows live[0 .. n_live): packed[r * pick_stride] (zero on entry for those rows) receives row r's word,
    whose low half is ~token; logits (optional, [M, V]) its logits."""
    _chk_f32(out2, W, b, logits)
    _chk_live(live, n_live)
    M, H = out2.shape
    check(lib().s2vt_vocab_pick_live(_ptr(out2), out2.stride(0), _ptr(W), _ptr(b), M, H, W.shape[1], _ptr(video_id), _ptr(sample_id), step,
                                     seed, _ptr(packed), pick_stride, _ptr(logits), _ptr(live), _ptr(n_live), tile_cfg, _stream()),
          "s2vt_vocab_pick_live")
    return packed, logits


def frame_embed_fwd(dims: Dims, params: Params, video):
    _chk_f32(video)
    B = video.shape[0]
    emb = torch.empty((B * dims.n_video_lstm_step, dims.word_dim), dtype=torch.float32, device=video.device)
    check(lib().s2vt_frame_embed_fwd(C.byref(dims), C.byref(params), _ptr(video), B, _ptr(emb), _stream()),
          "s2vt_frame_embed_fwd")
    return emb


def zero_(*tensors):
    """Zero up to 8 device tensors (contiguous) with ONE library launch (s2vt_zero_regions)."""
    ts = [t for t in tensors if t is not None and t.numel()]
    for i in range(0, len(ts), 8):
        grp = ts[i:i + 8]
        for t in grp:
            assert t.is_cuda and t.is_contiguous() and (t.numel() * t.element_size()) % 4 == 0
        ptrs = (C.c_void_p * len(grp))(*[t.data_ptr() for t in grp])
        nb = (C.c_size_t * len(grp))(*[t.numel() * t.element_size() for t in grp])
        check(lib().s2vt_zero_regions(ptrs, nb, len(grp), _stream()), "s2vt_zero_regions")


_ws_cache = {}


def workspace(nbytes: int, device, tag="default"):
    """A cached, 256-byte aligned device scratch buffer (torch owns the memory)."""
    key = (tag, str(device))
    t = _ws_cache.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        assert t.data_ptr() % 256 == 0
        _ws_cache[key] = t
    return t


def sample(dims: Dims, params: Params, video, K: int, seed: int, video_base: int = 0, with_greedy: bool = True, stop_at_eos: bool = False):
    """K multinomial captions per video (+ greedy).  Returns (sampled [K*B,Tc], greedy [B,Tc]) int32.
    stop_at_eos (opt-in, not the reference's behaviour): a row leaves the loop once it has picked <eos>; its later ids are 0.  Ids up to
    and including the first <eos> -- the positions the objective's mask keeps -- are unchanged."""
    _chk_f32(video)
    assert video.is_contiguous()
    B = video.shape[0]
    g = 1 if with_greedy else 0
    L = lib()
    nbytes = L.s2vt_sample_workspace_bytes(C.byref(dims), B, K, g)
    ws = workspace(nbytes, video.device, "sample")
    ids = torch.empty(((K + g) * B, dims.n_caption_lstm_step), dtype=torch.int32, device=video.device)
    if stop_at_eos:
        check(L.s2vt_sample_ex(C.byref(dims), C.byref(params), _ptr(video), B, K, g, seed, video_base, 1, _ptr(ids), _ptr(ws),
                               ws.numel(), _stream()), "s2vt_sample_ex")
    else:
        # the screened pick (same ids) where the library serves the shape; its scratch is a block of its own, the sampler workspace is unchanged
        sbytes = L.s2vt_sample_screen_workspace_bytes(C.byref(dims), B, K, g)
        if sbytes > 0:
            sws = workspace(sbytes, video.device, "sample_screen")
            check(L.s2vt_sample_screened(C.byref(dims), C.byref(params), _ptr(video), B, K, g, seed, video_base, _ptr(ids), _ptr(ws),
                                         ws.numel(), _ptr(sws), sws.numel(), _stream()), "s2vt_sample_screened")
        else:
            check(L.s2vt_sample(C.byref(dims), C.byref(params), _ptr(video), B, K, g, seed, video_base, _ptr(ids), _ptr(ws),
                                ws.numel(), _stream()), "s2vt_sample")
    sample.serial += 1                                                 # the workspace is shared by every caller: a later call overwrites it
    sample.last_state = (ws, (K + g) * B, video.data_ptr(), B, sample.serial)   # for teacher_forced_fwd(sampler_state=...)
    return ids[:K * B], (ids[K * B:] if with_greedy else None)


sample.last_state = None
sample.serial = 0


def sample_mix(dims: Dims, params: Params, video, caption, p_gt: float, seed: int, video_base: int = 0, with_greedy: bool = True):
    """The mixed decode of build_mix_sample (s2vt_sample_mix): a greedy decode whose fed word at step t >= 1 is caption[:, t-1] with
    probability p_gt (the coin: a pure function of seed, global video id and step) and the row's own argmax otherwise; with_greedy adds the
    plain greedy rows from the same encode.  caption: int32 device tensor [B, Tc] (ids outside [0, n_words) are clamped by the kernel).
    Returns (mix [B,Tc], greedy [B,Tc] | None) int32.  A workspace of its own: sample.last_state is left alone, so
    teacher_forced_fwd(sampler_state=...) never sees a mixed call's buffers."""
    _chk_f32(video)
    assert video.is_contiguous()
    B = video.shape[0]
    assert caption.is_cuda and caption.dtype == torch.int32 and caption.is_contiguous()
    assert tuple(caption.shape) == (B, dims.n_caption_lstm_step)
    g = 1 if with_greedy else 0
    L = lib()
    nbytes = L.s2vt_sample_mix_workspace_bytes(C.byref(dims), B, g)
    ws = workspace(nbytes, video.device, "sample_mix")
    ids = torch.empty(((1 + g) * B, dims.n_caption_lstm_step), dtype=torch.int32, device=video.device)
    check(L.s2vt_sample_mix(C.byref(dims), C.byref(params), _ptr(video), B, _ptr(caption), float(p_gt), g, seed, video_base, _ptr(ids),
                            _ptr(ws), ws.numel(), _stream()), "s2vt_sample_mix")
    return ids[:B], (ids[B:] if with_greedy else None)


def train_workspace(dims: Dims, B: int, N: int, device):
    nbytes = lib().s2vt_train_workspace_bytes(C.byref(dims), B, N)
    assert nbytes > 0, "bad dims / B / N (N must be a multiple of B)"
    return workspace(nbytes, device, "train")


def teacher_forced_fwd(dims: Dims, params: Params, video, caption, N: int, keep=1.0, seed=0, video_id=None,
                       sample_id=None, ws=None, logits=None, sampler_state=None, steps=None, live=None, split=False):
    """Teacher-forced unroll on N = rep*B sample-major rows.  Returns time-major logits [Tc*N, V].
    split=True: the forward of an update whose backward is the fused split form (s2vt_teacher_forced_fwd_split, with the split
    workspace of (dims, B, N)): by split_fwd_stage() the vocabulary logits (stage 1) and LSTM2's hoisted input partials (stage 2)
    run as split-bf16 products where the shape fits.  Without it every product is the bit-exact fp32 chain.
    sampler_state = (workspace tensor, rows) of the sample() call of the same step on the same video block:
    LSTM1's trajectory is taken from it instead of being recomputed.
    steps (1..Tc): unroll only the first `steps` decode steps (every later position of the batch is masked); logits
    is then [steps*N, V].  caption stays [N, Tc].
    live: int32 device tensor of the unrolled rows (time-major index t*N + n, ascending) whose logits are wanted: logits is
    [len(live), V], the vocabulary projection of every other row is skipped."""
    _chk_f32(video)
    assert caption.is_cuda and caption.dtype == torch.int32 and caption.is_contiguous() and caption.shape[0] == N
    assert caption.shape[1] == dims.n_caption_lstm_step
    B = video.shape[0]
    steps = dims.n_caption_lstm_step if steps is None else int(steps)
    if ws is None:
        ws = train_workspace(dims, B, N, video.device)
    R = steps * N
    if live is not None:
        assert live.is_cuda and live.dtype == torch.int32 and live.is_contiguous() and live.dim() == 1
        R = live.numel()
    if logits is None:
        logits = torch.empty((R, dims.n_words), dtype=torch.float32, device=video.device)
    assert logits.shape[0] == R
    sws, srows = sampler_state if sampler_state is not None else (None, 0)
    if split:
        gws = split_grad_workspace(dims, B, N, video.device)
        check(lib().s2vt_teacher_forced_fwd_split(C.byref(dims), C.byref(params), _ptr(video), B, N, _ptr(caption), steps,
                                                  _ptr(live), 0 if live is None else live.numel(), float(keep), seed,
                                                  _ptr(video_id), _ptr(sample_id), _ptr(logits), _ptr(ws), ws.numel(), _ptr(sws),
                                                  0 if sws is None else sws.numel(), srows, _ptr(gws), gws.numel(), _stream()),
              "s2vt_teacher_forced_fwd_split")
        return logits, ws
    check(lib().s2vt_teacher_forced_fwd_live(C.byref(dims), C.byref(params), _ptr(video), B, N, _ptr(caption), steps,
                                             _ptr(live), 0 if live is None else live.numel(), float(keep), seed,
                                              _ptr(video_id), _ptr(sample_id), _ptr(logits), _ptr(ws), ws.numel(), _ptr(sws),
                                              0 if sws is None else sws.numel(), srows, _stream()),
          "s2vt_teacher_forced_fwd")
    return logits, ws


def scheduled_fwd(dims: Dims, params: Params, video, caption, N: int, p_gt: float, coin_seed: int, loss_weight=1.0, keep=1.0, seed=0,
                  video_id=None, sample_id=None, ws=None, mask_sum=None, mask_sum_copy=None):
    """The scheduled-sampling unroll of generate_words_tf_s2vt.py:101-211 (s2vt_scheduled_fwd): the training forward decodes, and at step
    t >= 1 each row is fed caption[:, t-1] with probability p_gt (the coin: a pure function of coin_seed, video id, sample id and step) and its
    own argmax otherwise.  caption: int32 device tensor [N, Tc] (ids outside [0, n_words) are clamped by the kernel); video_id / sample_id
    [N] int32 are required.  Returns a dict: logits [Tc*N, V] time-major, generated / fed [N, Tc] int32, mask [N, Tc], coef_tm [Tc*N]
    (= loss_weight * mask), target_tm [Tc*N] int32, mask_sum [1], ws -- the training workspace, left as teacher_forced_fwd leaves it for
    the fed words, so bptt_bwd runs on it."""
    _chk_f32(video, mask_sum, mask_sum_copy)
    assert video.is_contiguous()
    assert caption.is_cuda and caption.dtype == torch.int32 and caption.is_contiguous()
    Tc = dims.n_caption_lstm_step
    assert tuple(caption.shape) == (N, Tc)
    for t in (video_id, sample_id):
        assert t is not None and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == N, "video_id / sample_id: int32 [N]"
    B = video.shape[0]
    dev = video.device
    L = lib()
    if ws is None:
        ws = train_workspace(dims, B, N, dev)
    nb = L.s2vt_scheduled_scratch_bytes(C.byref(dims), N)
    assert nb > 0, "bad dims / N"
    scratch = workspace(nb, dev, "scheduled")
    out = dict(logits=torch.empty((Tc * N, dims.n_words), dtype=torch.float32, device=dev),
               generated=torch.empty((N, Tc), dtype=torch.int32, device=dev), fed=torch.empty((N, Tc), dtype=torch.int32, device=dev),
               mask=torch.empty((N, Tc), dtype=torch.float32, device=dev), coef_tm=torch.empty(Tc * N, dtype=torch.float32, device=dev),
               target_tm=torch.empty(Tc * N, dtype=torch.int32, device=dev),
               mask_sum=torch.empty(1, dtype=torch.float32, device=dev) if mask_sum is None else mask_sum, ws=ws)
    check(L.s2vt_scheduled_fwd(C.byref(dims), C.byref(params), _ptr(video), B, N, _ptr(caption), float(p_gt), int(coin_seed) & (2 ** 64 - 1),
                               float(loss_weight), float(keep), seed, _ptr(video_id), _ptr(sample_id), _ptr(out["logits"]), _ptr(out["generated"]),
                               _ptr(out["fed"]), _ptr(out["mask"]), _ptr(out["coef_tm"]), _ptr(out["target_tm"]), _ptr(out["mask_sum"]),
                               _ptr(mask_sum_copy), _ptr(ws), ws.numel(), _ptr(scratch), scratch.numel(), _stream()), "s2vt_scheduled_fwd")
    return out


def averaged_fwd(dims: Dims, params: Params, video, caption, mask, N: int, loss_weight=1.0, keep=1.0, seed=0, video_id=None, sample_id=None,
                 ws=None, mask_sum=None, mask_sum_copy=None, scratch=None):
    """The averaged-embedding unroll of average_generate_words_tf_s2vt.py:88-165 (s2vt_averaged_fwd): the training forward decodes, and at
    step t >= 1 LSTM2 is fed (Wemb[caption[:, t-1]] + Wemb[argmax of step t-1]) / 2; step 0 feeds <bos> alone.  caption: int32 device tensor
    [N, Tc] (ids outside [0, n_words) are clamped by the kernel); mask: fp32 device tensor [N, Tc], the fed caption_mask; video_id /
    sample_id [N] int32 are required.  Returns a dict: logits [Tc*N, V] time-major, generated [N, Tc] int32, coef_tm [Tc*N]
    (= loss_weight * mask), target_tm [Tc*N] int32, mask_sum [1], ws -- the training workspace -- and scratch, which holds the mean operands
    and the id pairs: averaged_bptt_bwd takes both (bptt_bwd on ws alone would differentiate another graph)."""
    _chk_f32(video, mask, mask_sum, mask_sum_copy)
    assert video.is_contiguous() and mask.is_contiguous()
    assert caption.is_cuda and caption.dtype == torch.int32 and caption.is_contiguous()
    Tc = dims.n_caption_lstm_step
    assert tuple(caption.shape) == (N, Tc) and tuple(mask.shape) == (N, Tc)
    for t in (video_id, sample_id):
        assert t is not None and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == N, "video_id / sample_id: int32 [N]"
    B = video.shape[0]
    dev = video.device
    L = lib()
    if ws is None:
        ws = train_workspace(dims, B, N, dev)
    if scratch is None:
        nb = L.s2vt_averaged_scratch_bytes(C.byref(dims), N)
        assert nb > 0, "bad dims / N"
        scratch = workspace(nb, dev, "averaged")
    out = dict(logits=torch.empty((Tc * N, dims.n_words), dtype=torch.float32, device=dev),
               generated=torch.empty((N, Tc), dtype=torch.int32, device=dev), coef_tm=torch.empty(Tc * N, dtype=torch.float32, device=dev),
               target_tm=torch.empty(Tc * N, dtype=torch.int32, device=dev),
               mask_sum=torch.empty(1, dtype=torch.float32, device=dev) if mask_sum is None else mask_sum, ws=ws, scratch=scratch)
    check(L.s2vt_averaged_fwd(C.byref(dims), C.byref(params), _ptr(video), B, N, _ptr(caption), _ptr(mask), float(loss_weight), float(keep), seed,
                              _ptr(video_id), _ptr(sample_id), _ptr(out["logits"]), _ptr(out["generated"]), _ptr(out["coef_tm"]),
                              _ptr(out["target_tm"]), _ptr(out["mask_sum"]), _ptr(mask_sum_copy), _ptr(ws), ws.numel(), _ptr(scratch),
                              scratch.numel(), _stream()), "s2vt_averaged_fwd")
    return out


def averaged_bptt_bwd(dims: Dims, params: Params, grads: Params, video, N: int, dlogits, ws, scratch, keep=1.0, seed=0, video_id=None,
                      sample_id=None, precision="fp32", products=None):
    """The backward of averaged_fwd (s2vt_averaged_bptt_bwd) on its workspace and scratch; gradients are accumulated into `grads`.
    precision "fp32": the split-bf16 products where split_grad_active(N) and fp32 MFMA below, as bptt_bwd (dlogits None: the planes
    softmax_nll_fwd_bwd_split left); "bf16": bf16 operands.  products="fp32" forces the fp32 MFMA products at every row count."""
    _chk_f32(video, dlogits)
    if precision not in GRAD_PRECISIONS:
        raise ValueError(f"precision must be one of {GRAD_PRECISIONS}, got {precision!r}")
    B = video.shape[0]
    assert dlogits is None or dlogits.shape[0] == dims.n_caption_lstm_step * N
    if products == "fp32":
        mode, gws = 0, None
    elif precision == "bf16":
        mode, gws = 1, bf16_grad_workspace(dims, B, N, video.device)
    else:
        mode, gws = 2, split_grad_workspace(dims, B, N, video.device)
    assert dlogits is not None or mode == 2
    check(lib().s2vt_averaged_bptt_bwd(C.byref(dims), C.byref(params), C.byref(grads), _ptr(video), B, N, _ptr(dlogits), float(keep), seed,
                                       _ptr(video_id), _ptr(sample_id), _ptr(ws), ws.numel(), _ptr(scratch), scratch.numel(), mode, _ptr(gws),
                                       0 if gws is None else gws.numel(), _stream()), "s2vt_averaged_bptt_bwd")


def topk_feed_fwd(dims: Dims, params: Params, video, caption, mask, N: int, k=5, loss_weight=1.0, keep=1.0, seed=0, video_id=None,
                  sample_id=None, ws=None, mask_sum=None, mask_sum_copy=None, scratch=None):
    """The top-k score-weighted unroll of sum_generate_words_tf_s2vt.py:101-219 (s2vt_topk_feed_fwd): the training forward decodes, and at
    step t >= 1 LSTM2 is fed sum_j w_j Wemb[id_j] over the top-k logits of step t-1, w = those logits over their sum; step 0 feeds <bos>.
    Arguments as averaged_fwd, plus k (1..8).  Returns a dict: logits [Tc*N, V] time-major, generated [N, Tc] int32, coef_tm [Tc*N]
    (= loss_weight * mask), target_tm [Tc*N] int32, mask_sum [1], k, ws -- the training workspace -- and scratch, which holds the operands
    X, the ids, the weights and the raw sums (topk_feed_scratch_views): topk_feed_bptt_bwd takes both."""
    _chk_f32(video, mask, mask_sum, mask_sum_copy)
    assert video.is_contiguous() and mask.is_contiguous()
    assert caption.is_cuda and caption.dtype == torch.int32 and caption.is_contiguous()
    Tc = dims.n_caption_lstm_step
    assert tuple(caption.shape) == (N, Tc) and tuple(mask.shape) == (N, Tc)
    for t in (video_id, sample_id):
        assert t is not None and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == N, "video_id / sample_id: int32 [N]"
    B = video.shape[0]
    dev = video.device
    L = lib()
    if ws is None:
        ws = train_workspace(dims, B, N, dev)
    if scratch is None:
        nb = L.s2vt_topk_feed_scratch_bytes(C.byref(dims), N, int(k))
        assert nb > 0, "bad dims / N / k"
        scratch = workspace(nb, dev, "topk_feed")
    out = dict(logits=torch.empty((Tc * N, dims.n_words), dtype=torch.float32, device=dev),
               generated=torch.empty((N, Tc), dtype=torch.int32, device=dev), coef_tm=torch.empty(Tc * N, dtype=torch.float32, device=dev),
               target_tm=torch.empty(Tc * N, dtype=torch.int32, device=dev),
               mask_sum=torch.empty(1, dtype=torch.float32, device=dev) if mask_sum is None else mask_sum, k=int(k), ws=ws, scratch=scratch)
    check(L.s2vt_topk_feed_fwd(C.byref(dims), C.byref(params), _ptr(video), B, N, _ptr(caption), _ptr(mask), float(loss_weight), float(keep), seed,
                               _ptr(video_id), _ptr(sample_id), int(k), _ptr(out["logits"]), _ptr(out["generated"]), _ptr(out["coef_tm"]),
                               _ptr(out["target_tm"]), _ptr(out["mask_sum"]), _ptr(mask_sum_copy), _ptr(ws), ws.numel(), _ptr(scratch),
                               scratch.numel(), _stream()), "s2vt_topk_feed_fwd")
    return out


def topk_feed_scratch_views(dims: Dims, N: int, k: int, scratch):
    """Views into topk_feed_fwd's scratch (uint8 tensor), time-major: X [Tc, N, E] fp32, ids [Tc, N, k] int32, w [Tc, N, k] fp32, S [Tc, N]
    fp32 -- block t is what step t was fed.  The layout is include/s2vt.h's: 256-byte granules, the packed picks and the pick launches'
    sample ids in front."""
    Tc, E = dims.n_caption_lstm_step, dims.word_dim
    R = Tc * N
    g = lambda nbytes: (nbytes + 255) // 256 * 256
    off = g(R * 16 * 8) + g(N * 4)
    out = {}
    for name, n, dt, shape in (("X", R * E, torch.float32, (Tc, N, E)), ("ids", R * k, torch.int32, (Tc, N, k)),
                               ("w", R * k, torch.float32, (Tc, N, k)), ("S", R, torch.float32, (Tc, N))):
        out[name] = scratch[off:off + n * 4].view(dt).view(shape)
        off += g(n * 4)
    assert off <= scratch.numel()
    return out


def topk_feed_bptt_bwd(dims: Dims, params: Params, grads: Params, video, N: int, dlogits, ws, scratch, k=5, keep=1.0, seed=0, video_id=None,
                       sample_id=None):
    """The backward of topk_feed_fwd (s2vt_topk_feed_bptt_bwd) on its workspace and scratch; gradients are accumulated into `grads`.
    dlogits [Tc*N, V] is read AND written: it comes in as the softmax part (what softmax_nll_fwd_bwd leaves) and holds the completed
    gradient with respect to the logits on return -- the mix's weights are differentiated.  fp32 products only."""
    _chk_f32(video, dlogits)
    assert dlogits.is_contiguous() and tuple(dlogits.shape) == (dims.n_caption_lstm_step * N, dims.n_words)
    check(lib().s2vt_topk_feed_bptt_bwd(C.byref(dims), C.byref(params), C.byref(grads), _ptr(video), video.shape[0], N, _ptr(dlogits), float(keep),
                                        seed, _ptr(video_id), _ptr(sample_id), int(k), _ptr(ws), ws.numel(), _ptr(scratch), scratch.numel(),
                                        _stream()), "s2vt_topk_feed_bptt_bwd")


def topk_feed_decode(dims: Dims, params: Params, video, k=5, weights_mode=1, unshifted_softmax=True, return_logits=False, ws=None):
    """build_generator of sum_generate_words_tf_s2vt.py:221-275 for the B videos of `video` (s2vt_topk_feed_decode): greedy decoding with
    a soft feed.  weights_mode 1 with unshifted_softmax (the defaults) is the script's generator -- top-k, weights and mix from the
    unshifted softmax's probabilities, the emitted word argmax(probs); weights_mode 0 mixes from the raw logits, the training rule.
    Returns ids [B, Tc] int32, or (ids, logits [Tc*B, V] time-major) with return_logits."""
    _chk_f32(video)
    assert video.is_contiguous()
    B, dev = video.shape[0], video.device
    L = lib()
    if ws is None:
        nb = L.s2vt_topk_feed_decode_workspace_bytes(C.byref(dims), B, int(k))
        assert nb > 0, "bad dims / B / k"
        ws = workspace(nb, dev, "topk_feed_decode")
    ids = torch.empty((B, dims.n_caption_lstm_step), dtype=torch.int32, device=dev)
    logits = torch.empty((dims.n_caption_lstm_step * B, dims.n_words), dtype=torch.float32, device=dev) if return_logits else None
    check(L.s2vt_topk_feed_decode(C.byref(dims), C.byref(params), _ptr(video), B, int(k), int(weights_mode), int(bool(unshifted_softmax)),
                                  _ptr(ids), _ptr(logits), _ptr(ws), ws.numel(), _stream()), "s2vt_topk_feed_decode")
    return (ids, logits) if return_logits else ids


def topk_mix_fwd(scores, Wemb, k, weights_mode=0):
    """The top-k mix alone (s2vt_topk_mix_fwd) on the rows of `scores` [R, V] (a row-strided view is fine): weights_mode 0 reads them as
    logits, 1 as a caller-made plane (the unshifted softmax's probabilities in the generator) -- the rule is the same, the entry's
    argument differs.  Returns ids [R, k] int32, w [R, k], S [R], x [R, E]."""
    _chk_f32(scores, Wemb)
    assert scores.dim() == 2 and scores.stride(1) == 1 and Wemb.is_contiguous()
    R, V = scores.shape
    E = Wemb.shape[1]
    dev = scores.device
    ids = torch.empty((R, k), dtype=torch.int32, device=dev)
    w = torch.empty((R, k), dtype=torch.float32, device=dev)
    S = torch.empty(R, dtype=torch.float32, device=dev)
    x = torch.empty((R, E), dtype=torch.float32, device=dev)
    a = (None, 0, _ptr(scores), scores.stride(0)) if weights_mode else (_ptr(scores), scores.stride(0), None, 0)
    check(lib().s2vt_topk_mix_fwd(a[0], a[1], a[2], a[3], int(weights_mode), R, V, int(k), _ptr(Wemb), E, _ptr(ids), _ptr(w), _ptr(S), _ptr(x), E,
                                  _stream()), "s2vt_topk_mix_fwd")
    return ids, w, S, x


def topk_mix_bwd(dx, ids, w, S, Wemb, dscores, Wout=None, dO=None):
    """The mix's backward (s2vt_topk_mix_bwd), in place: dscores[r, ids[r, j]] += (ds_j - g) / S[r] and, with Wout [H, V] and dO [R, H],
    dO[r] += sum_j that * Wout[:, ids[r, j]].  dx [R, E], dscores [R, V] and dO may be row-strided views."""
    _chk_f32(dx, w, S, Wemb, dscores, Wout, dO)
    R, k = ids.shape
    assert ids.dtype == torch.int32 and ids.is_contiguous() and w.is_contiguous() and S.is_contiguous() and Wemb.is_contiguous()
    assert dx.stride(1) == 1 and dscores.stride(1) == 1 and (dO is None) == (Wout is None)
    assert dO is None or (dO.stride(1) == 1 and Wout.is_contiguous())
    check(lib().s2vt_topk_mix_bwd(_ptr(dx), dx.stride(0), _ptr(ids), _ptr(w), _ptr(S), _ptr(Wemb), Wemb.shape[1], _ptr(Wout), dscores.shape[1],
                                  0 if dO is None else dO.shape[1], k, R, _ptr(dscores), dscores.stride(0), _ptr(dO),
                                  0 if dO is None else dO.stride(0), _stream()), "s2vt_topk_mix_bwd")


def softmax_nll_fwd_bwd(logits, target, coef, smoothing=0.0):
    """In place: logits <- coef * (softmax - q).  Returns (nll [R], lp_target [R]).  smoothing: a float, or a CUDA fp32
    tensor [R] with one label-smoothing value per row."""
    _chk_f32(logits, coef)
    R, V = logits.shape
    assert target.dtype == torch.int32 and target.is_cuda and target.numel() == R and coef.numel() == R
    nll = torch.empty(R, dtype=torch.float32, device=logits.device)
    lp = torch.empty_like(nll)
    if isinstance(smoothing, torch.Tensor):
        _chk_f32(smoothing)
        assert smoothing.numel() == R and smoothing.is_contiguous()
        check(lib().s2vt_softmax_nll_fwd_bwd_rows(_ptr(logits), logits.stride(0), R, V, _ptr(target), _ptr(coef), _ptr(smoothing),
                                                  _ptr(nll), _ptr(lp), _stream()), "s2vt_softmax_nll_fwd_bwd_rows")
        return nll, lp
    check(lib().s2vt_softmax_nll_fwd_bwd(_ptr(logits), logits.stride(0), R, V, _ptr(target), _ptr(coef), float(smoothing),
                                         _ptr(nll), _ptr(lp), _stream()), "s2vt_softmax_nll_fwd_bwd")
    return nll, lp


def split_grad_active(N: int) -> bool:
    """Whether the fp32-mode backward at N unrolled rows runs the fused split form (s2vt_split_grad_active): then
    softmax_nll_fwd_bwd_split can hand it dlogits as planes."""
    return bool(lib().s2vt_split_grad_active(int(N)))


def split_fwd_stage() -> int:
    """The stage of teacher_forced_fwd(split=True) (s2vt_split_fwd_stage: the env S2VT_SPLIT_FWD, read once by the library):
    0 the fp32 forward, 1 the vocabulary logits on split-bf16, 2 LSTM2's hoisted input partials too."""
    return int(lib().s2vt_split_fwd_stage())


def split_fwd_active(N: int) -> int:
    """The stage teacher_forced_fwd(split=True) runs at N unrolled rows (s2vt_split_fwd_active): 0 where the split mode is off."""
    return int(lib().s2vt_split_fwd_active(int(N)))


def softmax_nll_fwd_bwd_split(logits, target, coef, smoothing, dims: Dims, B: int, N: int):
    """softmax_nll_fwd_bwd for an update whose backward is the fused split form (split_grad_active(N)): the same nll / lp, but
    dlogits goes as split-bf16 planes into the split-gradient workspace of (dims, B, N), where bptt_bwd(..., dlogits=None) reads
    it, and `logits` stays as it was.  Returns (nll, lp, in_planes); in_planes False: the shape is not the fused kernel's and
    `logits` now holds the fp32 dlogits, as after softmax_nll_fwd_bwd."""
    _chk_f32(logits, coef)
    R, V = logits.shape
    assert target.dtype == torch.int32 and target.is_cuda and target.numel() == R and coef.numel() == R
    nll = torch.empty(R, dtype=torch.float32, device=logits.device)
    lp = torch.empty_like(nll)
    rows = None
    if isinstance(smoothing, torch.Tensor):
        _chk_f32(smoothing)
        assert smoothing.numel() == R and smoothing.is_contiguous()
        rows, smoothing = smoothing, 0.0
    sws = split_grad_workspace(dims, B, N, logits.device)
    rc = lib().s2vt_softmax_nll_fwd_bwd_split(_ptr(logits), logits.stride(0), R, V, _ptr(target), _ptr(coef), float(smoothing), _ptr(rows),
                                              _ptr(nll), _ptr(lp), C.byref(dims), B, N, _ptr(sws), sws.numel(), _stream())
    if rc != 1:
        check(rc, "s2vt_softmax_nll_fwd_bwd_split")
    return nll, lp, rc == 0


def train_workspace_dz2(dims: Dims, B: int, N: int, ws):
    """View [T, N, 4H] of LSTM2's pre-activation gradients in the training workspace `ws` after LSTM2's phase of bptt_bwd."""
    off, n = C.c_size_t(), C.c_size_t()
    check(lib().s2vt_train_workspace_dz2(C.byref(dims), B, N, C.byref(off), C.byref(n)), "s2vt_train_workspace_dz2")
    return ws[off.value:off.value + 4 * n.value].view(torch.float32).view(-1, N, 4 * dims.lstm_dim)


def split_grad_dlogits_planes(dims: Dims, B: int, N: int, R: int, device):
    """Views (hi, lo), bf16 [R, bf16_pad(V)], of the dlogits planes softmax_nll_fwd_bwd_split left in the split workspace."""
    hi_off, lo_off, ld = C.c_size_t(), C.c_size_t(), C.c_int32()
    check(lib().s2vt_split_grad_dlogits_planes(C.byref(dims), B, N, C.byref(hi_off), C.byref(lo_off), C.byref(ld)), "s2vt_split_grad_dlogits_planes")
    sws = split_grad_workspace(dims, B, N, device)
    n = R * ld.value * 2
    return tuple(sws[o.value:o.value + n].view(torch.bfloat16).view(R, ld.value) for o in (hi_off, lo_off))


def softmax_unshifted_argmax(logits, want_probs=False):
    """tf_s2vt.py:208-209 as written: argmax(exp(l) / sum(exp(l))) in fp32 without a max shift (ids int32 [R], probs)."""
    _chk_f32(logits)
    R, V = logits.shape
    ids = torch.empty(R, dtype=torch.int32, device=logits.device)
    probs = torch.empty((R, V), dtype=torch.float32, device=logits.device) if want_probs else None
    check(lib().s2vt_softmax_unshifted_argmax(_ptr(logits), logits.stride(0), R, V, _ptr(ids), _ptr(probs), _stream()),
          "s2vt_softmax_unshifted_argmax")
    return ids, probs


GRAD_PRECISIONS = ("fp32", "bf16")


def bf16_grad_workspace(dims: Dims, B: int, N: int, device):
    """The scratch of the bf16 backward (s2vt_bf16_grad_workspace_bytes), cached beside the train workspace."""
    nbytes = lib().s2vt_bf16_grad_workspace_bytes(C.byref(dims), B, N)
    assert nbytes > 0, "bad dims / B / N (N must be a multiple of B)"
    return workspace(nbytes, device, "bf16_grad")


def split_grad_workspace(dims: Dims, B: int, N: int, device):
    """The scratch of the split-bf16 backward (s2vt_split_grad_workspace_bytes), cached beside the train workspace."""
    nbytes = lib().s2vt_split_grad_workspace_bytes(C.byref(dims), B, N)
    assert nbytes > 0, "bad dims / B / N (N must be a multiple of B)"
    return workspace(nbytes, device, "split_grad")


def bptt_bwd(dims: Dims, params: Params, grads: Params, video, N: int, dlogits, ws, keep=1.0, seed=0, video_id=None,
             sample_id=None, phase=0, steps=None, live=None, precision="fp32"):
    """phase 0 = the whole backward; 1 = vocab projection only; 2 = the rest (data-parallel overlap).
    steps: what the forward call (teacher_forced_fwd) was given.
    precision "bf16": the gradient contractions on bf16 operands with fp32 accumulation (s2vt_bptt_bwd_bf16, non-parity:
    only the gradients change).
    dlogits None (fp32 precision): softmax_nll_fwd_bwd_split has left it as planes in the split workspace, where the vocabulary phase
    (phase 0 or 1) reads it; the later phases do not use dlogits."""
    _chk_f32(video, dlogits)
    if precision not in GRAD_PRECISIONS:
        raise ValueError(f"precision must be one of {GRAD_PRECISIONS}, got {precision!r}")
    steps = dims.n_caption_lstm_step if steps is None else int(steps)
    assert dlogits is None or dlogits.shape[0] == (steps * N if live is None else live.numel())
    assert dlogits is not None or precision == "fp32"
    if precision == "bf16":
        bws = bf16_grad_workspace(dims, video.shape[0], N, video.device)
        check(lib().s2vt_bptt_bwd_bf16(C.byref(dims), C.byref(params), C.byref(grads), _ptr(video), video.shape[0], N, _ptr(dlogits),
                                       steps, _ptr(live), 0 if live is None else live.numel(), float(keep), seed, _ptr(video_id),
                                       _ptr(sample_id), _ptr(ws), ws.numel(), phase, _ptr(bws), bws.numel(), _stream()),
              "s2vt_bptt_bwd_bf16")
        return
    # fp32: the split-bf16 products (s2vt_bptt_bwd_split; its fp32-MFMA body at <= 256 rows)
    sws = split_grad_workspace(dims, video.shape[0], N, video.device)
    check(lib().s2vt_bptt_bwd_split(C.byref(dims), C.byref(params), C.byref(grads), _ptr(video), video.shape[0], N, _ptr(dlogits),
                                    steps, _ptr(live), 0 if live is None else live.numel(), float(keep), seed, _ptr(video_id),
                                    _ptr(sample_id), _ptr(ws), ws.numel(), phase, _ptr(sws), sws.numel(), _stream()),
          "s2vt_bptt_bwd_split")


def cast_bf16(src, rowidx=None, transpose=False, pad_rows=None, colsum=None, row_copy=False):
    """s2vt_cast_bf16 on an fp32 [R, C] tensor (rows optionally gathered through the int32 `rowidx`, R = len(rowidx)).
    transpose False: bf16 [R, Kp] (Kp = C rounded up to 64, zeros past C).  True: bf16 [C, Rp] (Rp = pad_rows, default R rounded
    up to 64, zeros past R), plus (row_copy) the row form, and colsum[c] += the fp32 column sums of the rows.  Returns the bf16
    tensor, or (transposed, rows) with row_copy."""
    _chk_f32(src, colsum)
    assert src.dim() == 2 and src.stride(1) == 1
    if rowidx is not None:
        assert rowidx.is_cuda and rowidx.dtype == torch.int32 and rowidx.is_contiguous()
    R = src.shape[0] if rowidx is None else rowidx.numel()
    Cc = src.shape[1]
    Kp = (Cc + 63) // 64 * 64
    dev = src.device
    if not transpose:
        out = torch.empty((R, Kp), dtype=torch.bfloat16, device=dev)
        check(lib().s2vt_cast_bf16(_ptr(src), src.stride(0), _ptr(rowidx), R, Cc, 0, _ptr(out), Kp, 0, None, None, 0, None, 0, _stream()),
              "s2vt_cast_bf16")
        return out
    Rp = (R + 63) // 64 * 64 if pad_rows is None else int(pad_rows)
    out = torch.empty((Cc, Rp), dtype=torch.bfloat16, device=dev)
    rows = torch.empty((R, Kp), dtype=torch.bfloat16, device=dev) if row_copy else None
    scratch = workspace(4 * ((Rp + 255) // 256) * Cc, dev, "cast_bf16") if colsum is not None else None
    check(lib().s2vt_cast_bf16(_ptr(src), src.stride(0), _ptr(rowidx), R, Cc, 1, _ptr(out), Rp, Rp, _ptr(colsum), _ptr(rows), Kp,
                               _ptr(scratch), 0 if scratch is None else scratch.numel(), _stream()), "s2vt_cast_bf16")
    return (out, rows) if row_copy else out


def gemm_bf16x3_tn(Ah, Al, Bh, Bl, M=None, N=None, out=None, accumulate=False, split_k=True, bias=None):
    """C[M, N] (+)= sum_k A[k, m] B[k, n] as Ah^T Bh + Ah^T Bl + Al^T Bh on split-bf16 planes stored by rows, [K, lda] and [K, ldb]
    (s2vt_gemm_bf16x3_tn; M, N default to the planes' widths).  bias [N]: += the product's row M -- column M of Ah must hold ones."""
    for t in (Ah, Al, Bh, Bl):
        assert t.is_cuda and t.dtype == torch.bfloat16 and t.stride(1) == 1
    assert Ah.shape == Al.shape and Bh.shape == Bl.shape and Ah.stride(0) == Al.stride(0) and Bh.stride(0) == Bl.stride(0)
    K = Ah.shape[0]
    assert Bh.shape[0] == K
    M = Ah.shape[1] if M is None else int(M)
    N = Bh.shape[1] if N is None else int(N)
    if out is None:
        assert not accumulate
        out = torch.empty((M, N), dtype=torch.float32, device=Ah.device)
    _chk_f32(out, bias)
    assert out.shape[0] == M and out.shape[1] == N and out.stride(1) == 1
    scratch = workspace(32 * (M + 1) * N, Ah.device, "gemm_bf16x3") if split_k and M * N else None
    check(lib().s2vt_gemm_bf16x3_tn(_ptr(Ah), _ptr(Al), Ah.stride(0), _ptr(Bh), _ptr(Bl), Bh.stride(0), _ptr(out), out.stride(0), M, N, K,
                                    int(bool(accumulate)), _ptr(bias), _ptr(scratch), 0 if scratch is None else scratch.numel(), _stream()),
          "s2vt_gemm_bf16x3_tn")
    return out


def gemm_bf16x3_nn(Ah, Al, Bh, Bl, N=None, K=None, out=None, accumulate=False, split_k=True, bias=None):
    """C[M, N] (+)= sum_k A[m, k] B[k, n] as Ah Bh + Ah Bl + Al Bh on split-bf16 planes: A by rows [M, >= bf16_pad(K)], B K-major
    [K, ldb] (s2vt_gemm_bf16x3_nn; N defaults to B's width, K to its rows).  bias [N] fp32 (not with accumulate): added once per column."""
    for t in (Ah, Al, Bh, Bl):
        assert t.is_cuda and t.dtype == torch.bfloat16 and t.stride(1) == 1
    assert Ah.shape == Al.shape and Bh.shape == Bl.shape and Ah.stride(0) == Al.stride(0) and Bh.stride(0) == Bl.stride(0)
    M = Ah.shape[0]
    K = Bh.shape[0] if K is None else int(K)
    N = Bh.shape[1] if N is None else int(N)
    if out is None:
        assert not accumulate
        out = torch.empty((M, N), dtype=torch.float32, device=Ah.device)
    _chk_f32(out, bias)
    assert out.shape[0] == M and out.shape[1] == N and out.stride(1) == 1
    scratch = workspace(32 * M * N, Ah.device, "gemm_bf16x3") if split_k and M * N else None
    check(lib().s2vt_gemm_bf16x3_nn(_ptr(Ah), _ptr(Al), Ah.stride(0), _ptr(Bh), _ptr(Bl), Bh.stride(0), _ptr(out), out.stride(0), M, N, K,
                                    int(bool(accumulate)), _ptr(bias), _ptr(scratch), 0 if scratch is None else scratch.numel(), _stream()),
          "s2vt_gemm_bf16x3_nn")
    return out


def cast_bf16_split(src, rowidx=None, transpose=False, pad_rows=None, colsum=None, row_copy=False):
    """cast_bf16 in split form (s2vt_cast_bf16_split): returns (hi, lo), or ((hi, lo), (row_hi, row_lo)) with row_copy."""
    _chk_f32(src, colsum)
    assert src.dim() == 2 and src.stride(1) == 1
    if rowidx is not None:
        assert rowidx.is_cuda and rowidx.dtype == torch.int32 and rowidx.is_contiguous()
    R = src.shape[0] if rowidx is None else rowidx.numel()
    Cc = src.shape[1]
    Kp = (Cc + 63) // 64 * 64
    dev = src.device
    if not transpose:
        hi = torch.empty((R, Kp), dtype=torch.bfloat16, device=dev)
        lo = torch.empty_like(hi)
        check(lib().s2vt_cast_bf16_split(_ptr(src), src.stride(0), _ptr(rowidx), R, Cc, 0, _ptr(hi), _ptr(lo), Kp, 0, None, None, None, 0,
                                         None, 0, _stream()), "s2vt_cast_bf16_split")
        return hi, lo
    Rp = (R + 63) // 64 * 64 if pad_rows is None else int(pad_rows)
    hi = torch.empty((Cc, Rp), dtype=torch.bfloat16, device=dev)
    lo = torch.empty_like(hi)
    rh = torch.empty((R, Kp), dtype=torch.bfloat16, device=dev) if row_copy else None
    rl = torch.empty((R, Kp), dtype=torch.bfloat16, device=dev) if row_copy else None
    scratch = workspace(4 * ((Rp + 255) // 256) * Cc, dev, "cast_bf16") if colsum is not None else None
    check(lib().s2vt_cast_bf16_split(_ptr(src), src.stride(0), _ptr(rowidx), R, Cc, 1, _ptr(hi), _ptr(lo), Rp, Rp, _ptr(colsum), _ptr(rh),
                                     _ptr(rl), Kp, _ptr(scratch), 0 if scratch is None else scratch.numel(), _stream()), "s2vt_cast_bf16_split")
    return ((hi, lo), (rh, rl)) if row_copy else (hi, lo)


def gemm_bf16x3_nt(Ah, Al, Bh, Bl, out=None, accumulate=False, split_k=True):
    """C[M, N] (+)= Ah Bh^T + Ah Bl^T + Al Bh^T on split-bf16 operands [M | N, Kp] (Kp % 64 == 0), fp32 accumulation
    (s2vt_gemm_bf16x3_nt).  split_k: give it the scratch that lets it split the reduction where its tiles do not fill the chip."""
    for t in (Ah, Al, Bh, Bl):
        assert t.is_cuda and t.dtype == torch.bfloat16 and t.stride(1) == 1
    assert Ah.shape == Al.shape and Bh.shape == Bl.shape and Ah.stride(0) == Al.stride(0) and Bh.stride(0) == Bl.stride(0)
    M, Kp = Ah.shape
    N = Bh.shape[0]
    if out is None:
        assert not accumulate
        out = torch.empty((M, N), dtype=torch.float32, device=Ah.device)
    _chk_f32(out)
    assert out.shape[0] == M and out.shape[1] == N and out.stride(1) == 1
    scratch = workspace(32 * M * N, Ah.device, "gemm_bf16x3") if split_k and M * N else None
    check(lib().s2vt_gemm_bf16x3_nt(_ptr(Ah), _ptr(Al), Ah.stride(0), _ptr(Bh), _ptr(Bl), Bh.stride(0), _ptr(out), out.stride(0), M, N, Kp,
                                    int(bool(accumulate)), _ptr(scratch), 0 if scratch is None else scratch.numel(), _stream()),
          "s2vt_gemm_bf16x3_nt")
    return out


def gemm_bf16x3_nt_tile(Ah, Al, Bh, Bl, tile, out=None, accumulate=False):
    """gemm_bf16x3_nt without split-K on the workgroup tile `tile`: 0 = 128 x 128, 1 = 192 x 96 (s2vt_gemm_bf16x3_nt_tile) -- the same bits."""
    for t in (Ah, Al, Bh, Bl):
        assert t.is_cuda and t.dtype == torch.bfloat16 and t.stride(1) == 1
    assert Ah.shape == Al.shape and Bh.shape == Bl.shape and Ah.stride(0) == Al.stride(0) and Bh.stride(0) == Bl.stride(0)
    M, Kp = Ah.shape
    N = Bh.shape[0]
    if out is None:
        assert not accumulate
        out = torch.empty((M, N), dtype=torch.float32, device=Ah.device)
    _chk_f32(out)
    assert out.shape[0] == M and out.shape[1] == N and out.stride(1) == 1
    check(lib().s2vt_gemm_bf16x3_nt_tile(_ptr(Ah), _ptr(Al), Ah.stride(0), _ptr(Bh), _ptr(Bl), Bh.stride(0), _ptr(out), out.stride(0), M, N, Kp,
                                         int(bool(accumulate)), _stream(), int(tile)), "s2vt_gemm_bf16x3_nt_tile")
    return out


def gemm_bf16x1_nt(Ah, Bh, out=None, accumulate=False):
    """C[M, N] (+)= Ah Bh^T on the bf16 hi planes alone [M | N, Kp] (Kp % 64 == 0), fp32 accumulation (s2vt_gemm_bf16x1_nt): the sampler's
    one-product pick screen -- within 2^-7 of sum |a_k b_k|, no more."""
    for t in (Ah, Bh):
        assert t.is_cuda and t.dtype == torch.bfloat16 and t.stride(1) == 1
    M, Kp = Ah.shape
    N = Bh.shape[0]
    if out is None:
        assert not accumulate
        out = torch.empty((M, N), dtype=torch.float32, device=Ah.device)
    _chk_f32(out)
    assert out.shape[0] == M and out.shape[1] == N and out.stride(1) == 1
    check(lib().s2vt_gemm_bf16x1_nt(_ptr(Ah), Ah.stride(0), _ptr(Bh), Bh.stride(0), _ptr(out), out.stride(0), M, N, Kp, int(bool(accumulate)),
                                    _stream()), "s2vt_gemm_bf16x1_nt")
    return out


def gemm_bf16x3_nt_tile_choice(M, N, cus):
    """The tile the library's rule takes for an M x N NT split-bf16 product on `cus` compute units: 0 = 128 x 128, 1 = 192 x 96 (host only)."""
    r = lib().s2vt_gemm_bf16x3_nt_tile_choice(int(M), int(N), int(cus))
    if r < 0:
        check(r, "s2vt_gemm_bf16x3_nt_tile_choice")
    return r


def gemm_bf16_nt(A, B, out=None, accumulate=False, mfma=0, n=None):
    """C[M, N] (+)= A[M, Kp] B[N, Kp]^T on bf16 operands (Kp % 64 == 0), fp32 accumulation (s2vt_gemm_bf16_nt).  `out` may be a
    row-strided fp32 view; n: columns of C when B has more rows than are wanted."""
    assert A.is_cuda and B.is_cuda and A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16
    assert A.stride(1) == 1 and B.stride(1) == 1 and A.shape[1] == B.shape[1]
    M, Kp = A.shape
    N = B.shape[0] if n is None else int(n)
    if out is None:
        assert not accumulate
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    _chk_f32(out)
    assert out.shape[0] == M and out.shape[1] == N and out.stride(1) == 1
    check(lib().s2vt_gemm_bf16_nt(_ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(out), out.stride(0), M, N, Kp, int(bool(accumulate)),
                                  int(mfma), _stream()), "s2vt_gemm_bf16_nt")
    return out


def bptt_dvideo(dims: Dims, params: Params, B: int, N: int, ws):
    """Gradient w.r.t. the frame features [B, Tv, dim_image] after bptt_bwd on `ws` (end-to-end CNN fine-tuning)."""
    import torch
    out = torch.empty(B, dims.n_video_lstm_step, dims.dim_image, device=ws.device, dtype=torch.float32)
    check(lib().s2vt_bptt_dvideo(C.byref(dims), C.byref(params), B, N, _ptr(out), _ptr(ws), ws.numel(), _stream()), "s2vt_bptt_dvideo")
    return out


def caption_mask(ids, mask_sum=None, want_mask=True, want_target=True, mask_sum_copy=None):
    """ids [N, Tc] int32 -> (mask [N, Tc] fp32 | None, target_tm [Tc*N] int32 | None, mask_sum [1] fp32): one launch.
    mask_sum_copy: a second place that receives sum(mask) (the gradient bucket's tail slot)."""
    assert ids.is_cuda and ids.dtype == torch.int32 and ids.is_contiguous()
    N, Tc = ids.shape
    mask = torch.empty((N, Tc), dtype=torch.float32, device=ids.device) if want_mask else None
    tgt = torch.empty(N * Tc, dtype=torch.int32, device=ids.device) if want_target else None
    if mask_sum is None:
        mask_sum = torch.empty(1, dtype=torch.float32, device=ids.device)
    check(lib().s2vt_caption_mask(_ptr(ids), N, Tc, _ptr(mask), _ptr(tgt), _ptr(mask_sum), _ptr(mask_sum_copy), _stream()), "s2vt_caption_mask")
    return mask, tgt, mask_sum


def pg_coef(mask, rewards, baseline, scale=1.0):
    _chk_f32(mask, rewards, baseline)
    N, Tc = mask.shape
    coef = torch.empty(N * Tc, dtype=torch.float32, device=mask.device)
    check(lib().s2vt_pg_coef(_ptr(mask), _ptr(rewards), _ptr(baseline), float(scale), N, Tc, _ptr(coef), _stream()), "s2vt_pg_coef")
    return coef


def rouge_l_score(tokens, ref_offsets, video_refs, n_refs, ids, video_of_row, beta2, eos_id=0, want_pr=False, out=None, pr_out=None):
    """ROUGE-L of ids [N, Tc] (int32, unit stride along Tc, any row stride >= Tc) against the references of video_of_row [N] (int32):
    float32 [N], one launch (s2vt_rouge_l_score).  tokens / ref_offsets [n_refs + 1] / video_refs [n_videos + 1]: the corpus as int32
    device tensors, references sorted by video.  want_pr: also the [N, 2] float64 (p, r)."""
    for t in (tokens, ref_offsets, video_refs, ids, video_of_row):
        assert t.is_cuda and t.dtype == torch.int32, "expected a CUDA int32 tensor"
    assert tokens.is_contiguous() and ref_offsets.is_contiguous() and video_refs.is_contiguous() and video_of_row.is_contiguous()
    assert ids.dim() == 2 and (ids.shape[1] == 1 or ids.stride(1) == 1) and ref_offsets.numel() == n_refs + 1
    N, Tc = ids.shape
    assert video_of_row.numel() == N
    ld = int(ids.stride(0)) if N > 1 else max(int(ids.stride(0)), Tc)
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=ids.device)
    if want_pr and pr_out is None:
        pr_out = torch.empty((N, 2), dtype=torch.float64, device=ids.device)
    if N == 0:
        return (out, pr_out) if want_pr else out
    refs =_lib.RougeRefs(tokens.data_ptr(), ref_offsets.data_ptr(), video_refs.data_ptr(), video_refs.numel() - 1, int(n_refs))
    check(lib().s2vt_rouge_l_score(C.byref(refs), _ptr(ids), ld, N, Tc, int(eos_id), _ptr(video_of_row), float(beta2), _ptr(out), _ptr(pr_out),
                                   _stream()), "s2vt_rouge_l_score")
    return (out, pr_out) if want_pr else out


def xe_prep(mask, caption, loss_weight, n_global, q1):
    """(coef_tm [Tc*N], target_tm [Tc*N] int32, sum(mask) [1]) of the XE update in one launch (s2vt_xe_prep)."""
    _chk_f32(mask)
    N, Tc = mask.shape
    assert caption.is_cuda and caption.dtype == torch.int32 and caption.is_contiguous() and tuple(caption.shape) == (N, Tc)
    coef = torch.empty(N * Tc, dtype=torch.float32, device=mask.device)
    target = torch.empty(N * Tc, dtype=torch.int32, device=mask.device)
    msum = torch.empty(1, dtype=torch.float32, device=mask.device)
    check(lib().s2vt_xe_prep(_ptr(mask), _ptr(caption), N, Tc, float(loss_weight), float(n_global), int(bool(q1)), _ptr(coef), _ptr(target),
                             _ptr(msum), _stream()), "s2vt_xe_prep")
    return coef, target, msum


def mixed_prep(mask, gt_mask, rewards, baseline, sampled, gt_caption, lambda_loss, loss_weight, q1, smoothing, n_global_b):
    """The mixed objective's coefficients (s2vt_mixed_prep): (coef_tm [Tc*N], smooth_tm [Tc*N], caption_all [N, Tc] int32, target_tm [Tc*N] int32, sums [2])."""
    _chk_f32(mask, gt_mask, rewards, baseline)
    Ns, Tc = mask.shape
    B = gt_mask.shape[0]
    N = Ns + B
    for c_, n_ in ((sampled, Ns), (gt_caption, B)):
        assert c_.is_cuda and c_.dtype == torch.int32 and c_.is_contiguous() and tuple(c_.shape) == (n_, Tc)
    dev = mask.device
    coef = torch.empty(N * Tc, dtype=torch.float32, device=dev)
    smooth = torch.empty(N * Tc, dtype=torch.float32, device=dev)
    cap_all = torch.empty((N, Tc), dtype=torch.int32, device=dev)
    target = torch.empty(N * Tc, dtype=torch.int32, device=dev)
    sums = torch.empty(2, dtype=torch.float32, device=dev)
    check(lib().s2vt_mixed_prep(_ptr(mask), _ptr(gt_mask), _ptr(rewards), _ptr(baseline), _ptr(sampled), _ptr(gt_caption), Ns, B, Tc,
                                float(lambda_loss), float(loss_weight), int(bool(q1)), float(smoothing), float(n_global_b), _ptr(coef),
                                _ptr(smooth), _ptr(cap_all), _ptr(target), _ptr(sums), _stream()), "s2vt_mixed_prep")
    return coef, smooth, cap_all, target, sums


def mixed_loss(coef, nll, live, N, Ns):
    """[sum over the sampled rows, sum over the ground-truth rows, both] of coef * nll (s2vt_mixed_loss)."""
    _chk_f32(coef, nll)
    out = torch.empty(3, dtype=torch.float32, device=coef.device)
    check(lib().s2vt_mixed_loss(_ptr(coef), _ptr(nll), _ptr(live), coef.numel(), N, Ns, _ptr(out), _stream()), "s2vt_mixed_loss")
    return out


def step_scalars(coef, nll, msum_local, gsum_global, loss=None, gscale=None, sumsq=None):
    _chk_f32(coef, nll, msum_local, gsum_global, loss, gscale, sumsq)
    R = 0 if coef is None else coef.numel()
    check(lib().s2vt_step_scalars(_ptr(coef), _ptr(nll), R, _ptr(msum_local), _ptr(gsum_global), _ptr(loss), _ptr(gscale), _ptr(sumsq), _stream()),
          "s2vt_step_scalars")


def grad_finalize(g, theta, gscale, weight_decay, sumsq):
    _chk_f32(g, theta, gscale, sumsq)
    check(lib().s2vt_grad_finalize(_ptr(g), _ptr(theta), g.numel(), _ptr(gscale), float(weight_decay), _ptr(sumsq), _stream()),
          "s2vt_grad_finalize")


def adam_tf(theta, g, m, v, sumsq, clip_norm, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, applied_step=None):
    """applied_step: optional CUDA int32 tensor [1] that receives `step` when the update is applied (it is skipped on the
    device while a persistent-recurrence fault is pending, see chain_fault())."""
    _chk_f32(theta, g, m, v, sumsq)
    if applied_step is not None:
        assert applied_step.is_cuda and applied_step.dtype == torch.int32
    check(lib().s2vt_adam_tf_guarded(_ptr(theta), _ptr(g), _ptr(m), _ptr(v), theta.numel(), _ptr(sumsq), float(clip_norm), float(lr),
                                     int(step), beta1, beta2, eps, _ptr(applied_step), _stream()), "s2vt_adam_tf")


def sgd(theta, g, sumsq, clip_norm, lr, step, applied_step=None):
    """theta -= lr * g * clip_norm / max(sqrt(sumsq), clip_norm) (s2vt_sgd_guarded): tf.train.GradientDescentOptimizer behind
    tf.clip_by_global_norm.  applied_step: as adam_tf."""
    _chk_f32(theta, g, sumsq)
    if applied_step is not None:
        assert applied_step.is_cuda and applied_step.dtype == torch.int32
    check(lib().s2vt_sgd_guarded(_ptr(theta), _ptr(g), theta.numel(), _ptr(sumsq), float(clip_norm), float(lr), int(step), _ptr(applied_step),
                                 _stream()), "s2vt_sgd")


def chain_fault() -> bool:
    """True while a persistent-recurrence timeout is pending (a host-memory read: no synchronisation)."""
    return bool(lib().s2vt_chain_fault())


def chain_ack(disable_persistent: bool = True):
    """Synchronise the device, clear the fault; disable_persistent: per-step launches for the rest of the process."""
    check(lib().s2vt_chain_ack(1 if disable_persistent else 0), "s2vt_chain_ack")


class chain_hold:
    """Context manager: recurrences launched inside take their per-step form (s2vt_chain_hold) -- for the stretch of a step
    during which another stream's kernels (an asynchronous all-reduce) share the GPU with the library's stream."""

    def __enter__(self):
        check(lib().s2vt_chain_hold(1), "s2vt_chain_hold")
        return self

    def __exit__(self, *exc):
        check(lib().s2vt_chain_hold(0), "s2vt_chain_hold")
        return False


def prof_enable(on: bool):
    check(lib().s2vt_prof_enable(1 if on else 0), "s2vt_prof_enable")


def prof_filter(kernel_class: int = -1, tile_cfg: int = -1):
    check(lib().s2vt_prof_filter(kernel_class, tile_cfg), "s2vt_prof_filter")


def prof_collect():
    """Rows of the launch profiler (call after torch.cuda.synchronize())."""
    rows = (_lib.ProfRow * 64)()
    n = lib().s2vt_prof_collect(rows, 64)
    if n < 0:
        check(n, "s2vt_prof_collect")
    return [dict(kernel_class=r.kernel_class, tile_cfg=r.tile_cfg, launches=r.launches, total_ms=r.total_ms,
                 total_flops=r.total_flops, name=r.name.decode()) for r in rows[:n]]


def attention_fwd(hWa, P, Vt, w):
    """One attention step.  hWa [B,H], P/Vt [Tv,B,H], w [H] -> (scores [Tv,B], alpha [Tv,B], ctx [B,H])."""
    _chk_f32(hWa, P, Vt, w)
    Tv, B, H = P.shape
    sc = torch.empty((Tv, B), dtype=torch.float32, device=P.device)
    al = torch.empty_like(sc)
    ctx = torch.empty((B, H), dtype=torch.float32, device=P.device)
    check(lib().s2vt_attention_fwd(_ptr(hWa), _ptr(P), _ptr(Vt), _ptr(w), _ptr(sc), _ptr(al), _ptr(ctx), Tv, B, H, _stream()),
          "s2vt_attention_fwd")
    return sc, al, ctx


def attention_bwd(hWa, P, Vt, w, alpha, dctx, dw):
    """Returns (dhWa, dP, dVt); accumulates into dw [H]."""
    _chk_f32(hWa, P, Vt, w, alpha, dctx, dw)
    Tv, B, H = P.shape
    de = torch.empty((Tv, B), dtype=torch.float32, device=P.device)
    dh = torch.empty_like(hWa); dP = torch.empty_like(P); dV = torch.empty_like(Vt)
    check(lib().s2vt_attention_bwd(_ptr(hWa), _ptr(P), _ptr(Vt), _ptr(w), _ptr(alpha), _ptr(dctx), _ptr(de), _ptr(dh), _ptr(dP),
                                   _ptr(dV), _ptr(dw), Tv, B, H, _stream()), "s2vt_attention_bwd")
    return dh, dP, dV


# ---------------------------------------------------------------------------------------------
# the temporal-attention captioner as a whole model (csrc/attn_model.hip)
# ---------------------------------------------------------------------------------------------
def make_attn_params(tensors: dict) -> AttnParams:
    """tensors: name -> CUDA fp32 tensor for every name of _lib.ATTN_PARAM_FIELDS."""
    p = AttnParams()
    for n in _lib.ATTN_PARAM_FIELDS:
        t = tensors[n]
        _chk_f32(t)
        assert t.is_contiguous()
        setattr(p, n, t.data_ptr())
    p._keep = tensors
    return p


def attn_workspace(dims: Dims, B: int, device):
    nbytes = lib().s2vt_attn_workspace_bytes(C.byref(dims), B)
    assert nbytes > 0, "bad dims / B (n_video_lstm_step <= 64)"
    return workspace(nbytes, device, "attn")


def attn_teacher_forced_fwd(dims: Dims, params: AttnParams, video, caption, keep=1.0, seed=0, video_id=None, sample_id=None, steps=None,
                            ws=None, logits=None, want_alphas=False):
    """build_model's unroll (original_attention.py:88-143).  Returns (time-major logits [steps*B, V], alphas [steps,Tv,B] | None, ws)."""
    _chk_f32(video)
    B = video.shape[0]
    assert video.is_contiguous() and caption.is_cuda and caption.dtype == torch.int32 and caption.is_contiguous()
    assert caption.shape == (B, dims.n_caption_lstm_step)
    steps = dims.n_caption_lstm_step if steps is None else int(steps)
    if ws is None:
        ws = attn_workspace(dims, B, video.device)
    if logits is None:
        logits = torch.empty((steps * B, dims.n_words), dtype=torch.float32, device=video.device)
    al = torch.empty((steps, dims.n_video_lstm_step, B), dtype=torch.float32, device=video.device) if want_alphas else None
    check(lib().s2vt_attn_teacher_forced_fwd(C.byref(dims), C.byref(params), _ptr(video), B, _ptr(caption), steps, float(keep), seed,
                                             _ptr(video_id), _ptr(sample_id), _ptr(logits), _ptr(al), _ptr(ws), ws.numel(), _stream()),
          "s2vt_attn_teacher_forced_fwd")
    return logits, al, ws


def attn_loss_inputs(caption, mask, beta=0.0, want_reg=False):
    """caption [B,Tc] int32, mask [B,Tc] fp32 (device) -> (target_tm [Tc*B] int32, coef_tm [Tc*B], reg_tm | None, mask_sum [1]): one launch."""
    _chk_f32(mask)
    assert caption.is_cuda and caption.dtype == torch.int32 and caption.is_contiguous() and mask.is_contiguous() and mask.shape == caption.shape
    B, Tc = caption.shape
    dev = caption.device
    tgt = torch.empty(B * Tc, dtype=torch.int32, device=dev)
    coef = torch.empty(B * Tc, dtype=torch.float32, device=dev)
    reg = torch.empty(B * Tc, dtype=torch.float32, device=dev) if want_reg else None
    msum = torch.empty(1, dtype=torch.float32, device=dev)
    check(lib().s2vt_attn_loss_inputs(_ptr(caption), _ptr(mask), B, Tc, float(beta), _ptr(tgt), _ptr(coef), _ptr(reg), _ptr(msum), _stream()),
          "s2vt_attn_loss_inputs")
    return tgt, coef, reg, msum


def attn_step_scalars(dims: Dims, B: int, ws, coef, nll, reg_coef, reg_m, msum_local, gsum_global, loss, gscale, sumsq):
    _chk_f32(coef, nll, reg_coef, msum_local, gsum_global, loss, gscale, sumsq)
    check(lib().s2vt_attn_step_scalars(_ptr(coef), _ptr(nll), coef.numel(), _ptr(reg_coef), float(reg_m), _ptr(msum_local), _ptr(gsum_global),
                                       _ptr(loss), _ptr(gscale), _ptr(sumsq), C.byref(dims), B, _ptr(ws), ws.numel(), _stream()),
          "s2vt_attn_step_scalars")


def attn_bptt_bwd(dims: Dims, params: AttnParams, grads: AttnParams, video, dlogits, ws, steps=None, reg_coef=None, reg_m=0.5, keep=1.0,
                  seed=0, video_id=None, sample_id=None):
    _chk_f32(video, dlogits, reg_coef)
    B = video.shape[0]
    steps = dims.n_caption_lstm_step if steps is None else int(steps)
    assert dlogits.shape[0] == steps * B and (reg_coef is None or reg_coef.numel() == steps * B)
    check(lib().s2vt_attn_bptt_bwd(C.byref(dims), C.byref(params), C.byref(grads), _ptr(video), B, _ptr(dlogits), steps, _ptr(reg_coef),
                                   float(reg_m), float(keep), seed, _ptr(video_id), _ptr(sample_id), _ptr(ws), ws.numel(), _stream()),
          "s2vt_attn_bptt_bwd")


def attn_decode_greedy(dims: Dims, params: AttnParams, video, video_base=0, want_alphas=False, ws=None):
    """build_generator / build_sampler (original_attention.py:155-251): (ids [B,Tc] int32, alphas [Tc,Tv,B] | None)."""
    _chk_f32(video)
    assert video.is_contiguous()
    B = video.shape[0]
    if ws is None:
        ws = attn_workspace(dims, B, video.device)
    ids = torch.empty((B, dims.n_caption_lstm_step), dtype=torch.int32, device=video.device)
    al = torch.empty((dims.n_caption_lstm_step, dims.n_video_lstm_step, B), dtype=torch.float32, device=video.device) if want_alphas else None
    check(lib().s2vt_attn_decode_greedy(C.byref(dims), C.byref(params), _ptr(video), B, int(video_base), _ptr(ids), _ptr(al), _ptr(ws),
                                        ws.numel(), _stream()), "s2vt_attn_decode_greedy")
    return ids, al


# ---- rows that share image blocks (self-critical REINFORCE on the attention captioner): N = n_video * samples, sample-major
def attention_fwd_rows(hWa, P, Vt, w):
    """s2vt_attention_fwd for hWa [N,H] over P/Vt [Tv,n_video,H], N = samples * n_video (row s*n_video + j reads block j)
    -> (scores [Tv,N], alpha [Tv,N], ctx [N,H])."""
    _chk_f32(hWa, P, Vt, w)
    Tv, nv, H = P.shape
    N = hWa.shape[0]
    assert N % nv == 0
    sc = torch.empty((Tv, N), dtype=torch.float32, device=P.device)
    al = torch.empty_like(sc)
    ctx = torch.empty((N, H), dtype=torch.float32, device=P.device)
    rv = torch.empty(N, dtype=torch.int32, device=P.device)
    check(lib().s2vt_attention_fwd_rows(_ptr(hWa), _ptr(P), _ptr(Vt), _ptr(w), _ptr(sc), _ptr(al), _ptr(ctx), _ptr(rv), Tv, nv, N // nv, H,
                                        _stream()), "s2vt_attention_fwd_rows")
    return sc, al, ctx


def attention_bwd_rows(hWa, P, Vt, w, alpha, dctx, dw, dP=None, dVt=None):
    """Returns (dhWa [N,H], dP, dVt [Tv,n_video,H] summed over each video's rows); accumulates into dw [H], and into dP / dVt when given."""
    _chk_f32(hWa, P, Vt, w, alpha, dctx, dw, dP, dVt)
    Tv, nv, H = P.shape
    N = hWa.shape[0]
    assert N % nv == 0 and (dP is None) == (dVt is None)
    acc = dP is not None
    de = torch.empty(N * Tv, dtype=torch.float32, device=P.device)
    dh = torch.empty_like(hWa)
    if not acc:
        dP = torch.empty_like(P); dVt = torch.empty_like(Vt)
    check(lib().s2vt_attention_bwd_rows(_ptr(hWa), _ptr(P), _ptr(Vt), _ptr(w), _ptr(alpha), _ptr(dctx), _ptr(de), _ptr(dh), _ptr(dP),
                                        _ptr(dVt), _ptr(dw), Tv, nv, N // nv, H, int(acc), _stream()), "s2vt_attention_bwd_rows")
    return dh, dP, dVt


def attn_sample(dims: Dims, params: AttnParams, video, K: int, seed: int, video_base: int = 0, with_greedy: bool = True, stop_at_eos: bool = False):
    """K multinomial captions per video (+ greedy) from the attention captioner: (sampled [K*B,Tc] | None, greedy [B,Tc] | None) int32.
    stop_at_eos (opt-in, not the reference's behaviour; s2vt_attn_sample_ex): a row leaves the loop once it has picked <eos>; its later
    ids are 0.  Ids up to and including the first <eos> -- the positions the objective's mask keeps -- are unchanged."""
    _chk_f32(video)
    assert video.is_contiguous()
    B = video.shape[0]
    g = 1 if with_greedy else 0
    nbytes = lib().s2vt_attn_sample_workspace_bytes(C.byref(dims), B, K, g)
    assert nbytes > 0, "bad dims / B / K (n_video_lstm_step <= 64, K >= 0, K > 0 or with_greedy)"
    ws = workspace(nbytes, video.device, "attn_sample")
    Tc = dims.n_caption_lstm_step
    ids = torch.empty((K * B, Tc), dtype=torch.int32, device=video.device) if K > 0 else None
    gr = torch.empty((B, Tc), dtype=torch.int32, device=video.device) if g else None
    if stop_at_eos:
        check(lib().s2vt_attn_sample_ex(C.byref(dims), C.byref(params), _ptr(video), B, K, g, seed, int(video_base), 1, _ptr(ids), _ptr(gr),
                                        _ptr(ws), ws.numel(), _stream()), "s2vt_attn_sample_ex")
    else:
        check(lib().s2vt_attn_sample(C.byref(dims), C.byref(params), _ptr(video), B, K, g, seed, int(video_base), _ptr(ids), _ptr(gr), _ptr(ws),
                                     ws.numel(), _stream()), "s2vt_attn_sample")
    return ids, gr


def attn_rows_workspace(dims: Dims, n_video: int, samples: int, device):
    nbytes = lib().s2vt_attn_rows_workspace_bytes(C.byref(dims), n_video, samples)
    assert nbytes > 0, "bad dims / n_video / samples (n_video_lstm_step <= 64)"
    return workspace(nbytes, device, "attn_rows")


def attn_teacher_forced_fwd_rows(dims: Dims, params: AttnParams, video, caption, keep=1.0, seed=0, video_id=None, sample_id=None, steps=None,
                                 ws=None, want_alphas=False):
    """attn_teacher_forced_fwd on N = caption.shape[0] sample-major rows that share the n_video = video.shape[0] image blocks.
    Returns (time-major logits [steps*N, V], alphas [steps,Tv,N] | None, ws)."""
    _chk_f32(video)
    nv, N = video.shape[0], caption.shape[0]
    assert video.is_contiguous() and caption.is_cuda and caption.dtype == torch.int32 and caption.is_contiguous()
    assert N % nv == 0 and caption.shape == (N, dims.n_caption_lstm_step)
    steps = dims.n_caption_lstm_step if steps is None else int(steps)
    if ws is None:
        ws = attn_rows_workspace(dims, nv, N // nv, video.device)
    logits = torch.empty((steps * N, dims.n_words), dtype=torch.float32, device=video.device)
    al = torch.empty((steps, dims.n_video_lstm_step, N), dtype=torch.float32, device=video.device) if want_alphas else None
    check(lib().s2vt_attn_teacher_forced_fwd_rows(C.byref(dims), C.byref(params), _ptr(video), nv, N // nv, _ptr(caption), steps, float(keep), seed,
                                                  _ptr(video_id), _ptr(sample_id), _ptr(logits), _ptr(al), _ptr(ws), ws.numel(), _stream()),
          "s2vt_attn_teacher_forced_fwd_rows")
    return logits, al, ws


def attn_step_scalars_rows(dims: Dims, n_video: int, samples: int, ws, coef, nll, reg_coef, reg_m, msum_local, gsum_global, loss, gscale, sumsq):
    _chk_f32(coef, nll, reg_coef, msum_local, gsum_global, loss, gscale, sumsq)
    check(lib().s2vt_attn_step_scalars_rows(_ptr(coef), _ptr(nll), coef.numel(), _ptr(reg_coef), float(reg_m), _ptr(msum_local), _ptr(gsum_global),
                                            _ptr(loss), _ptr(gscale), _ptr(sumsq), C.byref(dims), n_video, samples, _ptr(ws), ws.numel(), _stream()),
          "s2vt_attn_step_scalars_rows")


def attn_bptt_bwd_rows(dims: Dims, params: AttnParams, grads: AttnParams, video, samples, dlogits, ws, steps=None, reg_coef=None, reg_m=0.5,
                       keep=1.0, seed=0, video_id=None, sample_id=None):
    _chk_f32(video, dlogits, reg_coef)
    nv = video.shape[0]
    N = nv * int(samples)
    steps = dims.n_caption_lstm_step if steps is None else int(steps)
    assert dlogits.shape[0] == steps * N and (reg_coef is None or reg_coef.numel() == steps * N)
    check(lib().s2vt_attn_bptt_bwd_rows(C.byref(dims), C.byref(params), C.byref(grads), _ptr(video), nv, int(samples), _ptr(dlogits), steps,
                                        _ptr(reg_coef), float(reg_m), float(keep), seed, _ptr(video_id), _ptr(sample_id), _ptr(ws), ws.numel(),
                                        _stream()), "s2vt_attn_bptt_bwd_rows")


def attr_head_fwd(video, attr_W, attr_b, labels=None):
    _chk_f32(video, attr_W, attr_b, labels)
    B, Tv, D = video.shape
    A = attr_W.shape[1]
    mean = torch.empty((B, D), dtype=torch.float32, device=video.device)
    z = torch.empty((B, A), dtype=torch.float32, device=video.device)
    bce = torch.empty_like(z) if labels is not None else None
    check(lib().s2vt_attr_head_fwd(_ptr(video), B, Tv, D, _ptr(attr_W), _ptr(attr_b), A, _ptr(labels), _ptr(mean), _ptr(z),
                                   _ptr(bce), _stream()), "s2vt_attr_head_fwd")
    return mean, z, bce


def attr_head_scores(video, attr_W, attr_b):
    """evaluate_multilabel (reinforce_multitask_e2e_attribute_loss.py:606-626): (z, sigmoid(z)) [B, A]."""
    _chk_f32(video, attr_W, attr_b)
    B, Tv, D = video.shape
    A = attr_W.shape[1]
    mean = torch.empty((B, D), dtype=torch.float32, device=video.device)
    z = torch.empty((B, A), dtype=torch.float32, device=video.device)
    scores = torch.empty_like(z)
    check(lib().s2vt_attr_head_scores(_ptr(video), B, Tv, D, _ptr(attr_W), _ptr(attr_b), A, _ptr(mean), _ptr(z), _ptr(scores), _stream()),
          "s2vt_attr_head_scores")
    return z, scores


def attr_head_bwd(mean, z, labels, scale, d_attr_W, d_attr_b):
    _chk_f32(mean, z, labels, d_attr_W, d_attr_b)
    B, D = mean.shape
    A = z.shape[1]
    dz = torch.empty_like(z)
    check(lib().s2vt_attr_head_bwd(_ptr(mean), _ptr(z), _ptr(labels), B, D, A, float(scale), _ptr(dz), _ptr(d_attr_W),
                                   _ptr(d_attr_b), _stream()), "s2vt_attr_head_bwd")
    return dz


# ---------------------------------------------------------------------------------------------
# session API + single-op entry points (include/s2vt.h, last section)
# ---------------------------------------------------------------------------------------------
class Session:
    """s2vt_create / s2vt_destroy: a handle that owns its sampler workspace.  encode once, then any
    number of greedy / multinomial decodes on that encode."""

    def __init__(self, dims: Dims, max_B: int, max_K: int):
        self.dims = dims
        self._h = C.c_void_p()
        check(lib().s2vt_create(C.byref(dims), max_B, max_K, C.byref(self._h)), "s2vt_create")
        self._B = 0

    def close(self):
        if self._h:
            check(lib().s2vt_destroy(self._h), "s2vt_destroy")
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode(self, params: Params, video):
        _chk_f32(video)
        assert video.is_contiguous()
        self._B = video.shape[0]
        check(lib().s2vt_encode_fwd(self._h, C.byref(params), _ptr(video), self._B, _stream()), "s2vt_encode_fwd")

    def decode_greedy(self, params: Params):
        ids = torch.empty((self._B, self.dims.n_caption_lstm_step), dtype=torch.int32, device="cuda")
        check(lib().s2vt_decode_greedy(self._h, C.byref(params), _ptr(ids), _stream()), "s2vt_decode_greedy")
        return ids

    def decode_multinomial(self, params: Params, K: int, seed: int, video_base: int = 0):
        ids = torch.empty((K * self._B, self.dims.n_caption_lstm_step), dtype=torch.int32, device="cuda")
        check(lib().s2vt_decode_multinomial(self._h, C.byref(params), K, seed, video_base, _ptr(ids), _stream()),
              "s2vt_decode_multinomial")
        return ids


def vocab_topk(logits, k: int):
    """s2vt_vocab_topk: (ids int32 [R, k], logp fp32 [R, k]) -- the k largest logits per row (value descending, index
    ascending on ties) and their log-softmax values, bit-identical to softmax_nll_fwd_bwd's lp for that target.  `logits` may be
    a row-strided view (stride(1) == 1)."""
    _chk_f32(logits)
    assert logits.dim() == 2 and logits.stride(1) == 1
    R, V = logits.shape
    ids = torch.empty((R, k), dtype=torch.int32, device=logits.device)
    logp = torch.empty((R, k), dtype=torch.float32, device=logits.device)
    check(lib().s2vt_vocab_topk(_ptr(logits), logits.stride(0), R, V, int(k), _ptr(ids), _ptr(logp), _stream()), "s2vt_vocab_topk")
    return ids, logp


class BeamDecoder:
    """s2vt_beam_workspace_bytes / s2vt_beam_encode / s2vt_beam_step: a handle that owns the workspace of a batched beam search over
    up to max_B videos with up to `beam` hypotheses each.  encode once per batch, then one step() per decode step: one
    host-to-device copy of the row lists, one device-to-host copy of the top-k words and log-probabilities."""

    def __init__(self, dims: Dims, max_B: int, beam: int, device="cuda"):
        self.dims, self.max_B, self.beam, self.device = dims, int(max_B), int(beam), torch.device(device)
        nbytes = lib().s2vt_beam_workspace_bytes(C.byref(dims), self.max_B, self.beam)
        if not nbytes:
            raise ValueError(f"beam decoder: bad shape (B={max_B}, beam={beam}; 1 <= beam <= 16)")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        assert self.ws.data_ptr() % 256 == 0
        self._B = 0

    def encode(self, params: Params, video):
        _chk_f32(video)
        assert video.is_contiguous() and video.shape[0] <= self.max_B
        self._B = video.shape[0]
        check(lib().s2vt_beam_encode(C.byref(self.dims), C.byref(params), _ptr(video), self._B, self.beam, _ptr(self.ws), self.ws.numel(),
                                     _stream()), "s2vt_beam_encode")

    def step(self, params: Params, t: int, rows, k: int, want_logits=False):
        """rows: int32 [3, R] host array (video of each row, parent row of step t - 1, word).  Returns numpy (ids [R, k],
        logp [R, k]) and, with want_logits, the step's logits [R, V] on the device."""
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        R = rows.shape[1]
        dev = torch.from_numpy(rows).to(self.device)                            # the one host-to-device copy
        out = torch.empty((2, R, k), dtype=torch.int32, device=self.device)    # ids, then the bits of logp
        logits = torch.empty((R, self.dims.n_words), dtype=torch.float32, device=self.device) if want_logits else None
        check(lib().s2vt_beam_step(C.byref(self.dims), C.byref(params), self._B, self.beam, int(t), R, _ptr(dev[0]), _ptr(dev[1]),
                                   _ptr(dev[2]), int(k), _ptr(out[0]), _ptr(out[1]), _ptr(logits), _ptr(self.ws), self.ws.numel(),
                                   _stream()), "s2vt_beam_step")
        host = out.cpu().numpy()                                                # the one device-to-host copy
        ids, logp = host[0], host[1].view(np.float32)
        return (ids, logp, logits) if want_logits else (ids, logp)


class BidirBeamDecoder:
    """s2vt_bidir_beam_workspace_bytes / s2vt_bidir_beam_encode / s2vt_bidir_beam_step: BeamDecoder for the bidirectional captioner (same
    interface; params: make_bidir_params).  encode runs what a video's hypotheses share -- both LSTM1 directions, their products into
    LSTM2, LSTM2's encode steps -- once per batch; a step is one gathered-state cell launch, the vocabulary product and the top-k.  Steps
    are issued in order t = 0, 1, ...; at t = 0 the parent row is ignored and the word row holds <bos>."""

    def __init__(self, dims: Dims, max_B: int, beam: int, device="cuda", lstm1_form=-1):
        self.dims, self.max_B, self.beam, self.device, self.lstm1_form = dims, int(max_B), int(beam), torch.device(device), int(lstm1_form)
        nbytes = lib().s2vt_bidir_beam_workspace_bytes(C.byref(dims), self.max_B, self.beam)
        if not nbytes:
            raise ValueError(f"bidirectional beam decoder: bad shape (B={max_B}, beam={beam}; 1 <= beam <= 16, n_caption_lstm_step <= 128)")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        assert self.ws.data_ptr() % 256 == 0
        self._B = 0

    def encode(self, params, video):
        _chk_f32(video)
        assert video.is_contiguous() and video.shape[0] <= self.max_B
        self._B = video.shape[0]
        check(lib().s2vt_bidir_beam_encode(C.byref(self.dims), C.byref(params), _ptr(video), self._B, self.beam, self.lstm1_form, _ptr(self.ws),
                                           self.ws.numel(), _stream()), "s2vt_bidir_beam_encode")

    def step(self, params, t: int, rows, k: int, want_logits=False):
        """rows: int32 [3, R] host array (video of each row, parent row of step t - 1, word).  Returns numpy (ids [R, k],
        logp [R, k]) and, with want_logits, the step's logits [R, V] on the device."""
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        R = rows.shape[1]
        dev = torch.from_numpy(rows).to(self.device)                            # the one host-to-device copy
        out = torch.empty((2, R, k), dtype=torch.int32, device=self.device)    # ids, then the bits of logp
        logits = torch.empty((R, self.dims.n_words), dtype=torch.float32, device=self.device) if want_logits else None
        check(lib().s2vt_bidir_beam_step(C.byref(self.dims), C.byref(params), self._B, self.beam, int(t), R, _ptr(dev[0]), _ptr(dev[1]),
                                         _ptr(dev[2]), int(k), _ptr(out[0]), _ptr(out[1]), _ptr(logits), _ptr(self.ws), self.ws.numel(),
                                         _stream()), "s2vt_bidir_beam_step")
        host = out.cpu().numpy()                                                # the one device-to-host copy
        ids, logp = host[0], host[1].view(np.float32)
        return (ids, logp, logits) if want_logits else (ids, logp)


class AttnBeamDecoder:
    """s2vt_attn_beam_workspace_bytes / s2vt_attn_beam_encode / s2vt_attn_beam_step: BeamDecoder for the temporal-attention captioner
    (same interface).  encode embeds the frames and hoists the image part once per batch; a step's hypotheses read their video's
    block in place.  Steps are issued in order t = 0, 1, ...; at t = 0 the parent and word rows are ignored (zero state, no <bos>)."""

    def __init__(self, dims: Dims, max_B: int, beam: int, device="cuda"):
        self.dims, self.max_B, self.beam, self.device = dims, int(max_B), int(beam), torch.device(device)
        nbytes = lib().s2vt_attn_beam_workspace_bytes(C.byref(dims), self.max_B, self.beam)
        if not nbytes:
            raise ValueError(f"attention beam decoder: bad shape (B={max_B}, beam={beam}; 1 <= beam <= 16, n_video_lstm_step <= 64)")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        assert self.ws.data_ptr() % 256 == 0
        self._B = 0

    def encode(self, params: AttnParams, video):
        _chk_f32(video)
        assert video.is_contiguous() and video.shape[0] <= self.max_B
        self._B = video.shape[0]
        check(lib().s2vt_attn_beam_encode(C.byref(self.dims), C.byref(params), _ptr(video), self._B, self.beam, _ptr(self.ws), self.ws.numel(),
                                          _stream()), "s2vt_attn_beam_encode")

    def step(self, params: AttnParams, t: int, rows, k: int, want_logits=False, want_alphas=False):
        """rows: int32 [3, R] host array (video of each row, parent row of step t - 1, word).  Returns numpy (ids [R, k],
        logp [R, k]), then -- when asked for -- the step's logits [R, V] and alphas [Tv, R] on the device."""
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        R = rows.shape[1]
        dev = torch.from_numpy(rows).to(self.device)                            # the one host-to-device copy
        out = torch.empty((2, R, k), dtype=torch.int32, device=self.device)    # ids, then the bits of logp
        logits = torch.empty((R, self.dims.n_words), dtype=torch.float32, device=self.device) if want_logits else None
        alphas = torch.empty((self.dims.n_video_lstm_step, R), dtype=torch.float32, device=self.device) if want_alphas else None
        check(lib().s2vt_attn_beam_step(C.byref(self.dims), C.byref(params), self._B, self.beam, int(t), R, _ptr(dev[0]), _ptr(dev[1]),
                                        _ptr(dev[2]), int(k), _ptr(out[0]), _ptr(out[1]), _ptr(logits), _ptr(alphas), _ptr(self.ws),
                                        self.ws.numel(), _stream()), "s2vt_attn_beam_step")
        host = out.cpu().numpy()                                                # the one device-to-host copy
        res = (host[0], host[1].view(np.float32))
        if want_logits:
            res += (logits,)
        if want_alphas:
            res += (alphas,)
        return res


def pack_weights(W_tf, in_dim: int):
    _chk_f32(W_tf)
    H = W_tf.shape[1] // 4
    Wx = torch.empty((in_dim, H, 4), dtype=torch.float32, device=W_tf.device)
    Wh = torch.empty((H, H, 4), dtype=torch.float32, device=W_tf.device)
    check(lib().s2vt_pack_weights(_ptr(W_tf), in_dim, H, _ptr(Wx), _ptr(Wh), _stream()), "s2vt_pack_weights")
    return Wx, Wh


def unpack_weights(Wx, Wh):
    _chk_f32(Wx, Wh)
    in_dim, H = Wx.shape[0], Wh.shape[0]
    W = torch.empty((in_dim + H, 4 * H), dtype=torch.float32, device=Wh.device)
    check(lib().s2vt_unpack_weights(_ptr(Wx), _ptr(Wh), in_dim, H, _ptr(W), _stream()), "s2vt_unpack_weights")
    return W


def frame_embed_bwd(dims: Dims, video, d_emb, dW, db):
    _chk_f32(video, d_emb, dW, db)
    check(lib().s2vt_frame_embed_bwd(C.byref(dims), _ptr(video), _ptr(d_emb), video.shape[0], _ptr(dW), _ptr(db), _stream()),
          "s2vt_frame_embed_bwd")


def lstm_cell_bwd(gates, c_new, c_prev, dh, dc_in=None):
    _chk_f32(gates, c_new, c_prev, dh, dc_in)
    M, H = c_new.shape
    dz = torch.empty((M, 4 * H), dtype=torch.float32, device=dh.device)
    dc_prev = torch.empty_like(c_new)
    check(lib().s2vt_lstm_cell_bwd(_ptr(gates), _ptr(c_new), _ptr(c_prev), _ptr(dh), _ptr(dc_in), _ptr(dz), _ptr(dc_prev), M, H,
                                   _stream()), "s2vt_lstm_cell_bwd")
    return dz, dc_prev


def xent_smooth_fwd_bwd(logits, target, coef, label_smoothing=0.05):
    _chk_f32(logits, coef)
    R, V = logits.shape
    nll = torch.empty(R, dtype=torch.float32, device=logits.device)
    check(lib().s2vt_xent_smooth_fwd_bwd(_ptr(logits), logits.stride(0), R, V, _ptr(target), _ptr(coef), float(label_smoothing),
                                         _ptr(nll), _stream()), "s2vt_xent_smooth_fwd_bwd")
    return nll


def pg_nll_fwd_bwd(logits, target_tm, adv, mask):
    """logits [Tc*N, V] time-major (overwritten with d/dlogits), target_tm int32 [Tc*N], adv [N], mask [N,Tc]."""
    _chk_f32(logits, adv, mask)
    N, Tc = mask.shape
    V = logits.shape[1]
    coef = torch.empty(N * Tc, dtype=torch.float32, device=logits.device)
    nll = torch.empty_like(coef)
    lp = torch.empty_like(coef)
    check(lib().s2vt_pg_nll_fwd_bwd(_ptr(logits), logits.stride(0), N, Tc, V, _ptr(target_tm), _ptr(adv), _ptr(mask), _ptr(coef),
                                    _ptr(nll), _ptr(lp), _stream()), "s2vt_pg_nll_fwd_bwd")
    return nll, lp, coef


def embed_gather(Wemb, idx):
    _chk_f32(Wemb)
    assert idx.dtype == torch.int32 and idx.is_cuda
    out = torch.empty((idx.numel(), Wemb.shape[1]), dtype=torch.float32, device=Wemb.device)
    check(lib().s2vt_embed_gather(_ptr(Wemb), Wemb.stride(0), _ptr(idx), idx.numel(), Wemb.shape[1], _ptr(out), out.stride(0),
                                  _stream()), "s2vt_embed_gather")
    return out


def embed_scatter_add(dE, idx, dWemb):
    """dWemb[idx[r], :] += dE[r, :] (s2vt_embed_scatter_add): dE [R, E] may be a row-strided view, dWemb [V, E] is contiguous."""
    _chk_f32(dE, dWemb)
    assert idx.dtype == torch.int32 and idx.is_cuda and idx.numel() == dE.shape[0]
    assert dE.dim() == 2 and dE.stride(1) == 1 and dWemb.is_contiguous() and dWemb.shape[1] == dE.shape[1]
    check(lib().s2vt_embed_scatter_add(_ptr(dE), dE.stride(0), _ptr(idx), dE.shape[0], dE.shape[1], _ptr(dWemb), _stream()),
          "s2vt_embed_scatter_add")


def embed_scatter_add2(dE, idx_a, idx_b, dWemb, scale=0.5):
    """dWemb[idx_a[r], :] += scale * dE[r, :] and dWemb[idx_b[r], :] += scale * dE[r, :] (s2vt_embed_scatter_add2; both additions land when
    the two ids are equal): dE [R, E] may be a row-strided view, dWemb [V, E] is contiguous."""
    _chk_f32(dE, dWemb)
    for idx in (idx_a, idx_b):
        assert idx.dtype == torch.int32 and idx.is_cuda and idx.is_contiguous() and idx.numel() == dE.shape[0]
    assert dE.dim() == 2 and dE.stride(1) == 1 and dWemb.is_contiguous() and dWemb.shape[1] == dE.shape[1]
    check(lib().s2vt_embed_scatter_add2(_ptr(dE), dE.stride(0), _ptr(idx_a), _ptr(idx_b), float(scale), dE.shape[0], dE.shape[1], _ptr(dWemb),
                                        _stream()), "s2vt_embed_scatter_add2")


def embed_scatter_addk(dE, ids, w, dWemb):
    """dWemb[ids[r, j], :] += w[r, j] * dE[r, :] for every j (s2vt_embed_scatter_addk): dE [R, E] may be a row-strided view, ids int32 and
    w fp32 [R, k] and dWemb [V, E] are contiguous."""
    _chk_f32(dE, w, dWemb)
    assert ids.dtype == torch.int32 and ids.is_cuda and ids.is_contiguous() and w.is_contiguous() and ids.shape == w.shape
    assert dE.dim() == 2 and dE.stride(1) == 1 and dWemb.is_contiguous() and dWemb.shape[1] == dE.shape[1] and ids.shape[0] == dE.shape[0]
    check(lib().s2vt_embed_scatter_addk(_ptr(dE), dE.stride(0), _ptr(ids), _ptr(w), ids.shape[1], dE.shape[0], dE.shape[1], _ptr(dWemb), _stream()),
          "s2vt_embed_scatter_addk")


def global_norm_clip(g, clip_norm: float):
    _chk_f32(g)
    sumsq = torch.empty(1, dtype=torch.float32, device=g.device)
    check(lib().s2vt_global_norm_clip(_ptr(g), g.numel(), float(clip_norm), _ptr(sumsq), _stream()), "s2vt_global_norm_clip")
    return sumsq


def gemm_tn(A, B, C_, accumulate=True, rowidx=None):
    """C_[Kout,N] (+)= A[row(m)]^T @ B over the rows m (weight gradient of X @ W)."""
    _chk_f32(A, B, C_)
    Mred, N = B.shape
    Kout = C_.shape[0]
    check(lib().s2vt_gemm_tn(_ptr(A), A.stride(0), _ptr(rowidx), _ptr(B), B.stride(0), _ptr(C_), C_.stride(0), Mred, Kout, N,
                             1 if accumulate else 0, _stream()), "s2vt_gemm_tn")


def transpose(W):
    _chk_f32(W)
    R, Cc = W.shape
    out = torch.empty((Cc, R), dtype=torch.float32, device=W.device)
    check(lib().s2vt_transpose(_ptr(W), W.stride(0), _ptr(out), R, R, Cc, _stream()), "s2vt_transpose")
    return out


def colsum(X, out):
    _chk_f32(X, out)
    check(lib().s2vt_colsum(_ptr(X), X.stride(0), X.shape[0], X.shape[1], _ptr(out), _stream()), "s2vt_colsum")


def tanh_bwd(y, dy):
    _chk_f32(y, dy)
    dx = torch.empty_like(y)
    check(lib().s2vt_tanh_bwd(_ptr(y), _ptr(dy), _ptr(dx), y.numel(), _stream()), "s2vt_tanh_bwd")
    return dx


def dropout_bwd(dout, keep, seed, drop_code, video_id, sample_id):
    _chk_f32(dout)
    M, H = dout.shape
    dh = torch.empty((M, H), dtype=torch.float32, device=dout.device)
    check(lib().s2vt_dropout_bwd(_ptr(dout), dout.stride(0), _ptr(dh), M, H, float(keep), seed, drop_code, _ptr(video_id),
                                 _ptr(sample_id), _stream()), "s2vt_dropout_bwd")
    return dh
