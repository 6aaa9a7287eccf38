"""The model bit S2VT_MODEL_RESIDUAL (s2vt_dims.reserved) and s2vt_lstm_cell_fwd_res without a GPU: the size queries and the argument
checks that come before any device work, and the Python surface's refusals and checkpoint round trip."""
import ctypes

import numpy as np
import pytest

import s2vt_amd
from s2vt_amd import _lib

BADARG, ALIGN = -1, -2
RES = _lib.MODEL_RESIDUAL
SHAPES = [(16, 11, 3, 4, 2, 3), (1536, 2000, 300, 992, 5, 8), (96, 300, 20, 48, 2, 7), (128, 260, 32, 64, 5, 12)]


def _dims(shape=SHAPES[0], bits=0, label_dim=0):
    return _lib.Dims(*shape, label_dim, bits)


def _params():
    p = _lib.Params()
    for n in _lib.PARAM_FIELDS[:9]:
        setattr(p, n, 256)                                         # (never dereferenced: the checks come first)
    return p


ONE = ctypes.c_void_p(256)
ODD = ctypes.c_void_p(264)                                         # a workspace that fails the alignment check, which comes after the argument checks


def _r256(n):
    return (n + 255) // 256 * 256


def test_the_struct_is_unchanged():
    assert ctypes.sizeof(_lib.Dims) == 32 and _lib.Dims.reserved.offset == 28
    assert RES == 1


@pytest.mark.parametrize("bits", [2, 3, 4, 1 << 16, -1, -2])
def test_unknown_bits_are_refused_everywhere(bits):
    L = s2vt_amd.lib()
    d, p = _dims(bits=bits), _params()
    r = ctypes.byref(d)
    assert L.s2vt_sample_workspace_bytes(r, 4, 2, 1) == 0
    assert L.s2vt_sample_mix_workspace_bytes(r, 4, 1) == 0
    assert L.s2vt_beam_workspace_bytes(r, 4, 3) == 0
    assert L.s2vt_train_workspace_bytes(r, 4, 8) == 0
    assert L.s2vt_bf16_grad_workspace_bytes(r, 4, 8) == 0
    assert L.s2vt_split_grad_workspace_bytes(r, 4, 8) == 0
    assert L.s2vt_scheduled_scratch_bytes(r, 8) == 0
    assert L.s2vt_attn_workspace_bytes(r, 4) == 0
    assert L.s2vt_sample_ex(r, ctypes.byref(p), ONE, 4, 2, 1, 0, 0, 0, ONE, ODD, 1 << 20, None) == BADARG
    assert L.s2vt_beam_encode(r, ctypes.byref(p), ONE, 4, 3, ODD, 1 << 20, None) == BADARG
    assert L.s2vt_frame_embed_fwd(r, ctypes.byref(p), ONE, 4, ONE, None) == BADARG
    assert L.s2vt_teacher_forced_fwd_live(r, ctypes.byref(p), ONE, 4, 8, ONE, 3, None, 0, 1.0, 0, None, None, ONE, ODD, 1 << 20, None, 0, 0, None) == BADARG
    assert L.s2vt_bptt_bwd_live(r, ctypes.byref(p), ctypes.byref(p), ONE, 4, 8, ONE, 3, None, 0, 1.0, 0, None, None, ODD, 1 << 20, 0, None) == BADARG
    assert L.s2vt_bptt_dvideo(r, ctypes.byref(p), 4, 8, ONE, ODD, 1 << 20, None) == BADARG


@pytest.mark.parametrize("bits,want", [(0, ALIGN), (RES, ALIGN)])
def test_entry_points_that_honour_the_bit_pass_their_argument_checks(bits, want):
    """With a misaligned workspace a call whose arguments are accepted reports S2VT_E_ALIGN, before any device work."""
    L = s2vt_amd.lib()
    d, p = _dims(bits=bits), _params()
    r = ctypes.byref(d)
    assert L.s2vt_sample_ex(r, ctypes.byref(p), ONE, 4, 2, 1, 0, 0, 1, ONE, ODD, 1 << 20, None) == want
    assert L.s2vt_sample(r, ctypes.byref(p), ONE, 4, 2, 1, 0, 0, ONE, ODD, 1 << 20, None) == want
    assert L.s2vt_beam_encode(r, ctypes.byref(p), ONE, 4, 3, ODD, 1 << 20, None) == want
    assert L.s2vt_beam_step(r, ctypes.byref(p), 4, 3, 0, 4, ONE, ONE, ONE, 3, ONE, ONE, None, ODD, 1 << 20, None) == want
    assert L.s2vt_teacher_forced_fwd_live(r, ctypes.byref(p), ONE, 4, 8, ONE, 3, None, 0, 1.0, 0, None, None, ONE, ODD, 1 << 20, None, 0, 0, None) == want
    assert L.s2vt_bptt_bwd_live(r, ctypes.byref(p), ctypes.byref(p), ONE, 4, 8, ONE, 3, None, 0, 1.0, 0, None, None, ODD, 1 << 20, 0, None) == want


def test_refusing_entry_points_refuse_the_bit_and_are_unchanged_without_it():
    L = s2vt_amd.lib()
    p = _params()
    plain, res = _dims(), _dims(bits=RES)
    a, b = ctypes.byref(plain), ctypes.byref(res)
    # size functions: 0 with the bit, what they returned before without it
    assert L.s2vt_sample_mix_workspace_bytes(b, 4, 1) == 0 and L.s2vt_sample_mix_workspace_bytes(a, 4, 1) > 0
    assert L.s2vt_scheduled_scratch_bytes(b, 8) == 0 and L.s2vt_scheduled_scratch_bytes(a, 8) > 0
    for fn, args in ((L.s2vt_attn_workspace_bytes, (4,)), (L.s2vt_attn_rows_workspace_bytes, (4, 2)), (L.s2vt_attn_sample_workspace_bytes, (4, 2, 1)),
                     (L.s2vt_attn_beam_workspace_bytes, (4, 3))):
        assert fn(b, *args) == 0 and fn(a, *args) > 0
    # calls: BADARG with the bit; without it the same arguments get as far as the alignment check
    mix = lambda d: L.s2vt_sample_mix(d, ctypes.byref(p), ONE, 4, ONE, 0.5, 1, 0, 0, ONE, ODD, 1 << 20, None)
    assert mix(b) == BADARG and mix(a) == ALIGN
    sched = lambda d: L.s2vt_scheduled_fwd(d, ctypes.byref(p), ONE, 4, 8, ONE, 0.5, 0, 1.0, 1.0, 0, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None, None,
                                           ODD, 1 << 20, ONE, 1 << 20, None)
    assert sched(b) == BADARG and sched(a) == ALIGN
    ap = _lib.AttnParams()
    for n, _ in _lib.AttnParams._fields_:
        setattr(ap, n, 256)
    greedy = lambda d: L.s2vt_attn_decode_greedy(d, ctypes.byref(ap), ONE, 4, 0, ONE, None, ODD, 1 << 20, None)
    assert greedy(b) == BADARG and greedy(a) == ALIGN
    out = ctypes.c_void_p()
    assert L.s2vt_create(b, 4, 2, ctypes.byref(out)) == BADARG and not out.value


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("B", [1, 5, 16, 40, 150])
def test_workspaces_grow_by_the_documented_block_only(shape, B):
    """Sampler: one [R, H] float block; beam: [B beam, H] floats + [B beam] int32; each rounded up to 256 bytes, behind the plain
    regions.  The training workspace and the bf16 / split scratch are the plain model's.  (The bit-clear sizes themselves are pinned by
    tests/test_sampler_workspace_sizes_cpu.py and test_split_grads_cpu.py.)"""
    L = s2vt_amd.lib()
    a, b = ctypes.byref(_dims(shape)), ctypes.byref(_dims(shape, RES))
    H = shape[3]
    for K, g in ((2, 1), (0, 1), (5, 0), (1, 1)):
        R = (K + g) * B
        assert L.s2vt_sample_workspace_bytes(b, B, K, g) == L.s2vt_sample_workspace_bytes(a, B, K, g) + _r256(4 * R * H)
    for beam in (1, 3, 16):
        R = B * beam
        assert L.s2vt_beam_workspace_bytes(b, B, beam) == L.s2vt_beam_workspace_bytes(a, B, beam) + _r256(4 * R * H) + _r256(4 * R)
    for rep in (1, 3):
        for fn in (L.s2vt_train_workspace_bytes, L.s2vt_bf16_grad_workspace_bytes, L.s2vt_split_grad_workspace_bytes):
            assert fn(b, B, rep * B) == fn(a, B, rep * B) > 0
    hi = [ctypes.c_size_t(), ctypes.c_size_t()]; lo = [ctypes.c_size_t(), ctypes.c_size_t()]; ld = [ctypes.c_int32(), ctypes.c_int32()]
    for i, d in enumerate((a, b)):
        assert L.s2vt_split_grad_dlogits_planes(d, B, 3 * B, ctypes.byref(hi[i]), ctypes.byref(lo[i]), ctypes.byref(ld[i])) == 0
    assert (hi[0].value, lo[0].value, ld[0].value) == (hi[1].value, lo[1].value, ld[1].value)


def test_lstm_cell_fwd_res_argument_checks():
    L = s2vt_amd.lib()
    H, M = 8, 4
    good = _lib.Operand(256, None, H, H, 0, 0)
    call = lambda res, out=ONE: L.s2vt_lstm_cell_fwd_res(None, None, ONE, ONE, 0, ONE, ONE, res, ONE, ONE, out, None, M, H, 1.0, 0, None, None, 0, -1, None)
    assert call(None) == BADARG                                                    # res NULL
    assert call(ctypes.byref(_lib.Operand(None, None, H, H, 0, 0))) == BADARG      # res->ptr NULL
    assert call(ctypes.byref(_lib.Operand(256, None, H, H - 1, 0, 0))) == BADARG   # k != H
    assert call(ctypes.byref(_lib.Operand(256, None, H, H + 4, 0, 0))) == BADARG
    assert call(ctypes.byref(_lib.Operand(256, None, H - 1, H, 0, 0))) == BADARG   # ld < H
    assert call(ctypes.byref(_lib.Operand(256, None, H, H, -1, 0))) == BADARG      # rowmod < 0
    assert call(ctypes.byref(good), out=None) == BADARG                            # out NULL
    assert L.s2vt_lstm_cell_fwd_res(None, None, ONE, ONE, 0, ONE, ONE, ctypes.byref(good), ONE, ONE, ONE, None, 0, H, 1.0, 0, None, None, 0, -1, None) == 0   # M = 0: nothing to do


def test_live_row_entries_argument_checks():
    """s2vt_gemm_live, s2vt_lstm_cell_fwd_live, s2vt_vocab_pick_live: the dense entries' refusals, the residual operand's, and a row list
    and a count that are both absent -- all before any device work; M == 0 is nothing to do."""
    L = s2vt_amd.lib()
    H, M, K, N, V = 8, 4, 6, 12, 20
    seg = lambda ptr=256, ld=K, k=K: (_lib.Operand * 1)(_lib.Operand(ptr, None, ld, k, 0, 0))
    gemm = lambda segs=seg(), nseg=1, W=ONE, ldw=N, C=ONE, ldc=N, M=M, live=ONE, n_live=ONE, ldci=N, Cinit=None: L.s2vt_gemm_live(
        segs, nseg, W, ldw, None, Cinit, ldci, C, ldc, M, N, 0, live, n_live, -1, None)
    assert gemm(segs=None) == BADARG and gemm(W=None) == BADARG and gemm(C=None) == BADARG          # NULL operands
    assert gemm(nseg=0) == BADARG and gemm(nseg=4) == BADARG and gemm(M=-1) == BADARG
    assert gemm(live=None, n_live=None) == BADARG                                                   # neither a list nor a count
    assert gemm(segs=seg(ld=K - 1)) == BADARG                                                       # ld < k
    assert gemm(ldw=N - 1) == BADARG and gemm(ldc=N - 1) == BADARG and gemm(Cinit=ONE, ldci=N - 1) == BADARG
    assert gemm(M=0) == 0 and gemm(M=0, live=None) == 0 and gemm(M=0, n_live=None) == 0

    good = _lib.Operand(256, None, H, H, 0, 0)
    x0 = _lib.Operand(256, None, K, K, 0, 0)
    def cell(res=None, out=ONE, h=ONE, c=ONE, W=ONE, b=ONE, cn=ONE, hn=ONE, M=M, live=ONE, n_live=ONE, x=x0, keep=1.0, vid=None):
        return L.s2vt_lstm_cell_fwd_live(ctypes.byref(x), None, h, c, 0, W, b, res, cn, hn, out, None, M, H, keep, 0, vid, vid, 0, live, n_live, -1, None)
    for name in ("h", "c", "W", "b", "cn", "hn"):
        assert cell(**{name: None}) == BADARG, name                                                 # NULL operands
    assert cell(live=None, n_live=None) == BADARG
    assert cell(x=_lib.Operand(256, None, K - 1, K, 0, 0)) == BADARG                                # ld < k
    assert cell(keep=0.5) == BADARG and cell(keep=0.5, vid=ONE, out=None) == BADARG                 # dropout needs the ids and `out`
    assert cell(M=-1) == BADARG
    # the residual operand: optional here, checked as s2vt_lstm_cell_fwd_res checks it when given
    assert cell(ctypes.byref(_lib.Operand(None, None, H, H, 0, 0))) == BADARG                       # res->ptr NULL
    assert cell(ctypes.byref(_lib.Operand(256, None, H, H - 1, 0, 0))) == BADARG                    # k != H
    assert cell(ctypes.byref(_lib.Operand(256, None, H, H + 4, 0, 0))) == BADARG
    assert cell(ctypes.byref(_lib.Operand(256, None, H - 1, H, 0, 0))) == BADARG                    # ld < H
    assert cell(ctypes.byref(_lib.Operand(256, None, H, H, -1, 0))) == BADARG                       # rowmod < 0
    assert cell(ctypes.byref(good), out=None) == BADARG                                             # out NULL
    assert cell(M=0) == 0 and cell(ctypes.byref(good), M=0) == 0 and cell(M=0, live=None) == 0 and cell(M=0, n_live=None) == 0

    def pick(o2=ONE, ld=H, W=ONE, b=ONE, vid=ONE, sid=ONE, packed=ONE, stride=16, M=M, live=ONE, n_live=ONE, H=H, V=V):
        return L.s2vt_vocab_pick_live(o2, ld, W, b, M, H, V, vid, sid, 0, 0, packed, stride, None, live, n_live, -1, None)
    for name in ("o2", "W", "b", "vid", "sid", "packed"):
        assert pick(**{name: None}) == BADARG, name                                                 # NULL operands
    assert pick(live=None, n_live=None) == BADARG
    assert pick(ld=H - 1) == BADARG and pick(stride=0) == BADARG and pick(stride=-1) == BADARG
    assert pick(M=-1) == BADARG and pick(H=0, ld=0) == BADARG and pick(V=0) == BADARG
    assert pick(M=0) == 0 and pick(M=0, live=None) == 0 and pick(M=0, n_live=None) == 0


def test_tile_tables_are_described_without_a_gpu():
    from s2vt_amd import ops
    L = s2vt_amd.lib()
    assert L.s2vt_tile_count(3) == BADARG and L.s2vt_tile_count(-1) == BADARG and L.s2vt_tile_count(5) == BADARG
    d = _lib.TileDesc()
    assert L.s2vt_tile_info(0, 0, None) == BADARG and L.s2vt_tile_info(3, 0, ctypes.byref(d)) == BADARG
    assert ops.tile_count(_lib.TILE_STORE) == ops.tile_count(_lib.TILE_STORE_NT)                    # index-compatible tables
    for kind in (_lib.TILE_STORE, _lib.TILE_LSTM, _lib.TILE_PICK, _lib.TILE_STORE_NT):
        n = ops.tile_count(kind)
        assert n >= 8 and L.s2vt_tile_info(kind, n, ctypes.byref(d)) == BADARG and L.s2vt_tile_info(kind, -1, ctypes.byref(d)) == BADARG
        infos = [ops.tile_info(kind, i) for i in range(n)]
        assert len({t["name"] for t in infos}) == n
        for t in infos:
            assert t["rows"] % 16 == 0 and t["rows"] > 0 and t["cols"] % 16 == 0 and t["cols"] > 0
            assert t["has_scalar"] == (t["fallback"] < 0)                                           # only the LDS-DMA entries lack a scalar form
            if t["fallback"] >= 0:                                                                  # a fallback has every form its table has
                f = infos[t["fallback"]]
                assert f["fallback"] < 0 and f["has_scalar"] and (f["has_live"] or kind == _lib.TILE_STORE_NT)
            assert t["has_live"] or t["fallback"] >= 0 or kind == _lib.TILE_STORE_NT
        assert not any(t["has_live"] for t in infos) if kind == _lib.TILE_STORE_NT else any(t["has_live"] for t in infos)


def _model(residual, **kw):
    from s2vt_amd import model as M
    return M.Video_Caption_Generator(16, 11, 3, 4, 2, 5, 2, 3, device="cpu", seed=5, residual=residual, **kw)


def test_python_flag_rides_in_the_dims_and_refuses_what_is_not_built():
    from s2vt_amd import multitask, ops, residual
    assert ops.make_dims(16, 11, 3, 4, 2, 3).reserved == 0 and ops.make_dims(16, 11, 3, 4, 2, 3, residual=True).reserved == RES
    assert _model(False).dims.reserved == 0 and not _model(False).residual
    m = _model(True)
    assert m.dims.reserved == RES and m.residual
    assert residual.Video_Caption_Generator(16, 11, 3, 4, 2, 5, 2, 3, device="cpu").dims.reserved == RES
    assert multitask.Video_Caption_Generator(16, 11, 3, 4, 2, 5, 2, 3, device="cpu", feature_dim=16, label_dim=4, residual=True).dims.reserved == RES
    video = np.zeros((2, 2, 16), np.float32); cap = np.ones((2, 3), np.int64)
    for call in (lambda: m.mix_sample(video, cap), lambda: m.scheduled_update(video, cap, 1e-3), m.build_mix_sample, m.build_scheduled_model):
        with pytest.raises(ValueError, match="residual"):
            call()


def test_checkpoints_are_the_same_in_both_directions():
    a, b = _model(False), _model(True)
    for src, dst in ((a, b), (b, a)):
        for n in src.store.names:
            src.store.p[n].copy_(src.store.p[n] + 1.0)
        sd = src.state_dict()
        assert set(sd) == set(dst.state_dict())
        dst.load_state_dict(sd)
        for n in src.store.names:
            assert np.array_equal(dst.store.p[n].numpy(), src.store.p[n].numpy()), n


def _generic_args(argtypes, dims_ref, ap_ref):
    """One harmless value per parameter of a signature in _lib.SIGNATURES: never dereferenced when the dims are refused first."""
    out = []
    for t in argtypes:
        if t is _lib._DP:
            out.append(dims_ref)
        elif t is _lib._AP:
            out.append(ap_ref)
        elif t is _lib._vp:
            out.append(ONE)
        elif t is _lib._f32:
            out.append(1.0)
        elif t is _lib._sz:
            out.append(1 << 20)
        elif t in (_lib._i32, _lib._i64, _lib._u64, _lib._u32):
            out.append(2)
        else:
            raise AssertionError(f"no value for {t}")
    return out


def test_every_attention_entry_point_that_takes_dims_refuses_the_bit():
    """Table-driven over _lib.SIGNATURES: each s2vt_attn_* with an s2vt_dims parameter returns S2VT_E_BADARG (size functions: 0) with the
    residual bit, and with an unknown bit, before it looks at any other argument."""
    L = s2vt_amd.lib()
    ap = _lib.AttnParams()
    for n, _ in _lib.AttnParams._fields_:
        setattr(ap, n, 256)
    names = [n for n, (_, args) in _lib.SIGNATURES.items() if n.startswith("s2vt_attn_") and _lib._DP in args]
    assert len(names) >= 14 and {"s2vt_attn_teacher_forced_fwd", "s2vt_attn_teacher_forced_fwd_rows", "s2vt_attn_bptt_bwd", "s2vt_attn_bptt_bwd_rows",
                                 "s2vt_attn_sample", "s2vt_attn_sample_ex", "s2vt_attn_decode_greedy", "s2vt_attn_beam_encode", "s2vt_attn_beam_step",
                                 "s2vt_attn_step_scalars", "s2vt_attn_step_scalars_rows"} <= set(names)
    for bits in (RES, 2):
        d = _dims(bits=bits)
        for n in names:
            res, args = _lib.SIGNATURES[n]
            rc = getattr(L, n)(*_generic_args(args, ctypes.byref(d), ctypes.byref(ap)))
            assert rc == (0 if res is _lib._sz else BADARG), (n, bits, rc)
    for n in names:                                     # ... and the size functions still answer for a plain model
        res, args = _lib.SIGNATURES[n]
        if res is _lib._sz:
            assert getattr(L, n)(*_generic_args(args, ctypes.byref(_dims()), None)) > 0, n


def test_config_carries_the_flag():
    from s2vt_amd import train_common
    assert train_common.Config().residual is False and train_common.Config(residual=True).residual is True


@pytest.mark.parametrize("module,extra", [("train_xe", []), ("train_rl", [])])
def test_training_clis_parse_the_flag_into_the_config(monkeypatch, module, extra):
    """main(argv) up to the call of train(): --residual reaches Config.residual (the corpus files are not opened here; the drivers
    themselves run in tests/test_gpu_residual_cli.py)."""
    import importlib
    mod = importlib.import_module(f"s2vt_amd.{module}")
    seen = []
    monkeypatch.setattr(mod, "Corpus", lambda *a, **k: None)
    monkeypatch.setattr(mod, "train", lambda cfg, *a, **k: seen.append(cfg))
    base = ["--train-sents", "s", "--train-feats", "f", "--vocab", "v"] + extra
    mod.main(base)
    mod.main(base + ["--residual"])
    assert [c.residual for c in seen] == [False, True]


def test_beam_eval_cli_knows_the_flag():
    from s2vt_amd import beam_eval
    with pytest.raises(SystemExit) as e:
        beam_eval.main(["--residual", "--no-such-flag"])
    assert e.value.code == 2                                  # argparse: the unknown flag, not --residual
    with pytest.raises(Exception) as e:                       # parsed; stops at the missing files
        beam_eval.main(["--residual", "--checkpoint", "/nonexistent/c", "--test-sents", "/nonexistent/s", "--test-feats", "/nonexistent/f", "--vocab", "/nonexistent/v"])
    assert not (isinstance(e.value, SystemExit) and e.value.code == 2)
