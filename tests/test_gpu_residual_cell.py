"""s2vt_lstm_cell_fwd_res on the GPU: the fused cell step with a residual operand, out[m] = dropout(h'[m]) + res[row(m)], over every
cell-step tile of the table (as tests/test_gpu_fwd.py iterates them), with the operand given plainly, broadcast (rowmod) and gathered
(rowidx); then the same call inside guard bands."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (M, E, H): one ragged tile; exact 64-row tiles; a ragged last tile of every row count; two 96-row tiles + 8 rows; the bench width
SHAPES = [(5, 3, 4), (64, 32, 64), (70, 12, 20), (200, 8, 36), (96, 500, 1000)]


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _inputs(M, E, H):
    rng = np.random.default_rng(M + H)
    W = rng.uniform(-.3, .3, (E + H, 4 * H)).astype(np.float32); b = rng.uniform(-.5, .5, 4 * H).astype(np.float32)
    x = rng.standard_normal((M, E)).astype(np.float32); c = rng.standard_normal((M, H)).astype(np.float32)
    h = rng.uniform(-1, 1, (M, H)).astype(np.float32)
    vid = rng.integers(0, 1000, M).astype(np.int32); sid = rng.integers(0, 5, M).astype(np.int32)
    mod = 3 if M < 64 else 16
    table = rng.standard_normal((M + 7, H)).astype(np.float32)
    idx = rng.integers(0, M + 7, M).astype(np.int32)
    # (name, what the call is given, rowmod, rowidx, the rows it must add)
    variants = [("plain", table[:M], 0, None, table[:M]), ("rowmod", table[:mod], mod, None, table[np.arange(M) % mod]),
                ("rowidx", table, 0, idx, table[idx]), ("rowmod+rowidx", table, mod, idx[:mod], table[idx[np.arange(M) % mod]])]
    return W, b, x, c, h, vid, sid, variants


@pytest.mark.parametrize("M,E,H", SHAPES)
def test_cell_with_residual_operand_all_tiles(gpu, oracle, M, E, H):
    W, b, x, c, h, vid, sid, variants = _inputs(M, E, H)
    p = {"lstm1_W": W, "lstm1_b": b}
    dW, db, dx, dh, dc, dvid, dsid = (_dev(a) for a in (W, b, x, h, c, vid, sid))
    for keep, code in ((1.0, 0), (0.9, 258)):
        mask = None if keep >= 1 else oracle.dropout_mask(77, vid, sid, code, keep, H)
        rc, rh, rout, rg, _ = oracle.lstm1_step(p, x, c, h, mask, keep, want_gates=True)
        pc, ph, pout, pg = gpu.lstm_cell_fwd(gpu.operand(dx), None, dh, dc, dW, db, M, keep=keep, seed=77, video_id=dvid, sample_id=dsid,
                                             drop_code=code, want_gates=True)
        assert np.array_equal(pout.cpu().numpy(), rout)
        for cfg in range(-1, gpu.tile_count(1) + 1):       # every entry of fwd.hip kLstm; the count itself = out of range = the library's choice, as -1
            name, given, mod, idx, rows = variants[(cfg + 1) % len(variants)] if H >= 1000 else (None,) * 5
            for v in (variants if name is None else [(name, given, mod, idx, rows)]):       # (the widest shape: the variants take turns)
                name, given, mod, idx, rows = v
                res = gpu.operand(_dev(given), rowidx=None if idx is None else _dev(idx), rowmod=mod)
                gc, gh, gout, gg = gpu.lstm_cell_fwd(gpu.operand(dx), None, dh, dc, dW, db, M, keep=keep, seed=77, video_id=dvid,
                                                     sample_id=dsid, drop_code=code, want_gates=True, tile_cfg=cfg, res=res)
                what = (keep, cfg, name)
                # c, h and the gates: those of the plain call (and of the oracle); out: the oracle's dropped output + the operand's row, one fp32 addition
                assert np.array_equal(gc.cpu().numpy(), pc.cpu().numpy()) and np.array_equal(gh.cpu().numpy(), ph.cpu().numpy()), what
                assert np.array_equal(gg.cpu().numpy(), pg.cpu().numpy()) and np.array_equal(gc.cpu().numpy(), rc), what
                assert np.array_equal(gout.cpu().numpy(), (rout + rows).astype(np.float32)), what
                assert not np.array_equal(gout.cpu().numpy(), rout), what


def test_operand_and_state_broadcast_over_sample_blocks(gpu, oracle):
    """The single-op call as the sampler's first step uses it: the state and the residual operand of B videos broadcast over the sample
    blocks (state_rowmod, res rowmod).  The live-row (OM) residual instantiations -- what the early-exit sampler launches for the tiles it
    picks, tests/test_gpu_residual_sample.py::test_stop_at_eos... -- are launched for EVERY tile of the table, vector and scalar path, through
    s2vt_lstm_cell_fwd_live in tests/test_gpu_live_tiles.py::test_cell_tiles."""
    M, E, H, B = 12, 6, 20, 3
    W, b, x, c, h, vid, sid, _ = _inputs(M, E, H)
    p = {"lstm1_W": W, "lstm1_b": b}
    rc, rh, rout, _, _ = oracle.lstm1_step(p, x, np.tile(c[:B], (4, 1)), np.tile(h[:B], (4, 1)))
    res = np.random.default_rng(0).standard_normal((B, H)).astype(np.float32)
    gc, gh, gout, _ = gpu.lstm_cell_fwd(gpu.operand(_dev(x)), None, _dev(h[:B]), _dev(c[:B]), _dev(W), _dev(b), M, state_rowmod=B,
                                        res=gpu.operand(_dev(res), rowmod=B))
    assert np.array_equal(gc.cpu().numpy(), rc) and np.array_equal(gh.cpu().numpy(), rh)
    assert np.array_equal(gout.cpu().numpy(), (rout + np.tile(res, (4, 1))).astype(np.float32))


@pytest.mark.parametrize("M,E,H", [(5, 3, 4), (70, 12, 20), (200, 8, 36)])
@pytest.mark.parametrize("keep", [1.0, 0.9])
def test_inside_guard_bands(gpu, oracle, M, E, H, keep):
    """Every operand the call reads or writes per row lies in a guarded window (tests/guardband.py); the residual operand's rows are wider
    than H and its window is 4-byte, not 16-byte aligned."""
    import torch
    import s2vt_amd
    from s2vt_amd import _lib
    from guardband import Guarded
    L = s2vt_amd.lib()
    W, b, x, c, h, vid, sid, variants = _inputs(M, E, H)
    p = {"lstm1_W": W, "lstm1_b": b}
    code = 258
    mask = None if keep >= 1 else oracle.dropout_mask(77, vid, sid, code, keep, H)
    rc, rh, rout, rg, _ = oracle.lstm1_step(p, x, c, h, mask, keep, want_gates=True)
    dW, db = _dev(W), _dev(b)
    gx, gh, gc = Guarded.of(x, name="x"), Guarded.of(h, name="h_prev"), Guarded.of(c, name="c_prev")
    gvid, gsid = Guarded.of(vid, fill=0, name="video_id"), Guarded.of(sid, fill=0, name="sample_id")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, given, mod, idx, rows in variants:
        gres = Guarded.of(given, ld=H + 5, lead=65, name="res")
        gidx = None if idx is None else Guarded.of(idx, fill=0, name="res rowidx")
        outs = {n: Guarded(M, w, name=n) for n, w in (("c_new", H), ("h_new", H), ("out", H), ("gates", 4 * H))}
        x0 = _lib.Operand(gx.view.data_ptr(), None, gx.ld, E, 0, 0)
        res = _lib.Operand(gres.view.data_ptr(), None if gidx is None else gidx.view.data_ptr(), gres.ld, H, mod, 0)
        for cfg in (-1, 0, 4, 8, 12):
            for o in outs.values():
                o.reset()
            rcode = L.s2vt_lstm_cell_fwd_res(ctypes.byref(x0), None, gh.ptr, gc.ptr, 0, ctypes.c_void_p(dW.data_ptr()), ctypes.c_void_p(db.data_ptr()),
                                             ctypes.byref(res), outs["c_new"].ptr, outs["h_new"].ptr, outs["out"].ptr, outs["gates"].ptr, M, H,
                                             float(keep), 77, gvid.ptr, gsid.ptr, code, cfg, stream)
            assert rcode == 0, (name, cfg)
            torch.cuda.synchronize()
            assert np.array_equal(outs["c_new"].numpy(), rc) and np.array_equal(outs["h_new"].numpy(), rh), (name, cfg)
            assert np.array_equal(outs["gates"].numpy(), rg), (name, cfg)
            assert np.array_equal(outs["out"].numpy(), (rout + rows).astype(np.float32)), (name, cfg)
            for g in list(outs.values()) + [gx, gh, gc, gvid, gsid, gres] + ([] if gidx is None else [gidx]):
                g.assert_intact()
