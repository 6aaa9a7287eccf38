"""The fp32 forward contractions through the C ABI inside guard bands (tests/guardband.py): s2vt_gemm and s2vt_gemm_nt on every tile
of fwd.hip's tables, s2vt_lstm_cell_fwd and s2vt_vocab_pick on every tile of theirs -- bit for bit against the CPU oracle, at shapes one
row and a few columns past a tile, in four layouts:

    dense       every operand and output with ld == cols and a 16-byte aligned window, NaN guards around each;
    strided     every 2-D operand and output with its own row stride cols + 4 j: still the vector / LDS-DMA path;
    odd-ld:X    ld = cols + 1 on operand X alone: one `ld & 3` sends the launch to the scalar kernels;
    mis:X       operand X alone starts 4 bytes past a 16-byte boundary, on shapes with K % 4 == N % 4 == 0.

A store outside an output changes a guard (rows >= M of a partial tile, columns >= N, a packed pick word of a row >= M); a load outside
a row of an input reads a NaN that reaches a stored output.  Index arrays (rowidx, video_id, sample_id) carry 256 trailing entries that
hold a valid index.  For the LDS-DMA tiles the in-library launch profiler tells which kernel ran: the `+Ndma` tile on aligned operands,
its register-staged `fallback` tile (scalar form) otherwise."""
import ctypes as C

import numpy as np
import pytest

from guardband import Guarded
from test_gpu_timed_tiles import _launched_tiles

pytestmark = pytest.mark.gpu

# fwd.hip kStore / kStoreNT (the NT names carry the prefix "nt"): index -> name, and the LDS-DMA entries' fallback
STORE_NAMES = ["64x64(4x1)", "64x128(2x2)", "128x128(2x2)", "128x32(4x1)", "64x32(4x1)", "64x96(2x2)", "96x96(2x2)", "96x128(2x2)",
               "128x128(2x2)+4dma2", "96x96(2x2)+4dma2", "96x96(2x2)+4dma3", "128x128(2x2)+2dma2"]
STORE_FALLBACK = {8: 2, 9: 6, 10: 6, 11: 2}
IDX_TAIL = 256


def _lib():
    import s2vt_amd
    return s2vt_amd.lib()


def _operand(g=None, k=None, rowidx=None, rowmod=0):
    from s2vt_amd._lib import Operand
    if g is None:
        return Operand(None, None, 0, int(k), 0, 0)
    op = Operand(g.view.data_ptr(), None if rowidx is None else rowidx.view.data_ptr(), g.ld, g.cols if k is None else int(k), int(rowmod), 0)
    op._keep = (g, rowidx)
    return op


def _index(values, valid, name):
    """An int32 index array whose guards (256 entries behind it) hold the valid index `valid`."""
    return Guarded.of(np.asarray(values, np.int32), tail=IDX_TAIL, fill=int(valid), name=name)


def _intact(*gs):
    for g in gs:
        if g is not None:
            g.assert_intact()


def _tile_of(gpu, cls, call):
    rc, tiles = _launched_tiles(gpu, call)
    assert rc == 0
    names = [n for (c, n), cnt in tiles.items() if c == cls]
    assert len(names) == 1, tiles
    return names[0]


# ---------------------------------------------------------------------------------------------------- s2vt_gemm / s2vt_gemm_nt
GEMM_SHAPES = [(129, 132, 132),      # one row and four columns past a 128 tile; four K chunks and a ragged one: the 2- and 3-stage rings wrap
               (97, 36, 100),        # past the 96 tiles
               (65, 64, 68)]
GEMM_VARIANTS = ["dense", "strided", "odd-ld:A", "odd-ld:W", "odd-ld:C", "mis:A", "mis:W", "mis:C"]


def _layout(variant, who, j):
    """(pad, lead) of operand `who` in `variant`; j: its own stride step in the strided layout."""
    kind, _, target = variant.partition(":")
    if kind == "strided":
        return 4 * j, 64
    if kind == "odd-ld" and target == who:
        return 1, 64
    if kind == "mis" and target == who:
        return 0, 65
    return 0, 64


@pytest.fixture(scope="module")
def gemm_refs(oracle):
    """Inputs and oracle results per shape, computed once: plain, + bias, tanh(+ bias), chain continued from Cinit."""
    refs = {}
    for M, K, N in GEMM_SHAPES:
        rng = np.random.default_rng(M * 1000 + K)
        A = rng.standard_normal((M, K)).astype(np.float32); W = rng.standard_normal((K, N)).astype(np.float32)
        b = rng.standard_normal(N).astype(np.float32); Ci = rng.standard_normal((M, N)).astype(np.float32)
        with_bias = oracle.bias_add(oracle.gemm_chain(A, W), b)
        with_cinit = Ci.copy(); oracle.gemm_chain(A, W, with_cinit)
        refs[(M, K, N)] = dict(A=A, W=W, b=b, Ci=Ci, bias=with_bias, tanh=oracle.det_tanh(with_bias), cinit=with_cinit)
    return refs


@pytest.mark.parametrize("variant", GEMM_VARIANTS)
@pytest.mark.parametrize("M,K,N", GEMM_SHAPES)
@pytest.mark.parametrize("form", ["nn", "nt"])
def test_gemm_all_tiles_guarded(gpu, gemm_refs, form, M, K, N, variant):
    L, st = _lib(), gpu._stream()
    r = gemm_refs[(M, K, N)]
    nt = form == "nt"
    fn = L.s2vt_gemm_nt if nt else L.s2vt_gemm
    pa, la = _layout(variant, "A", 1)
    pw, lw = _layout(variant, "W", 2)
    pc, lc = _layout(variant, "C", 3)
    Wh = np.ascontiguousarray(r["W"].T) if nt else r["W"]                      # W^T [N, K] for the NT form
    gA = Guarded.of(r["A"], ld=K + pa, lead=la, name="A")
    gW = Guarded.of(Wh, ld=Wh.shape[1] + pw, lead=lw, name="W")
    gb = Guarded.of(r["b"], lead=lc, name="bias")
    gCi = Guarded.of(r["Ci"], ld=N + (pc + 4 if pc > 1 else pc), lead=lc, name="Cinit")
    out = Guarded(M, N, ld=N + pc, lead=lc, name="C")
    kind, _, target = variant.partition(":")
    assert gA.aligned16 == (variant != "mis:A") and gW.aligned16 == (variant != "mis:W") and out.aligned16 == (variant != "mis:C")
    scalar = kind in ("odd-ld", "mis") and target in ("A", "W")               # what can_vec() refuses; C / Cinit / bias are scalar accesses
    segs = (type(_operand(gA)) * 1)(_operand(gA))
    n_cfgs = gpu.tile_count(4 if nt else 0)
    for cfg in range(-1, n_cfgs + 1):                                         # every entry of the table; the count itself = out of range = auto
        for mode in ("bias", "tanh", "cinit"):
            out.reset()
            call = lambda: fn(segs, 1, gW.ptr, gW.ld, None if mode == "cinit" else gb.ptr, gCi.ptr if mode == "cinit" else None,
                              gCi.ld if mode == "cinit" else 0, out.ptr, out.ld, M, N, int(mode == "tanh"), cfg, st)
            if 8 <= cfg < n_cfgs and mode == "bias":
                want = STORE_NAMES[STORE_FALLBACK[cfg] if scalar else cfg]
                assert _tile_of(gpu, 4 if nt else 0, call) == ("nt" if nt else "") + want, (cfg, variant)
            else:
                assert call() == 0
            assert np.array_equal(out.bits(), r[mode].view(np.int32)), (cfg, mode, variant)
            out.assert_intact()
    _intact(gA, gW, gb, gCi)


SEG_SHAPE = (70, 100, 36, 64, 132, 50, 7)            # M, k0 (broadcast, rowmod), k1 (gathered), k2 (plain), N, table rows, rowmod
SEG_VARIANTS = ["dense", "strided"] + [f"{k}:{s}" for k in ("odd-ld", "mis") for s in ("s0", "s1", "s2")]


@pytest.fixture(scope="module")
def seg_ref(oracle):
    M, k0, k1, k2, N, T, mod = SEG_SHAPE
    rng = np.random.default_rng(11)
    A0 = rng.standard_normal((mod, k0)).astype(np.float32)
    Tab = rng.standard_normal((T, k1)).astype(np.float32)
    idx = rng.integers(0, T, M).astype(np.int32)
    idx[0], idx[1] = T - 1, 0
    A2 = rng.standard_normal((M, k2)).astype(np.float32)
    W = rng.standard_normal((k0 + k1 + k2, N)).astype(np.float32)
    Ci = rng.standard_normal((M, N)).astype(np.float32)
    ref = Ci.copy()
    oracle.gemm_chain(np.ascontiguousarray(A0[np.arange(M) % mod]), W[:k0], ref)
    oracle.gemm_chain(Tab, W[k0:k0 + k1], ref, rowidx=idx)
    oracle.gemm_chain(A2, W[k0 + k1:], ref)
    return dict(A0=A0, Tab=Tab, idx=idx, A2=A2, W=W, Ci=Ci, ref=ref)


@pytest.mark.parametrize("variant", SEG_VARIANTS)
@pytest.mark.parametrize("form", ["nn", "nt"])
def test_gemm_three_segments_guarded(gpu, seg_ref, form, variant):
    """[broadcast rows m % 7 ; gathered rows ; plain rows] @ W continuing a strided Cinit; odd-ld / mis on ONE segment, the others aligned."""
    L, st = _lib(), gpu._stream()
    M, k0, k1, k2, N, T, mod = SEG_SHAPE
    r = seg_ref
    nt = form == "nt"
    fn = L.s2vt_gemm_nt if nt else L.s2vt_gemm
    lay = [_layout(variant, f"s{s}", s + 1) for s in range(3)]
    g0 = Guarded.of(r["A0"], ld=k0 + lay[0][0], lead=lay[0][1], name="seg0 (broadcast)")
    g1 = Guarded.of(r["Tab"], ld=k1 + lay[1][0], lead=lay[1][1], name="seg1 (table)")
    g2 = Guarded.of(r["A2"], ld=k2 + lay[2][0], lead=lay[2][1], name="seg2")
    gi = _index(r["idx"], T - 1, "rowidx")
    strided = variant == "strided"
    Wh = np.ascontiguousarray(r["W"].T) if nt else r["W"]
    gW = Guarded.of(Wh, ld=Wh.shape[1] + (16 if strided else 0), name="W")
    gCi = Guarded.of(r["Ci"], ld=N + (8 if strided else 0), name="Cinit")
    out = Guarded(M, N, ld=N + (20 if strided else 0), name="C")
    ops_ = [_operand(g0, rowmod=mod), _operand(g1, rowidx=gi), _operand(g2)]
    segs = (type(ops_[0]) * 3)(*ops_)
    scalar = variant not in ("dense", "strided")
    for cfg in (-1, 0, 2, 8, 9):
        out.reset()
        call = lambda: fn(segs, 3, gW.ptr, gW.ld, None, gCi.ptr, gCi.ld, out.ptr, out.ld, M, N, 0, cfg, st)
        if cfg >= 8:
            want = STORE_NAMES[STORE_FALLBACK[cfg] if scalar else cfg]
            assert _tile_of(gpu, 4 if nt else 0, call) == ("nt" if nt else "") + want, (cfg, variant)
        else:
            assert call() == 0
        assert np.array_equal(out.bits(), r["ref"].view(np.int32)), (cfg, variant)
        out.assert_intact()
    _intact(g0, g1, g2, gi, gW, gCi)


@pytest.mark.parametrize("strided", [False, True])
def test_gemm_nt_segment_offset_not_a_multiple_of_4(gpu, oracle, strided):
    """s2vt_operand has no kw field: a segment's column offset into Wt is the sum of the k of the segments before it.  A zero segment
    (ptr == NULL) of k = 6 is skipped by the `k & 3` test of can_vec() but moves the next segment to kw = 6 -- no 16-byte loads from
    Wt's rows at that offset: the scalar kernels, and an LDS-DMA tile's fallback, on operands that are otherwise vector-friendly."""
    L, st = _lib(), gpu._stream()
    M, K, N, kz = 70, 64, 68, 6
    rng = np.random.default_rng(6)
    A = rng.standard_normal((M, K)).astype(np.float32); Wt = rng.standard_normal((N, kz + K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    ref = oracle.bias_add(oracle.gemm_chain(A, np.ascontiguousarray(Wt[:, kz:].T)), b)
    gA = Guarded.of(A, ld=K + (4 if strided else 0), name="A")
    gW = Guarded.of(Wt, ld=kz + K + (6 if strided else 2), name="Wt")         # ldw = 72 / 76: a multiple of 4, so that only kw decides
    gb, out = Guarded.of(b, name="bias"), Guarded(M, N, ld=N + (8 if strided else 0), name="C")
    assert gW.ld % 4 == 0
    ops_ = [_operand(None, k=kz), _operand(gA)]
    segs = (type(ops_[0]) * 2)(*ops_)
    for cfg in (-1, 0, 2, 8, 9):
        out.reset()
        call = lambda: L.s2vt_gemm_nt(segs, 2, gW.ptr, gW.ld, gb.ptr, None, 0, out.ptr, out.ld, M, N, 0, cfg, st)
        if cfg >= 8:
            assert _tile_of(gpu, 4, call) == "nt" + STORE_NAMES[STORE_FALLBACK[cfg]], cfg
        else:
            assert call() == 0
        assert np.array_equal(out.bits(), ref.view(np.int32)), cfg
        out.assert_intact()
    _intact(gA, gW, gb)


# ---------------------------------------------------------------------------------------------------- s2vt_lstm_cell_fwd
LSTM_SHAPES = [(70, 12, 20), (97, 32, 64)]           # rows 70 .. 95 of a 96-row tile, one row past it; H = 20: a ragged 16-unit tile
LSTM_KEEP = [(1.0, 0), (0.9, 258)]


@pytest.fixture(scope="module")
def lstm_refs(oracle):
    refs = {}
    for M, E, H in LSTM_SHAPES:
        rng = np.random.default_rng(M + H)
        W = rng.uniform(-.3, .3, (E + H, 4 * H)).astype(np.float32); b = rng.uniform(-.5, .5, 4 * H).astype(np.float32)
        x = rng.standard_normal((M, E)).astype(np.float32); c = rng.standard_normal((M, H)).astype(np.float32)
        h = rng.uniform(-1, 1, (M, H)).astype(np.float32)
        vid = rng.integers(0, 1000, M).astype(np.int32); sid = rng.integers(0, 5, M).astype(np.int32)
        p = {"lstm1_W": W, "lstm1_b": b}
        res = {}
        for keep, code in LSTM_KEEP:
            mask = None if keep >= 1 else oracle.dropout_mask(77, vid, sid, code, keep, H)
            res[keep] = oracle.lstm1_step(p, x, c, h, mask, keep, want_gates=True)[:4]
        refs[(M, E, H)] = dict(W=W, b=b, x=x, c=c, h=h, vid=vid, sid=sid, res=res)
    return refs


@pytest.mark.parametrize("variant", ["dense", "strided", "odd-ld:x0", "mis:x0"])
@pytest.mark.parametrize("M,E,H", LSTM_SHAPES)
def test_lstm_cell_all_tiles_guarded(gpu, lstm_refs, M, E, H, variant):
    """Every entry of fwd.hip kLstm (and -1 / the table's size = auto): c_new, h_new, out and gates bit for bit against oracle.lstm1_step, nothing
    written in rows >= M.  W, b, c_prev and h_prev have no stride argument; x0 takes the layouts."""
    L, st = _lib(), gpu._stream()
    r = lstm_refs[(M, E, H)]
    px, lx = _layout(variant, "x0", 2)
    gx = Guarded.of(r["x"], ld=E + px, lead=lx, name="x0")
    assert gx.aligned16 == (variant != "mis:x0")
    gW, gb = Guarded.of(r["W"], name="W"), Guarded.of(r["b"], name="b")
    gc, gh = Guarded.of(r["c"], name="c_prev"), Guarded.of(r["h"], name="h_prev")
    gvid, gsid = _index(r["vid"], 0, "video_id"), _index(r["sid"], 0, "sample_id")
    outs = [Guarded(M, H, name=n) for n in ("c_new", "h_new", "out")] + [Guarded(M, 4 * H, name="gates")]
    x0 = _operand(gx)
    for keep, code in LSTM_KEEP:
        for cfg in range(-1, gpu.tile_count(1) + 1):
            for o in outs:
                o.reset()
            rc = L.s2vt_lstm_cell_fwd(C.byref(x0), None, gh.ptr, gc.ptr, 0, gW.ptr, gb.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr,
                                      M, H, keep, 77, gvid.ptr, gsid.ptr, code, cfg, st)
            assert rc == 0
            for o, want in zip(outs, r["res"][keep]):
                assert np.array_equal(o.bits(), want.view(np.int32)), (o.name, keep, cfg, variant)
                o.assert_intact()
    _intact(gx, gW, gb, gc, gh, gvid, gsid)


# ---------------------------------------------------------------------------------------------------- s2vt_vocab_pick
PICK_SHAPES = [(70, 20, 100), (33, 64, 260), (100, 36, 97)]


@pytest.fixture(scope="module")
def pick_refs(oracle):
    refs = {}
    for M, H, V in PICK_SHAPES:
        rng = np.random.default_rng(V)
        o2 = rng.uniform(-1, 1, (M, H)).astype(np.float32); W = rng.uniform(-.1, .1, (H, V)).astype(np.float32)
        b = rng.uniform(-.1, .1, V).astype(np.float32)
        vid = rng.integers(0, 500, M).astype(np.int32); sid = rng.integers(-1, 4, M).astype(np.int32)
        logits = oracle.xw_plus_b(o2, W, b)
        refs[(M, H, V)] = dict(o2=o2, W=W, b=b, vid=vid, sid=sid, logits=logits, tok=oracle.pick_tokens(logits, vid, sid, 5, 2024))
    return refs


@pytest.mark.parametrize("variant", ["dense", "strided", "odd-ld:out2", "mis:out2"])
@pytest.mark.parametrize("M,H,V", PICK_SHAPES)
def test_vocab_pick_all_tiles_guarded(gpu, pick_refs, M, H, V, variant):
    """Every entry of fwd.hip kPick (and -1 / the table's size = auto), with and without logits_out: ids and logits bit for bit against
    oracle.pick_tokens; packed (one 8-byte word per row, zero on entry), tokens_out and logits_out keep their guards."""
    import torch
    L, st = _lib(), gpu._stream()
    r = pick_refs[(M, H, V)]
    po, lo = _layout(variant, "out2", 3)
    go = Guarded.of(r["o2"], ld=H + po, lead=lo, name="out2")
    assert go.aligned16 == (variant != "mis:out2")
    gW, gb = Guarded.of(r["W"], name="W"), Guarded.of(r["b"], name="b")
    gvid, gsid = _index(r["vid"], 0, "video_id"), _index(r["sid"], 0, "sample_id")
    packed = Guarded(1, M, dtype=torch.int64, name="packed")
    tok, logits = Guarded(1, M, dtype=torch.int32, name="tokens_out"), Guarded(M, V, name="logits_out")
    for cfg in range(-1, gpu.tile_count(2) + 1):
        for want_logits in (True, False):
            packed.reset(); packed.view.zero_(); tok.reset(); logits.reset()
            rc = L.s2vt_vocab_pick(go.ptr, go.ld, gW.ptr, gb.ptr, M, H, V, gvid.ptr, gsid.ptr, 5, 2024, packed.ptr, tok.ptr,
                                   logits.ptr if want_logits else None, cfg, st)
            assert rc == 0
            assert np.array_equal(tok.numpy()[0], r["tok"]), (cfg, want_logits, variant)
            words = packed.bits()[0]
            assert np.array_equal((~words & 0xFFFFFFFF).astype(np.int32), r["tok"]), (cfg, "packed low words = ~token")
            if want_logits:
                assert np.array_equal(logits.bits(), r["logits"].view(np.int32)), (cfg, variant)
            else:
                assert (logits._ibuf == logits._sentinel).all()
            _intact(packed, tok, logits)
    _intact(go, gW, gb, gvid, gsid)
