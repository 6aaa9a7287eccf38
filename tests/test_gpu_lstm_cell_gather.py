"""The gathered-state instantiations of the fused LSTM cell (gemm_mfma.h, GS: GemmArgs::cinit_rowidx / cprev_rowidx) on the GPU, every entry
of the cell-step tile table and the library's choice, through the single-op entry s2vt_lstm_cell_fwd_gather.

    z[m] = Cinit[cinit_rowidx[m]] + [x[word[m]] ; h_prev[state_rowidx[m]]] @ W + b,   the cell on c_prev[state_rowidx[m]]

as a beam step launches it: the x segment is a table gathered by its own rowidx (the Wemb rows by word), the state and the carried
partial are small source arrays -- 5 state rows, 3 Cinit rows -- read through index arrays that repeat rows, leave rows unused, are the
identity (then the sources have M rows), or are NULL on either side (row m of an M-row source).  Shapes: (H, E) = (32, 24) takes the
16-byte path, (18, 10) the scalar path (H % 4 != 0); M = 1, 17 (a ragged second 16-row tile) and 97 (one past the 96-row tile).
On the scalar path an index does not always run its own tile's kernel: the LDS-DMA entries hand the launch to their `fallback`, and
gw16x16u(1x4)k64, which has no scalar gathered-state twin, to gw16x16u(1x4) -- what a caller who forces that index gets, same bits.

Expected values are the CPU oracle's pieces on the host-gathered rows: gemm_chain continued from the gathered Cinit, bias_add,
lstm_pointwise.  No tolerance: c_new, h_new and gates are compared bit for bit.  Outputs and sources lie in guard bands
(tests/guardband.py); the guards of the index arrays hold a valid index.  The sources must come back unwritten."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LSTM = 1
SHAPES = {"vector": (32, 24), "scalar": (18, 10)}
ROWS = (1, 17, 97)
NS, NC, NTAB = 5, 3, 7                       # state rows, Cinit rows, rows of the x table
VARIANTS = ("repeat", "unused", "identity", "state-null", "cinit-null", "no-cinit")


def _case(path, M):
    H, E = SHAPES[path]
    rng = np.random.default_rng(1000 * H + M)
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    return dict(H=H, E=E, W=(u(E + H, 4 * H) * 0.3).astype(np.float32), b=u(4 * H), tab=u(NTAB, E), word=rng.integers(0, NTAB, M).astype(np.int32),
                h5=u(NS, H), c5=u(NS, H), ci3=u(NC, 4 * H), hM=u(M, H), cM=u(M, H), ciM=u(M, 4 * H))


def _maps(variant, M):
    """(state_rowidx | None, cinit_rowidx | None, state sources are the M-row ones, Cinit: 3-row / M-row / absent)"""
    m = np.arange(M)
    if variant == "repeat":                  # every source row, many times over at M > 5
        return ((m * 3 + 1) % NS).astype(np.int32), ((m * 2 + 1) % NC).astype(np.int32), False, "3"
    if variant == "unused":                  # state rows 1 and 3 and Cinit row 1 are never read
        return np.array([4, 0, 2], np.int32)[m % 3], np.array([2, 0], np.int32)[(m // 2) % 2], False, "3"
    if variant == "identity":
        return m.astype(np.int32), m.astype(np.int32), True, "M"
    if variant == "state-null":
        return None, ((m + 2) % NC).astype(np.int32), True, "3"
    if variant == "cinit-null":
        return ((m * 2) % NS).astype(np.int32), None, False, "M"
    return ((m + 3) % NS).astype(np.int32), None, False, None          # no-cinit: the chain starts from +0


def _expected(oracle, c, M, sidx, cidx, state_M, cinit):
    hs, cs = (c["hM"], c["cM"]) if state_M else (c["h5"], c["c5"])
    rs = np.arange(M) if sidx is None else sidx
    A = np.ascontiguousarray(np.concatenate([c["tab"][c["word"]], hs[rs]], axis=1))
    z0 = None
    if cinit is not None:
        src = c["ciM"] if cinit == "M" else c["ci3"]
        z0 = np.ascontiguousarray(src[np.arange(M) if cidx is None else cidx]).copy()
    z = oracle.bias_add(oracle.gemm_chain(A, c["W"], C_=z0), c["b"])
    cn, hn, _, gates = oracle.lstm_pointwise(z, np.ascontiguousarray(cs[rs]), want_gates=True)
    return cn, hn, gates


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("path", list(SHAPES))
def test_gathered_cell_every_tile(gpu, oracle, path, M):
    import torch
    from guardband import Guarded
    c = _case(path, M)
    H, E = c["H"], c["E"]
    vector = path == "vector"
    lead, pad = (64, 4) if vector else (65, 0)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    dW, db = dev(c["W"]), dev(c["b"])
    gtab = Guarded.of(c["tab"], ld=E + pad, lead=lead, name="x table")
    gword = Guarded.of(c["word"], fill=0, name="word")
    src = {k: Guarded.of(c[k], lead=lead, name=k) for k in ("h5", "c5", "hM", "cM")}
    src.update({k: Guarded.of(c[k], ld=4 * H + pad, lead=lead, name=k) for k in ("ci3", "ciM")})
    outs = {n: Guarded(M, w, lead=lead, name=n) for n, w in (("c_new", H), ("h_new", H), ("gates", 4 * H))}
    x = gpu.operand(gtab.view, rowidx=gword.view[0])
    tiles = list(range(gpu.tile_count(LSTM))) + [-1]
    assert len(tiles) >= 9
    for variant in VARIANTS:
        sidx, cidx, state_M, cinit = _maps(variant, M)
        exp = [dev(a) for a in _expected(oracle, c, M, sidx, cidx, state_M, cinit)]
        gs = None if sidx is None else Guarded.of(sidx, fill=0, name="state_rowidx")
        gc = None if cidx is None else Guarded.of(cidx, fill=0, name="cinit_rowidx")
        h_prev, c_prev = (src["hM"], src["cM"]) if state_M else (src["h5"], src["c5"])
        ci = None if cinit is None else src["ciM" if cinit == "M" else "ci3"]
        for tile in tiles:
            what = (path, M, variant, tile)
            for g in outs.values():
                g.reset()
            gpu.lstm_cell_fwd_gather(x, None, h_prev.view, c_prev.view, dW, db, M, state_rowidx=None if gs is None else gs.view[0],
                                     cinit=None if ci is None else ci.view, cinit_rowidx=None if gc is None else gc.view[0], tile_cfg=tile,
                                     c_new=outs["c_new"].view, h_new=outs["h_new"].view, gates=outs["gates"].view)
            for g, e in zip(outs.values(), exp):
                assert torch.equal(g.view, e), (what, g.name)
                g.assert_intact()
        for g in (gs, gc):
            if g is not None:
                g.assert_intact()
    # identity maps and no Cinit: the plain cell, bit for bit
    ident = Guarded.of(np.arange(M, dtype=np.int32), fill=0, name="identity")
    xd = gpu.operand(dev(c["tab"][c["word"]]))
    c0, h0, _, g0 = gpu.lstm_cell_fwd(xd, None, src["hM"].view, src["cM"].view, dW, db, M, want_gates=True)
    for tile in tiles:
        c1, h1, g1 = gpu.lstm_cell_fwd_gather(x, None, src["hM"].view, src["cM"].view, dW, db, M, state_rowidx=ident.view[0], want_gates=True,
                                              tile_cfg=tile)
        assert torch.equal(c1, c0) and torch.equal(h1, h0) and torch.equal(g1, g0), (path, M, "identity == plain", tile)
    # nothing wrote to a source
    for k, g in src.items():
        assert np.array_equal(g.numpy(), c[k]), k
        g.assert_intact()
    assert np.array_equal(gtab.numpy(), c["tab"]) and np.array_equal(gword.numpy()[0], c["word"])
    gtab.assert_intact(); gword.assert_intact(); ident.assert_intact()
