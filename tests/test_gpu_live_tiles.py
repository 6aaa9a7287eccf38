"""The live-row instantiations of gemm_kernel (GemmArgs::omap / m_dev) on the GPU, every entry of the store, cell-step and pick tile
tables through the single-op entries s2vt_gemm_live, s2vt_lstm_cell_fwd_live (plain and residual) and s2vt_vocab_pick_live, on the vector
path and on the scalar path.  The early-exit samplers launch a handful of these kernels; every other one is an environment knob or a
change of the tile choice away from the product path.

The entries, their rows and their fallbacks come from s2vt_tile_count / s2vt_tile_info; inputs, lists, counts and the oracle's expected
rows from tests/live_tile_cases.py, whose module docstring says how a wrong row shows by value (tests/test_live_tile_cases_cpu.py shows
that the expectation rejects four half-built kernels).  Every output, the list, the count and the packed words lie in guard bands
(tests/guardband.py).  After each launch the WHOLE allocation of every output is compared, bit for bit, with its image: the oracle's rows on
the live rows, the sentinel on every other row (the dedicated NaN row among them), in every pad and guard -- at count 0 nothing but
sentinels.  The live rows are then compared bit for bit with the dense call of the same tile_cfg on the gathered rows, and the profiler row
of the launch names the entry the case is about (or the entry that takes the launch for it).  No tolerances: the contract is bit identity."""
import ctypes

import numpy as np
import pytest

import live_tile_cases as lc

pytestmark = pytest.mark.gpu

STORE, LSTM, PICK = 0, 1, 2
R = lc.R


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _entries(gpu, kind):
    infos = [gpu.tile_info(kind, i) for i in range(gpu.tile_count(kind))]
    assert len(infos) >= 8 and any(t["has_live"] for t in infos)
    return infos


def _takes_the_launch(infos, i, vector):
    """The entry a live-row launch forced to entry i runs: i itself, or its fallback where it has no scalar / no live-row form."""
    if not vector and not infos[i]["has_scalar"]:
        i = infos[i]["fallback"]
    if not infos[i]["has_live"]:
        i = infos[i]["fallback"]
    assert i >= 0 and infos[i]["has_live"] and (vector or infos[i]["has_scalar"])
    return i


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _Lists:
    """`live` and `n_live` of one (list, count) in guard bands whose guards hold valid values (DEAD / 0).  A list of all R rows goes without
    a count (n_live == NULL: all M entries), except at the count above R."""
    def __init__(self, kind, n):
        from guardband import Guarded
        self.kind, self.n = kind, n
        lst, self.rows = lc.live_list(kind, n)
        self.glive = None if lst is None else Guarded.of(lst, fill=lc.DEAD, name="live")
        self.gn = None if (lst is not None and n == R) else Guarded.of(np.array([n], np.int32), fill=0, name="n_live")
        self.live = None if self.glive is None else self.glive.ptr
        self.n_live = None if self.gn is None else self.gn.ptr
        self.rows_dev = _dev(self.rows.astype(np.int64))

    def assert_intact(self):
        for g in (self.glive, self.gn):
            if g is not None:
                g.assert_intact()


class _Prof:
    """The launch inside names one (kernel class, tile) row."""
    def __init__(self, gpu, kind, infos, cfg, what):
        self.gpu, self.kind, self.infos, self.cfg, self.what = gpu, kind, infos, cfg, what

    def __enter__(self):
        self.gpu.prof_collect()                                      # (drop what an earlier test may have left pending)
        self.gpu.prof_filter(-1, -1)
        self.gpu.prof_enable(True)

    def __exit__(self, *exc):
        import torch
        self.gpu.prof_enable(False)
        torch.cuda.synchronize()
        rows = self.gpu.prof_collect()
        if exc[0] is None:
            got = [(r["kernel_class"], r["tile_cfg"], r["name"], r["launches"]) for r in rows]
            assert got == [(self.kind, self.cfg, self.infos[self.cfg]["name"], 1)], (self.what, got)


def _plan(infos):
    """(list, count) -> the entries whose counts include it: inputs and images are built once per (list, count)."""
    plan = {}
    for i, t in enumerate(infos):
        for n in lc.counts(t["rows"]):
            for kind in lc.LISTS:
                plan.setdefault((kind, n), []).append(i)
    return sorted(plan.items())


def _record(table, path, infos, ran):
    """On record (run with -s): the names of the entries whose live-row form ran."""
    names = sorted({infos[i]["name"] for i in ran})
    print(f"\nlive-row forms launched, {table} / {path}: {len(names)} tiles: {', '.join(names)}")


# ---------------------------------------------------------------------------------------------------------------- store tiles
@pytest.mark.parametrize("path", list(lc.STORE_SHAPES))
def test_store_tiles(gpu, oracle, path):
    import torch
    import s2vt_amd
    from s2vt_amd import _lib
    from guardband import Guarded
    L = s2vt_amd.lib()
    infos = _entries(gpu, STORE)
    vector = path != "scalar"
    lead, pad = (64, 4) if vector else (65, 0)                       # scalar: every operand 4 bytes off a 16-byte boundary
    clean = lc.store_clean(path)
    k0, k1, k2 = clean["k"]
    N = clean["N"]
    dW, dbias = _dev(clean["W"]), _dev(clean["bias"])
    tail = lambda ld: 64 + (lc.EXTRA + 1) * ld                       # a launch that ignored the clamp would still stay inside the allocation
    gC = Guarded(R, N, ld=N + pad, lead=lead, tail=tail(N + pad), name="C")
    ran = set()
    for (kind, n), entries in _plan(infos):
        ls = _Lists(kind, n)
        c = lc.store_inputs(path, ls.rows)
        gA0 = Guarded.of(c["A0"], ld=k0 + pad, lead=lead, name="A0")
        gTab = Guarded.of(c["Tab"], ld=k1 + pad, lead=lead, name="Tab")
        gidx = Guarded.of(c["idx"], fill=lc.STORE_TABLE - 1, name="rowidx")
        gA2 = Guarded.of(c["A2"], ld=k2 + pad, lead=lead, tail=tail(k2 + pad), name="A2")
        gCi = Guarded.of(c["Cinit"], ld=N + pad, lead=lead, tail=tail(N + pad), name="Cinit")
        assert all(g.aligned16 == vector for g in (gA0, gTab, gA2, gCi, gC))
        segs = (_lib.Operand * 3)(_lib.Operand(gA0.view.data_ptr(), None, gA0.ld, k0, lc.STORE_MOD, 0),
                                  _lib.Operand(gTab.view.data_ptr(), gidx.view.data_ptr(), gTab.ld, k1, 0, 0),
                                  _lib.Operand(gA2.view.data_ptr(), None, gA2.ld, k2, 0, 0))
        # the dense twin's operands: the same rows gathered on the host, three plain segments
        live = ls.rows
        dense = None
        if len(live):
            dense = ([gpu.operand(_dev(clean["A0"][live % lc.STORE_MOD])), gpu.operand(_dev(clean["Tab"][clean["idx"][live]])),
                      gpu.operand(_dev(clean["A2"][live]))], _dev(clean["Cinit"][live]))
        for variant in lc.STORE_VARIANTS:
            if variant.endswith("tanh") and (kind, n) != ("holes", 1):       # act_tanh once per entry: every entry has the count 1
                continue
            img = gC.image(live, lc.store_expected(oracle, path, variant)["C"][live])
            bias = None if variant == "nobias" else dbias
            for i in entries:
                what = (path, variant, kind, n, infos[i]["name"])
                run = _takes_the_launch(infos, i, vector)
                gC.reset()
                with _Prof(gpu, STORE, infos, run, what):
                    rc = L.s2vt_gemm_live(segs, 3, _ptr(dW), N, _ptr(bias), gCi.ptr, gCi.ld, gC.ptr, gC.ld, R, N, int(variant.endswith("tanh")),
                                          ls.live, ls.n_live, i, _stream())
                    assert rc == 0, what
                gC.assert_image(img, what)
                ran.add(run)
                if dense is not None:
                    C2 = gpu.gemm(dense[0], dW, bias, M=len(live), cinit=dense[1], act_tanh=variant.endswith("tanh"), tile_cfg=i)
                    assert torch.equal(C2, gC.view[ls.rows_dev]), what
        for g in (gA0, gTab, gidx, gA2, gCi):
            g.assert_intact()
        ls.assert_intact()
    assert ran == {i for i, t in enumerate(infos) if t["has_live"] and (vector or t["has_scalar"])}, "every entry with a live-row form of this path ran it"
    _record("store", path, infos, ran)


# ---------------------------------------------------------------------------------------------------------------- cell-step tiles
@pytest.mark.parametrize("keep,residual", lc.CELL_VARIANTS)
@pytest.mark.parametrize("path", list(lc.CELL_SHAPES))
def test_cell_tiles(gpu, oracle, path, keep, residual):
    """x per row; the state and the residual operand of B videos broadcast (state_rowmod = B, res rowmod = B), as the sampler's first decode
    step has them; the noise ids read through the list, so that the mask is the oracle's for the caller's row."""
    import torch
    import s2vt_amd
    from s2vt_amd import _lib
    from guardband import Guarded
    L = s2vt_amd.lib()
    infos = _entries(gpu, LSTM)
    vector = path != "scalar"
    lead, pad = (64, 4) if vector else (65, 0)
    clean = lc.cell_clean(path)
    E, H, B = clean["E"], clean["H"], lc.B
    dW, db = _dev(clean["W"]), _dev(clean["b"])
    exp = lc.cell_expected(oracle, path, keep, residual)
    outs = {name: Guarded(R, w, lead=64 if vector else 65, tail=64 + (lc.EXTRA + 1) * w, name=name)
            for name, w in (("c_new", H), ("h_new", H), ("out", H), ("gates", 4 * H))}
    ran = set()
    for (kind, n), entries in _plan(infos):
        ls = _Lists(kind, n)
        c = lc.cell_inputs(path, ls.rows)
        gx = Guarded.of(c["x"], ld=E + pad, lead=lead, tail=64 + (lc.EXTRA + 1) * (E + pad), name="x")
        gh, gc = Guarded.of(c["h"], name="h_prev"), Guarded.of(c["c"], name="c_prev")
        gres = Guarded.of(c["res"], ld=H + pad, lead=lead, name="res")
        gvid, gsid = Guarded.of(c["vid"], fill=lc.POISON_ID, name="video_id"), Guarded.of(c["sid"], fill=lc.POISON_ID, name="sample_id")
        assert gx.aligned16 == vector
        x0 = _lib.Operand(gx.view.data_ptr(), None, gx.ld, E, 0, 0)
        res = _lib.Operand(gres.view.data_ptr(), None, gres.ld, H, B, 0)
        live = ls.rows
        imgs = {name: g.image(live, exp[name][live]) for name, g in outs.items()}
        dense = None
        if len(live):                                                    # the dense twin's operands: the same rows gathered on the host
            dense = dict(x=gpu.operand(_dev(clean["x"][live])), h=_dev(clean["h"][live % B]), c=_dev(clean["c"][live % B]),
                         vid=_dev(clean["vid"][live]), sid=_dev(clean["sid"][live]), res=gpu.operand(_dev(clean["res"][live % B])) if residual else None)
        for i in entries:
            what = (path, keep, residual, kind, n, infos[i]["name"])
            run = _takes_the_launch(infos, i, vector)
            for g in outs.values():
                g.reset()
            with _Prof(gpu, LSTM, infos, run, what):
                rc = L.s2vt_lstm_cell_fwd_live(ctypes.byref(x0), None, gh.ptr, gc.ptr, B, _ptr(dW), _ptr(db), ctypes.byref(res) if residual else None,
                                               outs["c_new"].ptr, outs["h_new"].ptr, outs["out"].ptr, outs["gates"].ptr, R, H, float(keep),
                                               lc.DROP_SEED, gvid.ptr, gsid.ptr, lc.DROP_CODE, ls.live, ls.n_live, i, _stream())
                assert rc == 0, what
            for name, g in outs.items():
                g.assert_image(imgs[name], what)
            ran.add(run)
            if dense is not None:
                d = gpu.lstm_cell_fwd(dense["x"], None, dense["h"], dense["c"], dW, db, len(live), keep=keep, seed=lc.DROP_SEED, video_id=dense["vid"],
                                      sample_id=dense["sid"], drop_code=lc.DROP_CODE, want_gates=True, tile_cfg=i, res=dense["res"])
                for name, t in zip(("c_new", "h_new", "out", "gates"), d):
                    assert torch.equal(t, outs[name].view[ls.rows_dev]), (what, name)
        for g in (gx, gh, gc, gres, gvid, gsid):
            g.assert_intact()
        ls.assert_intact()
    assert ran == {i for i, t in enumerate(infos) if t["has_live"] and (vector or t["has_scalar"])}, "every entry with a live-row form of this path ran it"
    _record("cell" + (" (residual)" if residual else ""), path, infos, ran)


# ---------------------------------------------------------------------------------------------------------------- pick tiles
@pytest.mark.parametrize("stride", [1, 16])
@pytest.mark.parametrize("path", list(lc.PICK_SHAPES))
def test_pick_tiles(gpu, oracle, path, stride):
    """The packed words of the live rows are zero on entry and decode to the oracle's tokens (the tie row: the lowest index; the row of
    all-negative logits beats the zero word); the words of every other row keep their sentinel; greedy rows and sampled rows."""
    import torch
    import s2vt_amd
    from guardband import Guarded
    L = s2vt_amd.lib()
    infos = _entries(gpu, PICK)
    vector = path != "scalar"
    lead, pad = (64, 4) if vector else (65, 0)
    clean = lc.pick_clean(path)
    H, V = clean["H"], clean["V"]
    dW, db = _dev(clean["W"]), _dev(clean["b"])
    exp = lc.pick_expected(oracle, path)
    glog = Guarded(R, V, lead=lead, tail=64 + (lc.EXTRA + 1) * V, name="logits_out")
    gpk = Guarded(R, 1, ld=stride, dtype=torch.int64, tail=64 + (lc.EXTRA + 1) * stride, name="packed")
    ran = set()
    for (kind, n), entries in _plan(infos):
        ls = _Lists(kind, n)
        c = lc.pick_inputs(path, ls.rows)
        go2 = Guarded.of(c["o2"], ld=H + pad, lead=lead, tail=64 + (lc.EXTRA + 1) * (H + pad), name="out2")
        gvid, gsid = Guarded.of(c["vid"], fill=lc.POISON_ID, name="video_id"), Guarded.of(c["sid"], fill=lc.POISON_ID, name="sample_id")
        assert go2.aligned16 == vector
        live = ls.rows
        img_log = glog.image(live, exp["logits"][live])
        img_zero = gpk.image(live, np.zeros(len(live), np.int64))
        dense = None
        if len(live):
            dense = (_dev(clean["o2"][live]), _dev(clean["vid"][live]), _dev(clean["sid"][live]))
            assert {lc.TIE_ROW, lc.NEG_ROW} <= set(live.tolist()) or n < 3
        for i in entries:
            what = (path, stride, kind, n, infos[i]["name"])
            run = _takes_the_launch(infos, i, vector)
            glog.reset()
            gpk.reset()
            gpk.view[ls.rows_dev] = 0
            gpk.assert_image(img_zero, what)
            with _Prof(gpu, PICK, infos, run, what):
                rc = L.s2vt_vocab_pick_live(go2.ptr, go2.ld, _ptr(dW), _ptr(db), R, H, V, gvid.ptr, gsid.ptr, lc.PICK_STEP, lc.PICK_SEED, gpk.ptr, stride,
                                            glog.ptr, ls.live, ls.n_live, i, _stream())
                assert rc == 0, what
            glog.assert_image(img_log, what)
            words = gpk.view[ls.rows_dev, 0]
            tokens = (~words & 0xFFFFFFFF).to(torch.int32).cpu().numpy()
            assert np.array_equal(tokens, exp["token"][live]), what
            # every other word, pad and guard: unchanged (the image of the live rows' own words)
            gpk.assert_image(gpk.image(live, words.cpu().numpy()), what)
            ran.add(run)
            if dense is not None:
                tok2, log2, pk2 = gpu.vocab_pick(dense[0], dW, db, dense[1], dense[2], lc.PICK_STEP, lc.PICK_SEED, want_logits=True, tile_cfg=i)
                assert torch.equal(pk2, words) and torch.equal(log2, glog.view[ls.rows_dev]), what
        for g in (go2, gvid, gsid):
            g.assert_intact()
        ls.assert_intact()
    assert ran == {i for i, t in enumerate(infos) if t["has_live"] and (vector or t["has_scalar"])}, "every entry with a live-row form of this path ran it"
    _record("pick", f"{path}, stride {stride}", infos, ran)


# ---------------------------------------------------------------------------------------------------------------- the 2 GiB window
# The vector path addresses every operand by 32-bit byte offsets from a base (raw-buffer loads: an offset of 2 GiB or more returns zeros
# without touching memory).  A plain segment is addressed from the first row of the TILE, so can_vec bounds it by 256 rows -- but under a
# row list it is addressed from the operand's base by the caller's row (gemm_mfma.h seg_base / row_offsets), and the offsets span all M
# rows.  In both tests every address the vector path can form, at most 2 GiB from the base, lies inside the allocation.
def _gemm_live_rows(gpu, oracle, M, ld, rows, mapped):
    import torch
    from guardband import Guarded
    K, N = 64, 128
    rng = np.random.default_rng(5)
    A = rng.standard_normal((M, K)).astype(np.float32); W = rng.standard_normal((K, N)).astype(np.float32)
    big = torch.empty(M * ld, dtype=torch.float32, device="cuda")
    assert big.numel() * 4 > (1 << 31)
    view = big.view(M, ld)[:, :K]
    view.copy_(torch.as_tensor(A))
    ref = oracle.gemm_chain(A, W)
    gC = Guarded(M, N, name="C")
    rows = np.asarray(rows, np.int32)
    live = Guarded.of(rows, fill=0, name="live") if mapped else None
    n_live = Guarded.of(np.array([len(rows)], np.int32), fill=0, name="n_live")
    assert mapped or np.array_equal(rows, np.arange(len(rows)))
    gpu.gemm_live([gpu.operand(view)], _dev(W), gC.view, live=None if live is None else live.view.reshape(-1), n_live=n_live.view.reshape(-1))
    got = gC.numpy()
    for r in rows:
        assert np.array_equal(got[r], ref[r]), f"row {r} (starts at byte {4 * int(r) * ld:#x}): {'all zeros' if not got[r].any() else 'differs'}"
    gC.assert_image(gC.image(rows, ref[rows]))


@pytest.mark.parametrize("mapped", [True, False])
def test_plain_operand_beyond_the_2gib_window(gpu, oracle, mapped):
    """The operand of test_gpu_fwd.py::test_operand_beyond_the_2gib_window_uses_the_scalar_path (3 rows 2^28 floats apart: row 2 starts at
    byte 2^31, a 3 GiB allocation) through the live-row form, with the list [0, 1, 2] and with the count alone.  256 rows of this operand
    reach far beyond 2 GiB, so can_vec's per-tile bound already sends it to the scalar path, with or without a list."""
    _gemm_live_rows(gpu, oracle, 3, 1 << 28, [0, 1, 2], mapped)


@pytest.mark.parametrize("mapped", [True, False])
def test_plain_operand_of_many_rows_beyond_the_2gib_window(gpu, oracle, mapped):
    """300 rows 2^21 - 4 floats apart (a 2.5 GB allocation): 256 rows stay 4 KiB short of 2 GiB, so the dense call and the count-only
    launch (tile-relative addresses) keep the vector path; row 256 starts 4 KiB short of byte 2^31 and row 257 behind it.
    Under a list the offsets are taken from the operand's base: the launch must take the scalar path, or rows 257 and 299 read zeros."""
    M, ld = 300, (1 << 21) - 4
    assert 256 * ld * 4 < (1 << 31) <= 257 * ld * 4
    _gemm_live_rows(gpu, oracle, M, ld, [1, 255, 256, 257, 299] if mapped else np.arange(M), mapped)
