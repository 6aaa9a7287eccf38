"""The host-composable single-op entry points of include/s2vt.h, each at the sizes where its kernel changes course (one element,
odd sizes, a tile or slab boundary, more than one block, a grid-stride loop) and with row strides wider than the rows, inside guard
bands (tests/guardband.py): s2vt_transpose, s2vt_colsum, s2vt_tanh_bwd, s2vt_embed_gather, s2vt_embed_scatter_add,
s2vt_lstm_cell_bwd, s2vt_frame_embed_bwd, s2vt_grad_finalize / s2vt_adam_tf / s2vt_global_norm_clip, and the refusals their entry
points make on the host.  References are float64 (numpy / torch autograd), or plain fp32 numpy where the contract is bit-exactness."""
import ctypes as C

import numpy as np
import pytest

from guardband import Guarded

pytestmark = pytest.mark.gpu


def _lib():
    import s2vt_amd
    return s2vt_amd.lib()


def _intact(*gs):
    for g in gs:
        g.assert_intact()


# ---------------------------------------------------------------------------------------------------- transpose
@pytest.mark.parametrize("R,Cc,ldi,ldo", [(1, 1, 1, 1), (1, 33, 33, 1), (31, 33, 40, 35), (32, 32, 32, 32), (33, 65, 65, 33), (100, 7, 8, 101)])
def test_transpose_bit_exact(gpu, R, Cc, ldi, ldo):
    rng = np.random.default_rng(R * 100 + Cc)
    x = rng.standard_normal((R, Cc)).astype(np.float32)
    gin, out = Guarded.of(x, ld=ldi, name="in"), Guarded(Cc, R, ld=ldo, name="out")
    assert _lib().s2vt_transpose(gin.ptr, ldi, out.ptr, ldo, R, Cc, gpu._stream()) == 0
    assert np.array_equal(out.bits(), np.ascontiguousarray(x.T).view(np.int32))
    _intact(gin, out)


# ---------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("M,N,ld", [(1, 1, 1), (3, 63, 63), (255, 64, 70), (256, 65, 65), (257, 130, 130), (1030, 5, 8)])
def test_colsum_accumulates(gpu, M, N, ld):
    """out[n] += sum_m X[m, n] into an `out` that does not start from zero (up to 256 rows only that start tells += from =)."""
    rng = np.random.default_rng(M * 7 + N)
    x = rng.standard_normal((M, N)).astype(np.float32)
    out0 = rng.standard_normal(N).astype(np.float32)
    gx, out = Guarded.of(x, ld=ld, name="X"), Guarded.of(out0, name="out")
    assert _lib().s2vt_colsum(gx.ptr, ld, M, N, out.ptr, gpu._stream()) == 0
    ref = out0.astype(np.float64) + x.astype(np.float64).sum(0)
    err = float(np.abs(out.numpy()[0].astype(np.float64) - ref).max())
    bound = 1e-6 * float(np.abs(x.astype(np.float64)).sum(0).max() + np.abs(out0).max())
    print(f"\ncolsum {M}x{N} ld={ld}: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    _intact(gx, out)


# ---------------------------------------------------------------------------------------------------- tanh backward
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_tanh_bwd_bit_exact(gpu, n):
    rng = np.random.default_rng(n)
    y = np.tanh(rng.standard_normal(n) * 2).astype(np.float32)
    y[::5] = np.float32([0.0, 1.0, -1.0, 0.5, -0.0])[np.arange(len(y[::5])) % 5]
    dy = rng.standard_normal(n).astype(np.float32)
    gy, gdy, dx = Guarded.of(y, name="y"), Guarded.of(dy, name="dy"), Guarded(1, n, name="dx")
    assert _lib().s2vt_tanh_bwd(gy.ptr, gdy.ptr, dx.ptr, n, gpu._stream()) == 0
    yy = y * y                                                       # fp32 step by step: the library is built without contraction
    want = dy * (np.float32(1.0) - yy)
    assert want.dtype == np.float32 and np.array_equal(dx.bits()[0], want.view(np.int32))
    _intact(gy, gdy, dx)


# ---------------------------------------------------------------------------------------------------- embedding rows
@pytest.mark.parametrize("R,E,ldw,ldo", [(1, 1, 1, 1), (5, 3, 3, 5), (33, 12, 12, 12), (6, 500, 504, 500), (9, 65, 70, 67)])
def test_embed_gather_bit_exact(gpu, R, E, ldw, ldo):
    import torch
    rng = np.random.default_rng(R * 1000 + E)
    nrow = 11
    W = rng.standard_normal((nrow, E)).astype(np.float32)
    idx = rng.integers(0, nrow, R).astype(np.int32)
    idx[0] = nrow - 1                                                # the last table row, the first, a repeat
    if R >= 3:
        idx[1], idx[2] = 0, nrow - 1
    gW, gi, out = Guarded.of(W, ld=ldw, name="Wemb"), Guarded.of(idx, name="idx"), Guarded(R, E, ld=ldo, name="out")
    assert _lib().s2vt_embed_gather(gW.ptr, ldw, gi.ptr, R, E, out.ptr, ldo, gpu._stream()) == 0
    assert np.array_equal(out.bits(), W[idx].view(np.int32))
    _intact(gW, gi, out)
    if ldw == E and ldo == E:                                        # the wrapper (contiguous table, its own output)
        got = gpu.embed_gather(torch.as_tensor(W).cuda(), torch.as_tensor(idx).cuda())
        assert np.array_equal(got.cpu().numpy(), W[idx])


@pytest.mark.parametrize("pattern", ["same", "distinct", "mixed"])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 500])
def test_embed_scatter_add(gpu, E, pad, pattern):
    """dWemb[idx[r], :] += dE[r, :] into a table that does not start from zero; rows no index names keep their bits."""
    R, nrow, ld = 37, 41, E + pad
    rng = np.random.default_rng(E * 10 + pad)
    dE = rng.standard_normal((R, E)).astype(np.float32)
    W0 = rng.standard_normal((nrow, E)).astype(np.float32)
    idx = {"same": np.full(R, 17), "distinct": np.append(rng.permutation(nrow - 1)[:R - 1], nrow - 1),      # (with the last table row)
           "mixed": np.append(rng.integers(0, 5, R - 1) * 8, nrow - 1)}[pattern].astype(np.int32)
    assert len(np.unique(idx)) == {"same": 1, "distinct": R}.get(pattern, len(np.unique(idx))) and idx.max() < nrow
    gE, gi, gW = Guarded.of(dE, ld=ld, name="dE"), Guarded.of(idx, name="idx"), Guarded.of(W0, name="dWemb")
    gpu.embed_scatter_add(gE.view, gi.view[0], gW.view)
    ref = W0.astype(np.float64)
    mag = np.abs(W0).astype(np.float64)
    np.add.at(ref, idx, dE.astype(np.float64))
    np.add.at(mag, idx, np.abs(dE).astype(np.float64))
    got = gW.numpy()
    err = np.abs(got.astype(np.float64) - ref)
    print(f"\nscatter_add E={E} ld={ld} {pattern}: max err / bound {float((err / (1e-6 * mag)).max()):.3f}")
    assert (err <= 1e-6 * mag).all()                                 # per element: sum of |terms| + |initial|
    untouched = np.setdiff1d(np.arange(nrow), idx)
    assert len(untouched) and np.array_equal(got[untouched].view(np.int32), W0[untouched].view(np.int32))
    _intact(gE, gi, gW)


# ---------------------------------------------------------------------------------------------------- LSTM cell backward
@pytest.mark.parametrize("with_dc_in", [False, True])
@pytest.mark.parametrize("M,H,scale", [(1, 1, 1.0), (3, 5, 1.0), (7, 20, 1.0), (5, 64, 1.0), (2, 1000, 1.0), (7, 20, 30.0)])
def test_lstm_cell_bwd_vs_autograd(gpu, M, H, scale, with_dc_in):
    """dz, dc_prev against float64 autograd of the BasicLSTMCell pointwise part (scale 30: saturated gates)."""
    import torch
    torch.manual_seed(M * 1000 + H)
    z = (torch.randn(M, 4 * H, dtype=torch.float64) * scale).requires_grad_()
    c = torch.randn(M, H, dtype=torch.float64).requires_grad_()
    i, j, f, o = z.split(H, 1)
    si, tj, sf, so = torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + 1.0), torch.sigmoid(o)
    c_new = c * sf + si * tj
    h_new = torch.tanh(c_new) * so
    dh = torch.randn(M, H, dtype=torch.float64); dc_in = torch.randn(M, H, dtype=torch.float64)
    obj = (h_new * dh).sum() + ((c_new * dc_in).sum() if with_dc_in else 0.0)
    dz_ref, dc_ref = torch.autograd.grad(obj, [z, c])
    f32 = lambda t: t.detach().float().numpy()
    gates = Guarded.of(f32(torch.cat([si, tj, sf, so], 1)), name="gates")
    gcn, gcp, gdh = Guarded.of(f32(c_new), name="c_new"), Guarded.of(f32(c), name="c_prev"), Guarded.of(f32(dh), name="dh")
    gdc = Guarded.of(f32(dc_in), name="dc_in") if with_dc_in else None
    dz, dcp = Guarded(M, 4 * H, name="dz"), Guarded(M, H, name="dc_prev")
    rc = _lib().s2vt_lstm_cell_bwd(gates.ptr, gcn.ptr, gcp.ptr, gdh.ptr, None if gdc is None else gdc.ptr, dz.ptr, dcp.ptr, M, H, gpu._stream())
    assert rc == 0
    for name, got, ref in (("dz", dz.numpy(), dz_ref.numpy()), ("dc_prev", dcp.numpy(), dc_ref.numpy())):
        err = np.abs(got - ref)
        print(f"\nlstm_cell_bwd M={M} H={H} x{scale} dc_in={with_dc_in}: {name} max err {float(err.max()):.3e}, "
              f"{float((err / (2e-5 + 2e-4 * np.abs(ref))).max()):.3f} of bound")
        assert np.allclose(got, ref, rtol=2e-4, atol=2e-5), name
    _intact(gates, gcn, gcp, gdh, dz, dcp, *(() if gdc is None else (gdc,)))


# ---------------------------------------------------------------------------------------------------- frame embedding backward
@pytest.mark.parametrize("B,Tv,D,E", [(4, 3, 24, 12), (3, 5, 130, 36)])
def test_frame_embed_bwd_accumulates(gpu, B, Tv, D, E):
    """d_encode_image_W += video^T d_emb and d_encode_image_b += colsum(d_emb), both into non-zero starts."""
    rng = np.random.default_rng(D)
    dims = gpu.make_dims(D, 97, E, 20, Tv, 6)
    video = rng.standard_normal((B * Tv, D)); demb = rng.standard_normal((B * Tv, E))
    dW0 = rng.standard_normal((D, E)).astype(np.float32); db0 = rng.standard_normal(E).astype(np.float32)
    gv, gd = Guarded.of(video.astype(np.float32), name="video"), Guarded.of(demb.astype(np.float32), name="d_emb")
    gW, gb = Guarded.of(dW0, name="d_encode_image_W"), Guarded.of(db0, name="d_encode_image_b")
    assert _lib().s2vt_frame_embed_bwd(C.byref(dims), gv.ptr, gd.ptr, B, gW.ptr, gb.ptr, gpu._stream()) == 0
    v64, d64 = video.astype(np.float32).astype(np.float64), demb.astype(np.float32).astype(np.float64)
    refW, refb = dW0 + v64.T @ d64, db0 + d64.sum(0)
    print(f"\nframe_embed_bwd B={B} Tv={Tv} D={D} E={E}: dW max err {float(np.abs(gW.numpy() - refW).max()):.3e}, "
          f"db max err {float(np.abs(gb.numpy()[0] - refb).max()):.3e} (atol 1e-4 + rtol 1e-4)")
    assert np.allclose(gW.numpy(), refW, rtol=1e-4, atol=1e-4)
    assert np.allclose(gb.numpy()[0], refb, rtol=1e-4, atol=1e-4)
    _intact(gv, gd, gW, gb)


# ---------------------------------------------------------------------------------------------------- clip + Adam
SIZES = [1, 3, 4, 5, 1023, 524288 + 5, 1048576 + 7]                 # the last two exceed 2048 x 256 and 4096 x 256: grid-stride loops


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_grad_finalize_and_adam_tf_three_steps(gpu, n, misaligned):
    """g <- g * gscale + wd * theta with sum g^2, then clip_by_global_norm + TF-form Adam, against float64 (oracle/s2vt_torch.py) over
    three steps: the first and third below the clip norm, the second above it; without and with (weight decay, gscale).
    The clip norm is 0.05 sqrt(n), so that a clipped element is 0.05 rms and at most about 0.25 at every size.  That scale is what
    m's absolute bound of 1e-7 asks for: the clip factor carries the rounding of sum g^2, which is accumulated from up to 2048 block
    partials by fp32 atomics -- about sqrt(2048) 2^-24 = 3e-6 relative at worst, half of it in the factor -- and it enters m as
    0.1 |g| times that error, also where m itself cancels to nothing: 0.1 x 0.25 x 1.5e-6 = 4e-8.  (With a clip norm of sqrt(n),
    elements up to 5, the same arithmetic measured 0.9 to 1.4 of the bound at n >= 2^19.)"""
    import torch
    from oracle import s2vt_torch as T
    L = _lib()
    lead = 65 if misaligned else 64
    unit = 0.05
    clip, lr = unit * float(np.sqrt(n)), 1e-3
    for wd, gs in ((0.0, None), (1e-3, 0.5)):
        rng = np.random.default_rng(n + int(gs is not None))
        theta0 = rng.standard_normal(n).astype(np.float32)
        pt = {"w": torch.tensor(theta0, dtype=torch.float64)}
        mt = {"w": torch.zeros(n, dtype=torch.float64)}; vt = {"w": torch.zeros(n, dtype=torch.float64)}
        th, m, v = Guarded.of(theta0, lead=lead, name="theta"), Guarded.of(np.zeros(n, np.float32), lead=lead, name="m"), \
            Guarded.of(np.zeros(n, np.float32), lead=lead, name="v")
        g = Guarded(1, n, lead=lead, name="g")
        sumsq, applied = Guarded.of(np.zeros(1, np.float32), name="sumsq"), Guarded.of(np.zeros(1, np.int32), name="applied_step")
        gscale = None if gs is None else Guarded.of(np.float32([gs]), name="gscale")
        assert th.aligned16 != misaligned and g.aligned16 != misaligned
        worst = {}
        for step in (1, 2, 3):
            rms = unit * (3.0 if step == 2 else 0.5)                 # |g| = rms * sqrt(n) against clip = unit * sqrt(n)
            g0 = (rng.standard_normal(n) * rms / (gs or 1.0)).astype(np.float32)
            if n <= 5:
                g0 = (np.sign(g0) * rms / (gs or 1.0) * rng.uniform(0.9, 1.1, n)).astype(np.float32)      # few elements: fix the norm's side
            gfin = torch.tensor(g0, dtype=torch.float64) * (gs or 1.0) + wd * pt["w"]
            gt, nrm = T.clip_by_global_norm({"w": gfin}, clip)
            assert (nrm > clip) == (step == 2)
            pt, mt, vt = T.adam_tf(pt, gt, mt, vt, step, lr)
            g.fill(g0); sumsq.fill(np.zeros(1, np.float32))
            assert L.s2vt_grad_finalize(g.ptr, th.ptr, n, None if gscale is None else gscale.ptr, wd, sumsq.ptr, gpu._stream()) == 0
            ss = float(sumsq.numpy()[0, 0])
            assert abs(ss - nrm ** 2) <= 1e-4 * nrm ** 2, (step, ss, nrm ** 2)
            # two fp32 roundings, of g * gscale and of the sum: 2^-23 of the larger term (|wd * theta| << 1) bounds both
            assert np.allclose(g.numpy()[0], gfin.numpy(), rtol=1e-6, atol=1e-7)
            assert L.s2vt_adam_tf_guarded(th.ptr, g.ptr, m.ptr, v.ptr, n, sumsq.ptr, clip, lr, step, 0.9, 0.999, 1e-8, applied.ptr,
                                          gpu._stream()) == 0
            assert int(applied.numpy()[0, 0]) == step
            for name, got, ref, rtol, atol in (("theta", th, pt, 2e-5, 2e-6), ("m", m, mt, 1e-4, 1e-7), ("v", v, vt, 1e-4, 1e-7)):
                r = ref["w"].numpy()
                frac = float((np.abs(got.numpy()[0] - r) / (atol + rtol * np.abs(r))).max())
                worst[name] = max(worst.get(name, 0.0), frac)
                assert frac <= 1.0, (name, step, frac)
        print(f"\nclip+adam n={n} misaligned={misaligned} wd={wd} gscale={gs}: max err / bound " + ", ".join(f"{k} {f:.3f}" for k, f in worst.items()))
        _intact(th, m, v, g, sumsq, applied, *(() if gscale is None else (gscale,)))


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_global_norm_clip(gpu, n, misaligned):
    """s2vt_global_norm_clip below and above the norm: ||g||^2 and g * clip / max(||g||, clip), the bounds of
    test_gpu_session.py::test_embed_gather_and_clip."""
    lead = 65 if misaligned else 64
    clip = float(np.sqrt(n))
    rng = np.random.default_rng(n)
    for rms in (0.5, 3.0):
        g0 = (rng.standard_normal(n) * rms).astype(np.float32)
        if n <= 5:
            g0 = (np.sign(g0) * rms * rng.uniform(0.9, 1.1, n)).astype(np.float32)
        g, ss = Guarded.of(g0, lead=lead, name="g"), Guarded(1, 1, name="sumsq")
        assert _lib().s2vt_global_norm_clip(g.ptr, n, clip, ss.ptr, gpu._stream()) == 0
        nrm = float(np.sqrt((g0.astype(np.float64) ** 2).sum()))
        assert (nrm > clip) == (rms > 1)
        assert abs(float(ss.numpy()[0, 0]) - nrm ** 2) <= 1e-4 * nrm ** 2
        assert np.allclose(g.numpy()[0].astype(np.float64), g0.astype(np.float64) * (clip / max(nrm, clip)), rtol=1e-5, atol=1e-7)
        _intact(g, ss)


# ---------------------------------------------------------------------------------------------------- refusals
def test_host_side_refusals(gpu):
    """Preconditions each entry point checks on the host before any launch (session.hip / train.hip, the first line of each): an
    error, and the outputs -- window and guards -- keep what they held."""
    import torch
    L = _lib()
    st = gpu._stream()
    E = 8
    W, idx = Guarded.of(np.ones((5, E), np.float32), ld=E, name="Wemb"), Guarded.of(np.zeros(3, np.int32), name="idx")
    out = Guarded.of(np.zeros((3, E), np.float32), ld=E, name="out")
    assert L.s2vt_embed_gather(W.ptr, E - 1, idx.ptr, 3, E, out.ptr, E, st) == -1                   # ldw < E
    assert L.s2vt_embed_gather(W.ptr, E, idx.ptr, 3, E, out.ptr, E - 1, st) == -1                   # ldo < E
    dE, tab = Guarded.of(np.ones((3, E), np.float32), name="dE"), Guarded.of(np.zeros((5, E), np.float32), name="dWemb")
    assert L.s2vt_embed_scatter_add(dE.ptr, E - 1, idx.ptr, 3, E, tab.ptr, st) == -1                # ld < E
    dout, dh = Guarded.of(np.ones((3, E), np.float32), name="dout"), Guarded.of(np.zeros((3, E), np.float32), name="dh")
    assert L.s2vt_dropout_bwd(dout.ptr, E - 1, dh.ptr, 3, E, 1.0, 0, 0, None, None, st) == -1       # ld < H
    assert L.s2vt_dropout_bwd(dout.ptr, E, dh.ptr, 3, E, 0.0, 0, 0, idx.ptr, idx.ptr, st) == -1     # keep = 0
    g, ss = Guarded.of(np.ones(16, np.float32), name="g"), Guarded.of(np.zeros(1, np.float32), name="sumsq")
    assert L.s2vt_global_norm_clip(g.ptr, 16, 0.0, ss.ptr, st) == -1                                # clip_norm <= 0
    assert L.s2vt_global_norm_clip(g.ptr, 16, -1.0, ss.ptr, st) == -1
    torch.cuda.synchronize()
    for x in (out, tab, dh, ss):
        assert not x.bits().any(), x.name
    assert np.array_equal(g.numpy(), np.ones((1, 16), np.float32))
    _intact(W, idx, out, dE, tab, dout, dh, g, ss)
