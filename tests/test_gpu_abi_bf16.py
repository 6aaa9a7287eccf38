"""The bf16 and split-bf16 gradient products and their casts through the C ABI inside guard bands (tests/guardband.py):
s2vt_gemm_bf16_nt (both MFMA shapes), s2vt_gemm_bf16x3_nt, s2vt_gemm_bf16x3_tn (with and without the bias row), s2vt_cast_bf16 and
s2vt_cast_bf16_split (row and transposed forms).  The products run on planes with row strides wider than the rows (NT: lda = Kp + 8,
ldb = Kp + 16; TN: two different multiples of 8) and NaN behind every row and behind the last one, into a C with ldc = N + 3 that starts
4 bytes past a 16-byte boundary: within the bounds of test_gpu_bf16_grads.py / test_gpu_split_grads.py / test_gpu_split_fused.py against
float64 on the same bf16 values, and bit for bit what the same call gives on dense, aligned, unguarded tensors (no atomics anywhere).
The casts read a source that is misaligned with ld % 4 == 0 (the scalar branch that `ld & 3` does not reach) or strided, and write
destinations with ldd = Kp + 8: zeros in the pad columns up to Kp, the sentinel beyond.  And the refusals the entry points make on the host."""
import ctypes as C

import numpy as np
import pytest

from guardband import Guarded

pytestmark = pytest.mark.gpu
S2VT_E_BADARG, S2VT_E_ALIGN = -1, -2


def _lib():
    import s2vt_amd
    return s2vt_amd.lib()


def _intact(*gs):
    for g in gs:
        if g is not None:
            g.assert_intact()


def _split(x):
    import torch
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def _pad(n, m):
    return (n + m - 1) // m * m


def _f64(g):
    import torch
    return torch.as_tensor(g.numpy()).double()


def _ktol(K):
    return max(1.0, (K / 1000) ** 0.5)


# ---------------------------------------------------------------------------------------------------- NT products
@pytest.mark.parametrize("Kp", [192, 1088])          # six K steps of 32: the 4-slot ring wraps; 34 K steps: two split-K slabs with a scratch
@pytest.mark.parametrize("M,N", [(129, 130), (1, 1)])
@pytest.mark.parametrize("kernel", ["bf16_nt/16", "bf16_nt/32", "bf16x3_nt", "bf16x3_nt+scratch"])
def test_nt_products_strided_guarded(gpu, kernel, M, N, Kp):
    import torch
    L, st = _lib(), gpu._stream()
    x3 = kernel.startswith("bf16x3")
    with_scratch = kernel.endswith("+scratch")
    g = torch.Generator().manual_seed(M * 31 + N + Kp)
    a, b = torch.randn(M, Kp, generator=g), torch.randn(N, Kp, generator=g)
    C0 = torch.randn(M, N, generator=g)
    lda, ldb, ldc = Kp + 8, Kp + 16, N + 3
    # guards behind row M - 1 / N - 1 one whole 128-row tile deep: a tile that read on would find NaN, inside this allocation
    planes_a = [Guarded.of(p, ld=lda, tail=128 * lda, name=f"A{n}") for p, n in zip(_split(a) if x3 else (a.to(torch.bfloat16),), ("hi", "lo"))]
    planes_b = [Guarded.of(p, ld=ldb, tail=128 * ldb, name=f"B{n}") for p, n in zip(_split(b) if x3 else (b.to(torch.bfloat16),), ("hi", "lo"))]
    da, db = [p.view.double() for p in planes_a], [p.view.double() for p in planes_b]
    ref = (da[0] @ db[0].t() + ((da[0] @ db[1].t() + da[1] @ db[0].t()) if x3 else 0.0)).cpu()
    scale = float(ref.abs().max()) + 1e-30
    rel = 1e-6 * _ktol(Kp) if x3 else 1e-4                                     # test_gemm_bf16x3_vs_float64 / test_gemm_bf16_nt_vs_float64
    out = Guarded(M, N, ld=ldc, lead=65, name="C")
    scratch = Guarded(1, 8 * M * N, name="scratch") if with_scratch else None   # 32 M N bytes: "always suffices"
    assert not out.aligned16 and planes_a[0].aligned16 and planes_b[0].aligned16
    dense_a, dense_b = [p.view.contiguous() for p in planes_a], [p.view.contiguous() for p in planes_b]
    for accumulate in (0, 1):
        out.reset(); out.fill(C0)
        if x3:
            rc = L.s2vt_gemm_bf16x3_nt(planes_a[0].ptr, planes_a[1].ptr, lda, planes_b[0].ptr, planes_b[1].ptr, ldb, out.ptr, ldc, M, N, Kp, accumulate,
                                       None if scratch is None else scratch.ptr, 0 if scratch is None else 32 * M * N, st)
        else:
            rc = L.s2vt_gemm_bf16_nt(planes_a[0].ptr, lda, planes_b[0].ptr, ldb, out.ptr, ldc, M, N, Kp, accumulate, int(kernel[-2:]), st)
        assert rc == 0
        want = ref + C0.double() if accumulate else ref
        bound = rel * (scale + (float(C0.abs().max()) if accumulate else 0.0))
        err = float((_f64(out) - want).abs().max())
        print(f"\n{kernel} {M}x{N}x{Kp} acc={accumulate}: max err {err:.3e}, bound {bound:.3e} ({err / bound:.3f})")
        assert err <= bound
        dense = C0.clone().cuda()                                               # the same product on dense, aligned tensors: the same bits
        if x3:
            gpu.gemm_bf16x3_nt(dense_a[0], dense_a[1], dense_b[0], dense_b[1], out=dense, accumulate=bool(accumulate), split_k=with_scratch)
        else:
            gpu.gemm_bf16_nt(dense_a[0], dense_b[0], out=dense, accumulate=bool(accumulate), mfma=int(kernel[-2:]))
        assert np.array_equal(out.bits(), dense.cpu().numpy().view(np.int32)), accumulate
        _intact(out, scratch)
    if with_scratch and M > 1 and Kp == 1088:
        assert bool((scratch._iview != scratch._sentinel).any()), "two slabs of 17 K steps were expected to pass through the scratch"
    _intact(*planes_a, *planes_b)


# ---------------------------------------------------------------------------------------------------- the K-major product
@pytest.mark.parametrize("K", [165, 1088])           # 165: no multiple of 64, of 32, odd: the descriptor ends behind row 164
@pytest.mark.parametrize("M,N", [(129, 130), (1, 1)])
@pytest.mark.parametrize("with_scratch", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
def test_tn_product_strided_guarded(gpu, with_bias, with_scratch, M, N, K):
    import torch
    L, st = _lib(), gpu._stream()
    g = torch.Generator().manual_seed(M * 17 + N + K)
    a, b = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g)
    C0, bias0 = torch.randn(M, N, generator=g), torch.randn(N, generator=g)
    ah, al = _split(a)
    bh, bl = _split(b)
    if with_bias:                                                               # column M of A: ones in the hi plane, zeros in the lo plane
        ah = torch.cat([ah, torch.ones(K, 1, dtype=torch.bfloat16)], 1)
        al = torch.cat([al, torch.zeros(K, 1, dtype=torch.bfloat16)], 1)
    lda, ldb, ldc = _pad(M + 1, 8) + 8, _pad(N, 8) + 16, N + 3
    assert lda != ldb and lda % 8 == 0 and ldb % 8 == 0
    # s2vt.h: up to (K + 65) ld 2 bytes of a plane and the columns of a row up to the next multiple of 128 may be read: NaN there, too
    gAh, gAl = [Guarded.of(p, ld=lda, tail=65 * lda + 128, name=n) for p, n in ((ah, "Ahi"), (al, "Alo"))]
    gBh, gBl = [Guarded.of(p, ld=ldb, tail=65 * ldb + 128, name=n) for p, n in ((bh, "Bhi"), (bl, "Blo"))]
    A64h, A64l, B64h, B64l = ah[:, :M].double(), al[:, :M].double(), bh.double(), bl.double()
    ref = A64h.t() @ B64h + A64h.t() @ B64l + A64l.t() @ B64h
    ref_bias = bias0.double() + (B64h + B64l).sum(0)
    scale = float(ref.abs().max()) + 1e-30
    tol = 1e-6 * _ktol(K)                                                       # test_gemm_bf16x3_tn_vs_float64_and_nt / _bias_row
    out = Guarded(M, N, ld=ldc, lead=65, name="C")
    gbias = Guarded.of(bias0, lead=65, name="bias") if with_bias else None
    scratch = Guarded(1, 8 * (M + 1) * N, name="scratch") if with_scratch else None
    # the dense call: planes of the smallest legal stride with zeros in their pad columns, plain tensors
    lda0, ldb0 = _pad(M + int(with_bias), 8), _pad(N, 8)
    dA = [torch.zeros(K, lda0, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    dB = [torch.zeros(K, ldb0, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    for d, p in zip(dA + dB, (ah, al, bh, bl)):
        d[:, :p.shape[1]] = p.cuda()
    for accumulate in (0, 1):
        out.reset(); out.fill(C0)
        if gbias is not None:
            gbias.fill(bias0)
        rc = L.s2vt_gemm_bf16x3_tn(gAh.ptr, gAl.ptr, lda, gBh.ptr, gBl.ptr, ldb, out.ptr, ldc, M, N, K, accumulate, None if gbias is None else gbias.ptr,
                                   None if scratch is None else scratch.ptr, 0 if scratch is None else 32 * (M + 1) * N, st)
        assert rc == 0
        want = ref + C0.double() if accumulate else ref
        bound = tol * (scale + (float(C0.abs().max()) if accumulate else 0.0))
        err = float((_f64(out) - want).abs().max())
        print(f"\nbf16x3_tn {M}x{N}x{K} bias={with_bias} scratch={with_scratch} acc={accumulate}: max err {err:.3e}, bound {bound:.3e} ({err / bound:.3f})")
        assert err <= bound
        dense, dbias = C0.clone().cuda(), bias0.clone().cuda() if with_bias else None
        gpu.gemm_bf16x3_tn(dA[0], dA[1], dB[0], dB[1], M, N, out=dense, accumulate=bool(accumulate), split_k=with_scratch, bias=dbias)
        assert np.array_equal(out.bits(), dense.cpu().numpy().view(np.int32)), accumulate
        if with_bias:                                                           # added to bias whatever `accumulate` says
            bscale = float((B64h + B64l).sum(0).abs().max()) + float(bias0.abs().max())
            berr = float((_f64(gbias)[0] - ref_bias).abs().max())
            print(f"   bias row: max err {berr:.3e}, bound {tol * bscale:.3e} ({berr / (tol * bscale):.3f})")
            assert berr <= tol * bscale
            assert np.array_equal(gbias.bits()[0], dbias.cpu().numpy().view(np.int32))
        _intact(out, gbias, scratch)
    if with_scratch and M > 1 and K == 1088:
        assert bool((scratch._iview != scratch._sentinel).any()), "two slabs were expected to pass through the scratch"
    _intact(gAh, gAl, gBh, gBl)


# ---------------------------------------------------------------------------------------------------- refusals
def test_bf16_products_refuse_on_the_host(gpu):
    """A plane pointer 2 bytes off -> S2VT_E_ALIGN; lda & 7, Kp % 64 (NT), ldc < N, lda < M + 1 with a bias (TN) -> S2VT_E_BADARG; each
    before any launch: the guarded C keeps the sentinel everywhere."""
    import torch
    L, st = _lib(), gpu._stream()
    M, N, Kp = 128, 16, 128                                                     # M a multiple of 8: lda == M is a legal stride without a bias
    z = torch.zeros(Kp + 8, Kp + 8, dtype=torch.bfloat16)
    P = [Guarded.of(z, name=f"plane{i}") for i in range(4)]                    # rows and columns to spare in either orientation
    ld = P[0].ld
    out, bias = Guarded(M, N, name="C"), Guarded(1, N, name="bias")
    off = lambda g: C.c_void_p(g.view.data_ptr() + 2)
    p = [g.ptr for g in P]
    B, A = S2VT_E_BADARG, S2VT_E_ALIGN
    nt = lambda a, lda, b, ldb, ldc, kp: L.s2vt_gemm_bf16_nt(a, lda, b, ldb, out.ptr, ldc, M, N, kp, 0, 16, st)
    x3 = lambda ah, al, lda, bh, bl, ldb, ldc, kp: L.s2vt_gemm_bf16x3_nt(ah, al, lda, bh, bl, ldb, out.ptr, ldc, M, N, kp, 0, None, 0, st)
    tn = lambda ah, al, lda, bh, bl, ldb, ldc, bs: L.s2vt_gemm_bf16x3_tn(ah, al, lda, bh, bl, ldb, out.ptr, ldc, M, N, Kp, 0, bs, None, 0, st)
    checks = [
        ("nt A + 2 bytes", nt(off(P[0]), ld, p[1], ld, N, Kp), A), ("nt B + 2 bytes", nt(p[0], ld, off(P[1]), ld, N, Kp), A),
        ("nt lda & 7", nt(p[0], Kp + 4, p[1], ld, N, Kp), B), ("nt ldb & 7", nt(p[0], ld, p[1], Kp + 4, N, Kp), B),
        ("nt Kp % 64", nt(p[0], ld, p[1], ld, N, 96), B), ("nt ldc < N", nt(p[0], ld, p[1], ld, N - 1, Kp), B),
        ("x3 Ah + 2 bytes", x3(off(P[0]), p[1], ld, p[2], p[3], ld, N, Kp), A), ("x3 Al + 2 bytes", x3(p[0], off(P[1]), ld, p[2], p[3], ld, N, Kp), A),
        ("x3 Bh + 2 bytes", x3(p[0], p[1], ld, off(P[2]), p[3], ld, N, Kp), A), ("x3 Bl + 2 bytes", x3(p[0], p[1], ld, p[2], off(P[3]), ld, N, Kp), A),
        ("x3 lda & 7", x3(p[0], p[1], Kp + 4, p[2], p[3], ld, N, Kp), B), ("x3 Kp % 64", x3(p[0], p[1], ld, p[2], p[3], ld, N, 96), B),
        ("x3 ldc < N", x3(p[0], p[1], ld, p[2], p[3], ld, N - 1, Kp), B),
        ("tn Ah + 2 bytes", tn(off(P[0]), p[1], ld, p[2], p[3], ld, N, None), A), ("tn Bl + 2 bytes", tn(p[0], p[1], ld, p[2], off(P[3]), ld, N, None), A),
        ("tn lda & 7", tn(p[0], p[1], M + 4, p[2], p[3], ld, N, None), B), ("tn ldb & 7", tn(p[0], p[1], ld, p[2], p[3], N + 4, N, None), B),
        ("tn ldc < N", tn(p[0], p[1], ld, p[2], p[3], ld, N - 1, None), B),
        ("tn lda < M + 1 with a bias", tn(p[0], p[1], M, p[2], p[3], ld, N, bias.ptr), B),
    ]
    torch.cuda.synchronize()
    for what, rc, want in checks:
        assert rc == want, (what, rc)
    assert (out._ibuf == out._sentinel).all() and (bias._ibuf == bias._sentinel).all()
    assert tn(p[0], p[1], M, p[2], p[3], ld, N, None) == 0                      # the same strides without the bias are legal ...
    assert not out.bits().any()                                                 # ... and the product of zero planes is written
    _intact(out, bias, *P)


# ---------------------------------------------------------------------------------------------------- casts
def _cast_source(R, Cc, gather, layout):
    """fp32 [rows, Cc] with signed zeros, a denormal, bf16 rounding ties among normal values (finite: the column sums
    are compared, and NaN / Inf are test_gpu_bf16_grads.py's), guarded in `layout`, and the rows the cast selects."""
    import torch
    rng = np.random.default_rng(R * 11 + Cc)
    rows = R + 9 if gather else R
    x = (rng.standard_normal((rows, Cc)) * 3).astype(np.float32)
    sp = np.float32([0.0, -0.0, 1e-40, 1.00390625, 1.01171875, -1.00390625, 255.5, -1.5e-39])
    x.reshape(-1)[:sp.size] = sp
    x.reshape(-1)[-sp.size:] = sp
    ld, lead = (_pad(Cc, 4) + 4, 65) if layout == "mis" else (_pad(Cc, 4) + 8, 64)
    src = Guarded.of(x, ld=ld, lead=lead, name="src")
    assert src.ld % 4 == 0 and src.aligned16 == (layout != "mis")
    idx = rng.integers(0, rows, R).astype(np.int32) if gather else None
    if gather:
        idx[0], idx[-1] = rows - 1, 0
    gi = Guarded.of(idx, tail=256, fill=rows - 1, name="rowidx") if gather else None
    sel = torch.as_tensor(x[idx] if gather else x)
    return src, gi, sel


def _bits16(t):
    import torch
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("layout", ["mis", "strided"])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("R,Cc,gather", [(17, 37, False), (130, 100, False), (65, 500, True)])
def test_cast_rows_guarded(gpu, R, Cc, gather, split, layout):
    import torch
    L, st = _lib(), gpu._stream()
    src, gi, sel = _cast_source(R, Cc, gather, layout)
    Kp = _pad(Cc, 64)
    dst = [Guarded(R, Kp, ld=Kp + 8, dtype=torch.bfloat16, name=n) for n in (("dst_hi", "dst_lo") if split else ("dst",))]
    ip = None if gi is None else gi.ptr
    if split:
        rc = L.s2vt_cast_bf16_split(src.ptr, src.ld, ip, R, Cc, 0, dst[0].ptr, dst[1].ptr, Kp + 8, 0, None, None, None, 0, None, 0, st)
    else:
        rc = L.s2vt_cast_bf16(src.ptr, src.ld, ip, R, Cc, 0, dst[0].ptr, Kp + 8, 0, None, None, 0, None, 0, st)
    assert rc == 0
    for d, want in zip(dst, _split(sel)):
        got = d.numpy()
        assert np.array_equal(got[:, :Cc], _bits16(want)), d.name
        assert not got[:, Cc:].any(), "zeros in the pad columns up to Kp"
    _intact(src, gi, *dst)


@pytest.mark.parametrize("layout", ["mis", "strided"])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("R,Cc,gather", [(17, 37, False), (130, 100, False), (65, 500, True)])
def test_cast_transposed_guarded(gpu, R, Cc, gather, split, layout):
    """dst[c][r] with Rp > R (one 64 more than the round-up) and ldd = Rp + 8, the row form beside it with row_ldd = Kp + 4, and the fp32
    column sums added to a non-zero colsum through a scratch of exactly the size the header asks for."""
    import torch
    L, st = _lib(), gpu._stream()
    src, gi, sel = _cast_source(R, Cc, gather, layout)
    Kp, Rp = _pad(Cc, 64), _pad(R, 64) + 64
    names = ("hi", "lo") if split else ("",)
    dst = [Guarded(Cc, Rp, ld=Rp + 8, dtype=torch.bfloat16, name="dst" + n) for n in names]
    rdst = [Guarded(R, Kp, ld=Kp + 4, dtype=torch.bfloat16, name="row_dst" + n) for n in names]
    cs0 = np.random.default_rng(Cc).standard_normal(Cc).astype(np.float32)
    colsum = Guarded.of(cs0, name="colsum")
    part = (Rp + 255) // 256 * Cc
    scratch = Guarded(1, part, name="scratch")
    ip = None if gi is None else gi.ptr
    if split:
        rc = L.s2vt_cast_bf16_split(src.ptr, src.ld, ip, R, Cc, 1, dst[0].ptr, dst[1].ptr, Rp + 8, Rp, colsum.ptr, rdst[0].ptr, rdst[1].ptr, Kp + 4,
                                    scratch.ptr, 4 * part, st)
    else:
        rc = L.s2vt_cast_bf16(src.ptr, src.ld, ip, R, Cc, 1, dst[0].ptr, Rp + 8, Rp, colsum.ptr, rdst[0].ptr, Kp + 4, scratch.ptr, 4 * part, st)
    assert rc == 0
    for d, rd, want in zip(dst, rdst, _split(sel)):
        got, rgot = d.numpy(), rd.numpy()
        assert np.array_equal(got[:, :R], _bits16(want.t())), d.name
        assert not got[:, R:].any(), "zeros in the rows R .. Rp"
        assert np.array_equal(rgot[:, :Cc], _bits16(want)) and not rgot[:, Cc:].any(), rd.name
    ref = cs0.astype(np.float64) + sel.double().sum(0).numpy()
    bound = 1e-6 * float(sel.double().abs().sum(0).max() + np.abs(cs0).max())   # test_cast_transpose_bit_exact_with_colsum
    err = float(np.abs(colsum.numpy()[0].astype(np.float64) - ref).max())
    print(f"\ncast_tr {R}x{Cc} {layout} split={split}: colsum max err {err:.3e}, bound {bound:.3e} ({err / bound:.3f})")
    assert err <= bound
    _intact(src, gi, colsum, scratch, *dst, *rdst)
    # one float short of that scratch: refused (S2VT_E_WORKSPACE) before any launch
    for d in dst:
        d.reset()
    if split:
        rc = L.s2vt_cast_bf16_split(src.ptr, src.ld, ip, R, Cc, 1, dst[0].ptr, dst[1].ptr, Rp + 8, Rp, colsum.ptr, rdst[0].ptr, rdst[1].ptr, Kp + 4,
                                    scratch.ptr, 4 * part - 4, st)
    else:
        rc = L.s2vt_cast_bf16(src.ptr, src.ld, ip, R, Cc, 1, dst[0].ptr, Rp + 8, Rp, colsum.ptr, rdst[0].ptr, Kp + 4, scratch.ptr, 4 * part - 4, st)
    assert rc == -3
    assert all(bool((d._ibuf == d._sentinel).all()) for d in dst)
