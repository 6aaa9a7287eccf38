"""The order-free fp32 gradient contractions through the C ABI inside guard bands (tests/guardband.py): s2vt_gemm_nt_splitk (the split-K
slab product of the data gradients) and s2vt_gemm_tn (the weight gradients: the LDS-DMA 128x128 tile and the register-staged tiles),
against float64 within the bounds of test_gpu_splitk.py (2e-5 of max |ref|) and test_gpu_timed_tiles.py (5e-5 of max |ref|), in the
layouts of test_gpu_abi_gemm.py: dense, strided (row strides cols + 4 j, still the vector / DMA kernels), odd-ld:X and mis:X (one
operand with ld = cols + 1, or 4 bytes past a 16-byte boundary: the scalar kernels).  Outputs, slab buffers and inputs keep their NaN
guards; a gather index array is followed by 256 valid entries."""
import numpy as np
import pytest

from guardband import Guarded
from test_gpu_timed_tiles import _launched_tiles

pytestmark = pytest.mark.gpu
VARIANTS = ["dense", "strided", "odd-ld:A", "odd-ld:B", "mis:A", "mis:B"]
BK = 32                                              # gemm_mfma.h: the K chunk a slab is a whole number of


def _lib():
    import s2vt_amd
    return s2vt_amd.lib()


def _layout(variant, who, j):
    kind, _, target = variant.partition(":")
    if kind == "strided":
        return 4 * j, 64
    if kind == "odd-ld" and target == who:
        return 1, 64
    if kind == "mis" and target == who:
        return 0, 65
    return 0, 64


def _intact(*gs):
    for g in gs:
        if g is not None:
            g.assert_intact()


# ---------------------------------------------------------------------------------------------------- s2vt_gemm_nt_splitk
def _nslab(K, s):
    """What train.hip makes of `s` slabs: slabs of a whole number of chunks, and the count that then covers K."""
    kper = ((K + s - 1) // s + BK - 1) // BK * BK
    return (K + kper - 1) // kper


@pytest.fixture(scope="module")
def splitk_refs():
    import torch
    refs = {}
    for M, N, K in [(70, 36, 1028), (129, 132, 1028)]:
        g = torch.Generator().manual_seed(M + N)
        A = torch.randn(M, K, generator=g)
        Wt = torch.randn(N, K, generator=g) * 0.1
        refs[(M, N, K)] = (A.numpy(), Wt.numpy(), (A.double() @ Wt.double().t()).numpy())
    return refs


@pytest.mark.parametrize("variant", VARIANTS)
def test_splitk_forced_and_chosen_slab_counts_guarded(gpu, splitk_refs, variant):
    """(70, 36, 1028): the library's slab count (4 slabs of 288), none, 3 slabs of 352, and 5 asked for -- slabs of 224, not of
    K / 5 = 205.6 -- with `slabs` exactly as large as the slabs written."""
    L, st = _lib(), gpu._stream()
    M, N, K = 70, 36, 1028
    A, Wt, ref = splitk_refs[(M, N, K)]
    scale = float(np.abs(ref).max())
    pa, la = _layout(variant, "A", 1)
    pb, lb = _layout(variant, "B", 2)
    gA, gW = Guarded.of(A, ld=K + pa, lead=la, name="A"), Guarded.of(Wt, ld=K + pb, lead=lb, name="Wt")
    out = Guarded(M, N, name="C")                                              # ldc == N: what the slab sum needs
    for splits in (0, 1, 3, 5):
        n = _nslab(K, splits) if splits > 1 else (12 if splits == 0 else 1)     # splits = 0: room for the most the library chooses
        assert splits != 5 or (n == 5 and ((K + 4) // 5 + BK - 1) // BK * BK == 224)
        slabs = Guarded(1, n * M * N, name="slabs")
        out.reset()
        rc = L.s2vt_gemm_nt_splitk(gA.ptr, gA.ld, gW.ptr, gW.ld, out.ptr, out.ld, M, N, K, splits, -1, slabs.ptr, n * M * N, st)
        assert rc == 0
        err = float(np.abs(out.numpy().astype(np.float64) - ref).max())
        print(f"\nsplitk {M}x{N}x{K} {variant} splits={splits}: max err {err:.3e}, bound {2e-5 * scale:.3e} ({err / (2e-5 * scale):.3f})")
        assert err <= 2e-5 * scale, (splits, variant)
        written = bool((slabs._iview != slabs._sentinel).any())
        assert written == (splits != 1), (splits, "the slab buffer is used exactly when the reduction is cut")
        _intact(out, slabs)
    if variant == "dense":                                                      # one float short of the slabs it will write: refused
        slabs = Guarded(1, 5 * M * N, name="slabs")
        out.reset()
        assert L.s2vt_gemm_nt_splitk(gA.ptr, gA.ld, gW.ptr, gW.ld, out.ptr, out.ld, M, N, K, 5, -1, slabs.ptr, 5 * M * N - 1, st) == -3
        assert (out._ibuf == out._sentinel).all() and (slabs._ibuf == slabs._sentinel).all()
    _intact(gA, gW)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("pad_c", [0, 4])
def test_splitk_falls_back_to_one_pass_for_a_strided_output(gpu, splitk_refs, variant, pad_c):
    """(129, 132, 1028), splits = 0: with ldc == N the library cuts the reduction and the slab buffer is written; with ldc = N + 4 the
    slabs cannot be summed into C, the product runs in one pass and the slab buffer keeps every bit."""
    L, st = _lib(), gpu._stream()
    M, N, K = 129, 132, 1028
    A, Wt, ref = splitk_refs[(M, N, K)]
    scale = float(np.abs(ref).max())
    pa, la = _layout(variant, "A", 1)
    pb, lb = _layout(variant, "B", 2)
    gA, gW = Guarded.of(A, ld=K + pa, lead=la, name="A"), Guarded.of(Wt, ld=K + pb, lead=lb, name="Wt")
    out, slabs = Guarded(M, N, ld=N + pad_c, name="C"), Guarded(1, 12 * M * N, name="slabs")
    rc = L.s2vt_gemm_nt_splitk(gA.ptr, gA.ld, gW.ptr, gW.ld, out.ptr, out.ld, M, N, K, 0, -1, slabs.ptr, 12 * M * N, st)
    assert rc == 0
    err = float(np.abs(out.numpy().astype(np.float64) - ref).max())
    print(f"\nsplitk {M}x{N}x{K} {variant} ldc=N+{pad_c}: max err {err:.3e}, bound {2e-5 * scale:.3e} ({err / (2e-5 * scale):.3f})")
    assert err <= 2e-5 * scale
    assert bool((slabs._iview != slabs._sentinel).any()) == (pad_c == 0)
    _intact(out, slabs, gA, gW)
    if pad_c:                                                                   # an explicit slab count cannot be honoured: refused
        out.reset()
        assert L.s2vt_gemm_nt_splitk(gA.ptr, gA.ld, gW.ptr, gW.ld, out.ptr, out.ld, M, N, K, 3, -1, slabs.ptr, 12 * M * N, st) == -1
        assert (out._ibuf == out._sentinel).all()


# ---------------------------------------------------------------------------------------------------- s2vt_gemm_tn
# Mred, Kout, N, the tile the launcher selects on 16-byte aligned operands / on the others (aux.hip launch_gemm_tn)
TN_SHAPES = [
    (5, 520, 5124, "tn128x128(dma)", "tn128x128(2x2)"),      # 5 x 41 = 205 tiles of 128x128 (>= 200); a reduction shorter than a 16-row chunk
    (37, 520, 5124, "tn128x128(dma)", "tn128x128(2x2)"),     # ragged: two chunks and five rows
    (600, 520, 5124, "tn128x128(dma)", "tn128x128(2x2)"),    # three reduction slabs of 224 rows: atomics into a zeroed / pre-filled C
    (300, 132, 260, "tn64x64(2x2)", "tn64x64(2x2)"),         # register-staged, two reduction slabs
    (40, 68, 100, "tn64x64(2x2)", "tn64x64(2x2)"),           # register-staged, one slab
]


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("Mred,Kout,N,tile_vec,tile_scalar", TN_SHAPES)
def test_weight_gradient_layouts_guarded(gpu, Mred, Kout, N, tile_vec, tile_scalar, gather):
    """C[Kout, N] (+)= A[row(m)]^T B over m < Mred into a pre-filled guarded C, plain and gathered A, in every layout: the tile the
    launcher selected (launch profiler), the bound of test_weight_gradient_tiles_vs_float64 and -- where the launch is one reduction slab
    (Mred <= 256: no atomics) -- the same bits from the dense and the strided layout."""
    import torch
    L, st = _lib(), gpu._stream()
    g = torch.Generator().manual_seed(Mred + N + int(gather))
    rows = Mred + 50 if gather else Mred
    A = torch.randn(rows, Kout, generator=g)
    Bm = torch.randn(Mred, N, generator=g)
    C0 = torch.randn(Kout, N, generator=g)
    idx = torch.randint(0, rows, (Mred,), generator=g).int() if gather else None
    if gather:
        idx[0] = rows - 1
    Asel = A[idx.long()] if gather else A
    ref = (Asel.double().cuda().t() @ Bm.double().cuda()).cpu()
    scale = float(ref.abs().max())
    gi = Guarded.of(idx.numpy(), tail=256, fill=rows - 1, name="rowidx") if gather else None
    bits = {}
    for variant in VARIANTS:
        pa, la = _layout(variant, "A", 1)
        pb, lb = _layout(variant, "B", 2)
        gA, gB = Guarded.of(A, ld=Kout + pa, lead=la, name="A"), Guarded.of(Bm, ld=N + pb, lead=lb, name="B")
        out = Guarded(Kout, N, ld=N + (0 if variant == "dense" else 12), name="C")
        for accumulate in (0, 1):
            out.fill(C0)
            rc, tiles = _launched_tiles(gpu, lambda: L.s2vt_gemm_tn(gA.ptr, gA.ld, None if gi is None else gi.ptr, gB.ptr, gB.ld, out.ptr, out.ld,
                                                                   Mred, Kout, N, accumulate, st))
            assert rc == 0
            names = [n for (c, n) in tiles if c == 3]
            assert names == [tile_vec if variant in ("dense", "strided") else tile_scalar], (variant, tiles)
            want = ref + C0.double() if accumulate else ref
            got = torch.as_tensor(out.numpy())
            err = float((got.double() - want).abs().max())
            print(f"\ngemm_tn {Mred}x{Kout}x{N} gather={gather} {variant} acc={accumulate}: {names[0]}, max err {err:.3e}, "
                  f"bound {5e-5 * scale:.3e} ({err / (5e-5 * scale):.3f})")
            assert err <= 5e-5 * scale, (variant, accumulate)
            out.assert_intact()
            if variant in ("dense", "strided"):
                bits[(variant, accumulate)] = out.bits()
        _intact(gA, gB, gi)
    if Mred <= 256:
        for accumulate in (0, 1):
            assert np.array_equal(bits[("dense", accumulate)], bits[("strided", accumulate)]), accumulate
