"""gemm_bf16x3_nn, the forward form of the split-bf16 product: A by rows, B K-major.  Against float64 of the three split
products, against itself (two runs), accumulate, the fp32 column bias (exactly the bias-free output + bias), the guard columns of a
strided output, NaN everywhere the kernel must not read, and bit equality with gemm_bf16x3_nt on explicitly transposed B planes and
with gemm_bf16x3_tn on explicitly transposed A planes (the same K steps in the same order)."""
import pytest

from test_gpu_split_grads import _split_ref
from test_gpu_split_fused import _tn_planes

pytestmark = pytest.mark.gpu


def _pad64(n):
    return (n + 63) // 64 * 64


def _a_planes(x, K):
    """x [M, K] fp32 -> split row planes [M][lda], lda = bf16_pad(K) + 64: columns in [K, bf16_pad(K)) hold 1.0 (finite junk the kernel
    reads and multiplies with B's zeros), the columns beyond hold NaN (never read)."""
    import torch
    M = x.shape[0]
    Kp = _pad64(K)
    out = []
    for p in _split_ref(x):
        buf = torch.full((M, Kp + 64), float("nan"), device="cuda", dtype=torch.bfloat16)
        buf[:, :Kp] = 1.0
        buf[:, :K] = p
        out.append(buf)
    return out


# (1,1,64) smallest; (17,130,100) nk = 4: the prologue only; (130,17,37) odd K, nk = 2 < the ring; (129,257,320) 2 x 3 tiles, the ring wraps;
# (300,1100,1000) 27 tiles: the XCD remap with a remainder, K padded 1000 -> 1024; (320,500,1601) K just past a K step; (1000,4000,1500) stage B's K
@pytest.mark.parametrize("M,N,K", [(1, 1, 64), (17, 130, 100), (130, 17, 37), (129, 257, 320), (300, 1100, 1000), (320, 500, 1601),
                                   (1000, 4000, 1500)])
@pytest.mark.parametrize("split_k", [True, False])
def test_gemm_bf16x3_nn_vs_float64_nt_and_tn(gpu, M, N, K, split_k):
    import torch
    g = torch.Generator(device="cuda").manual_seed(M * 17 + N + K)
    a = torch.randn(M, K, device="cuda", generator=g)
    b = torch.randn(K, N, device="cuda", generator=g)
    ldb = (N + 7) // 8 * 8 + 8
    Ah, Al = _a_planes(a, K)
    # rows >= K and columns >= N of B hold NaN: they must never reach a stored output
    Bh, Bl = _tn_planes(b, ldb, float("nan"))
    ah, al = _split_ref(a)
    bh, bl = _split_ref(b)
    ref = ah.double() @ bh.double() + ah.double() @ bl.double() + al.double() @ bh.double()
    scale = float(ref.abs().max()) + 1e-30
    tol = 1e-6 * max(1.0, (K / 1000) ** 0.5)
    ldc = N + 3
    C0 = torch.randn(M, ldc, device="cuda", generator=g)
    out = C0.clone()
    gpu.gemm_bf16x3_nn(Ah, Al, Bh, Bl, N, out=out[:, :N], split_k=split_k)
    err = float((out[:, :N].double() - ref).abs().max())
    print(f"\nnn {M}x{N}x{K} split_k={split_k}: max err {err:.3e}, bound {tol * scale:.3e}")
    assert not torch.isnan(out).any()
    assert err <= tol * scale
    assert torch.equal(out[:, N:], C0[:, N:])                           # guard columns
    first = out.clone()
    gpu.gemm_bf16x3_nn(Ah, Al, Bh, Bl, N, out=out[:, :N], split_k=split_k)
    assert torch.equal(out, first)                                      # deterministic
    acc = C0.clone()
    gpu.gemm_bf16x3_nn(Ah, Al, Bh, Bl, N, out=acc[:, :N], accumulate=True, split_k=split_k)
    want = ref + C0[:, :N].double()
    assert float((acc[:, :N].double() - want).abs().max()) <= tol * (scale + float(C0.abs().max()))
    assert torch.equal(acc[:, N:], C0[:, N:])
    # the fp32 column bias: exactly the bias-free output + bias[col]
    bias = torch.randn(N, device="cuda", generator=g)
    withb = C0.clone()
    gpu.gemm_bf16x3_nn(Ah, Al, Bh, Bl, N, out=withb[:, :N], split_k=split_k, bias=bias)
    assert torch.equal(withb[:, :N], first[:, :N] + bias[None, :])
    assert torch.equal(withb[:, N:], C0[:, N:])
    # the same K steps in the same order: the bits of the NT form on explicitly transposed B planes ...
    Kp = _pad64(K)
    bt = [torch.zeros(N, Kp, device="cuda", dtype=torch.bfloat16) for _ in range(2)]
    for t, p in zip(bt, (bh, bl)):
        t[:, :K] = p.t()
    ar = [torch.zeros(M, Kp, device="cuda", dtype=torch.bfloat16) for _ in range(2)]
    for t, p in zip(ar, (ah, al)):
        t[:, :K] = p
    nt = gpu.gemm_bf16x3_nt(ar[0], ar[1], bt[0], bt[1], split_k=split_k)
    assert torch.equal(nt, first[:, :N])
    # ... and of the TN form on explicitly transposed A planes
    lda_t = (M + 7) // 8 * 8
    at = [torch.zeros(K, lda_t, device="cuda", dtype=torch.bfloat16) for _ in range(2)]
    for t, p in zip(at, (ah, al)):
        t[:, :M] = p.t()
    tn = gpu.gemm_bf16x3_tn(at[0], at[1], Bh, Bl, M, N, split_k=split_k)
    assert torch.equal(tn, first[:, :N])


def test_gemm_bf16x3_nn_refuses_planes_beyond_the_loader(gpu):
    """ldb beyond gemm_bf16x3_tn_ok's 32-bit offset rule: S2VT_E_BADARG before anything is launched (nothing is dereferenced)."""
    import ctypes
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    K, N = 64, 8
    ldb = (1 << 31) // (2 * (K + 1)) // 8 * 8 + 8                      # (bf16_pad(K) + 1) * ldb * 2 + 512 >= 2^31
    A = torch.zeros(64, 64, device="cuda", dtype=torch.bfloat16)      # (serves as A [8][64] and as B [64 k rows][64] of the accepted call)
    out = torch.zeros(8, N, device="cuda")
    p = ctypes.c_void_p(A.data_ptr())
    rc = L.s2vt_gemm_bf16x3_nn(p, p, 64, p, p, ldb, ctypes.c_void_p(out.data_ptr()), N, 8, N, K, 0, None, None, 0, None)
    assert rc == -1
    ok = L.s2vt_gemm_bf16x3_nn(p, p, 64, p, p, 64, ctypes.c_void_p(out.data_ptr()), N, 8, N, K, 0, None, None, 0, None)
    torch.cuda.synchronize()
    assert ok == 0 and not out.any()
