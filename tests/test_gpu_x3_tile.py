"""The 192 x 96 tile of the NT split-bf16 product (s2vt_gemm_bf16x3_nt_tile, csrc/bwd_bf16.hip) against the 128 x 128 tile: every output
element keeps one accumulator, the same K steps of 32 and the same order of the three products per step, so the bits do not depend on the
tile -- the WHOLE guarded output allocation of one call equals the other's (window, row pads and guards).  Shapes: the smallest that reach
every edge of the new geometry (one row, one short of / exactly / one past a 192-row and a 96-column tile, several tiles both ways, tile
counts that are no multiple of 8 for the XCD remap), two K steps (below the ring depth), four (equal to it) and more (slots reused)."""
import ctypes as C

import numpy as np
import pytest

from guardband import Guarded

pytestmark = pytest.mark.gpu
S2VT_E_BADARG = -1

# M, N, Kp, ldc - N, accumulate
CASES = [
    (1, 95, 64, 0, 0),
    (1, 96, 640, 0, 0),
    (191, 96, 128, 0, 0),
    (192, 96, 640, 0, 0),            # exactly one tile
    (192, 97, 256, 0, 0),
    (193, 95, 128, 0, 0),
    (193, 300, 640, 0, 0),           # 2 x 4 tiles
    (385, 300, 128, 0, 0),           # 3 x 4 = 12 tiles: no multiple of 8
    (200, 1000, 64, 0, 0),           # 2 x 11 = 22 tiles: no multiple of 8
    (385, 97, 256, 0, 0),
    (193, 97, 64, 5, 0),             # ldc > N
    (191, 300, 256, 3, 1),           # accumulate onto a non-zero C
]


def _planes(L, x, Kp):
    """hi / lo planes [rows, Kp] of fp32 x [rows, K] (K <= Kp) from s2vt_cast_bf16_split, zeros past K."""
    import torch
    rows, K = x.shape
    xd = torch.as_tensor(x).cuda()
    hi, lo = (torch.empty((rows, Kp), dtype=torch.int16, device="cuda") for _ in range(2))
    P = lambda t: C.c_void_p(t.data_ptr())
    assert L.s2vt_cast_bf16_split(P(xd), K, None, rows, K, 0, P(hi), P(lo), Kp, 0, None, None, None, 0, None, 0, None) == 0
    return hi, lo


def _operands(L, M, N, Kp):
    rng = np.random.default_rng(M * 7919 + N * 31 + Kp)
    K = Kp - 3                                                 # the last K step carries pad columns
    a = rng.uniform(-1.0, 1.0, (M, K)).astype(np.float32)
    b = rng.uniform(-1.0, 1.0, (N, K)).astype(np.float32)
    return _planes(L, a, Kp), _planes(L, b, Kp), rng.uniform(-1.0, 1.0, (M, N)).astype(np.float32)


@pytest.mark.parametrize("M,N,Kp,pad,accumulate", CASES)
def test_tile_192x96_gives_the_bits_of_128x128(gpu, M, N, Kp, pad, accumulate):
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    P = lambda t: C.c_void_p(t.data_ptr())
    (ah, al), (bh, bl), c0 = _operands(L, M, N, Kp)
    ldc = N + pad
    outs = []
    for tile in (None, 1, 0):
        out = Guarded(M, N, ld=ldc, lead=65, tail=192 * ldc, name=f"C(tile {tile})")
        if accumulate:
            out.fill(c0)
        if tile is None:
            rc = L.s2vt_gemm_bf16x3_nt(P(ah), P(al), Kp, P(bh), P(bl), Kp, out.ptr, ldc, M, N, Kp, accumulate, None, 0, None)
        else:
            rc = L.s2vt_gemm_bf16x3_nt_tile(P(ah), P(al), Kp, P(bh), P(bl), Kp, out.ptr, ldc, M, N, Kp, accumulate, None, tile)
        assert rc == 0, (tile, rc)
        torch.cuda.synchronize()
        out.assert_intact()
        outs.append(out._ibuf.cpu().numpy())
    assert not (outs[0][65:65 + N] == np.int32(0x7FC5A5A5)).any(), "the product did not write its first row"
    assert np.array_equal(outs[1], outs[0]), "192 x 96 tile: bits differ from s2vt_gemm_bf16x3_nt's"
    assert np.array_equal(outs[2], outs[0]), "tile 0 is the 128 x 128 tile of s2vt_gemm_bf16x3_nt"


@pytest.mark.parametrize("tile", [-1, 2, 192])
def test_bad_tile_is_refused_and_writes_nothing(gpu, tile):
    import torch
    import s2vt_amd
    L = s2vt_amd.lib()
    P = lambda t: C.c_void_p(t.data_ptr())
    M, N, Kp = 5, 9, 64
    (ah, al), (bh, bl), _ = _operands(L, M, N, Kp)
    out = Guarded(M, N, name="C")
    out.reset()
    assert L.s2vt_gemm_bf16x3_nt_tile(P(ah), P(al), Kp, P(bh), P(bl), Kp, out.ptr, N, M, N, Kp, 0, None, tile) == S2VT_E_BADARG
    torch.cuda.synchronize()
    out.assert_image(out.image(), "after a refused call")
