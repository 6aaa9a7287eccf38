"""The tile rule of the NT split-bf16 product without a GPU (s2vt_gemm_bf16x3_nt_tile_choice, host only): 192 x 96 where its rounds of
workgroups over the CUs, times its tile area, come to less than the 128 x 128 tile's; and the host-side refusals of the tile entry."""
import ctypes as C

import pytest

import s2vt_amd


@pytest.mark.parametrize("M,N,cus,want", [
    (384, 12000, 256, 1),            # the pick screen at the rl shape: 250 tiles in one round against 282 in two
    (128, 12000, 256, 0),            # one round either way: the smaller tile area wins
    (192, 12000, 256, 0),
    (6400, 1000, 256, 0),            # 374 against 400 tiles, two rounds both
    (2304, 9972, 256, 1),            # rl_ref: 1248 tiles in 5 rounds against 1404 in 6
])
def test_rule(M, N, cus, want):
    assert s2vt_amd.lib().s2vt_gemm_bf16x3_nt_tile_choice(M, N, cus) == want


def test_rule_is_the_documented_inequality():
    L = s2vt_amd.lib()
    up = lambda a, b: (a + b - 1) // b
    for M, N, cus in [(1, 1, 256), (193, 97, 8), (385, 300, 3), (5000, 5000, 304), (100000, 12000, 256), (384, 12000, 1)]:
        t192, t128 = up(M, 192) * up(N, 96), up(M, 128) * up(N, 128)
        want = int(up(t192, cus) * 192 * 96 < up(t128, cus) * 128 * 128)
        assert L.s2vt_gemm_bf16x3_nt_tile_choice(M, N, cus) == want, (M, N, cus)
    assert L.s2vt_gemm_bf16x3_nt_tile_choice(0, 12000, 256) == -1 and L.s2vt_gemm_bf16x3_nt_tile_choice(384, 12000, 0) == -1


def test_tile_entry_validates_before_any_launch():
    L = s2vt_amd.lib()
    P = C.c_void_p(4096)                                        # never dereferenced
    f = lambda tile=1, Ah=P, lda=64, Kp=64, acc=0, M=8: L.s2vt_gemm_bf16x3_nt_tile(Ah, P, lda, P, P, 64, P, 8, M, 8, Kp, acc, None, tile)
    assert f(tile=2) == -1 and f(tile=-1) == -1
    assert f(Ah=None) == -1 and f(lda=32) == -1 and f(Kp=32, lda=64) == -1 and f(acc=2) == -1
    assert f(Ah=C.c_void_p(4096 + 8)) == -2
    assert f(M=0) == 0                                          # nothing to do: nothing launched
