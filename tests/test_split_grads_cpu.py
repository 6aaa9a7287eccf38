"""The split-bf16 gradient products' host side, no GPU: the scratch size and the argument checks of s2vt_bptt_bwd_split,
s2vt_cast_bf16_split and s2vt_gemm_bf16x3_nt."""
import ctypes as C


def test_split_workspace_bytes():
    from s2vt_amd import ops
    L = ops.lib()
    good = ops.make_dims(1536, 12000, 500, 1000, 5, 20)
    split = L.s2vt_split_grad_workspace_bytes(C.byref(good), 64, 320)
    bf16 = L.s2vt_bf16_grad_workspace_bytes(C.byref(good), 64, 320)
    assert split >= 2 * bf16 - 2 * 4 * (bf16 // 4 // 8)                 # two planes of every operand (+ split-K slabs)
    assert split < 3 * bf16
    assert L.s2vt_split_grad_workspace_bytes(C.byref(good), 64, 320) > L.s2vt_split_grad_workspace_bytes(C.byref(good), 64, 64)
    assert L.s2vt_split_grad_workspace_bytes(None, 64, 320) == 0
    assert L.s2vt_split_grad_workspace_bytes(C.byref(good), 64, 100) == 0           # N not a multiple of B
    assert L.s2vt_split_grad_workspace_bytes(C.byref(good), 0, 64) == 0
    bad = ops.make_dims(1536, 0, 500, 1000, 5, 20)
    assert L.s2vt_split_grad_workspace_bytes(C.byref(bad), 64, 320) == 0


def test_split_entries_reject_null_arguments():
    from s2vt_amd import ops
    L = ops.lib()
    d = ops.make_dims(128, 260, 32, 64, 5, 8)
    args = [C.byref(d), None, None, None, 4, 8, None, 8, None, 0, 1.0, 0, None, None, None, 0, 0, None, 0, None]
    assert L.s2vt_bptt_bwd_split(*args) == -1
    args[0] = None
    assert L.s2vt_bptt_bwd_split(*args) == -1
    assert L.s2vt_gemm_bf16x3_nt(None, None, 64, None, None, 64, None, 8, 8, 8, 64, 0, None, 0, None) == -1
    assert L.s2vt_cast_bf16_split(None, 8, None, 8, 8, 0, None, None, 64, 0, None, None, None, 0, None, 0, None) == -1


def test_fp32_precision_is_the_default():
    from s2vt_amd import ops
    assert ops.GRAD_PRECISIONS[0] == "fp32"
    for name in ("s2vt_bptt_bwd_split", "s2vt_split_grad_workspace_bytes", "s2vt_cast_bf16_split", "s2vt_gemm_bf16x3_nt"):
        assert name in ops._lib.SIGNATURES
