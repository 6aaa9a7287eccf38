"""The fused split backward's host side, no GPU: the dispatch rule, where the dlogits planes lie, and the argument checks of
s2vt_softmax_nll_fwd_bwd_split and s2vt_gemm_bf16x3_tn."""
import ctypes as C


def test_split_grad_active_is_the_dispatch_rule():
    from s2vt_amd import ops
    assert ops.split_grad_active(320) and ops.split_grad_active(257)
    assert not ops.split_grad_active(256) and not ops.split_grad_active(64)       # the fp32 body's shapes


def test_dlogits_planes_lie_inside_the_split_workspace():
    from s2vt_amd import ops
    L = ops.lib()
    d = ops.make_dims(1536, 12000, 500, 1000, 5, 20)
    hi, lo, ld = C.c_size_t(99), C.c_size_t(0), C.c_int32(0)
    assert L.s2vt_split_grad_dlogits_planes(C.byref(d), 64, 320, C.byref(hi), C.byref(lo), C.byref(ld)) == 0
    plane = 20 * 320 * ld.value * 2
    total = L.s2vt_split_grad_workspace_bytes(C.byref(d), 64, 320)
    assert ld.value == 12032 and hi.value == 0 and lo.value % 256 == 0
    assert hi.value + plane <= lo.value and lo.value + plane <= total
    assert L.s2vt_split_grad_dlogits_planes(C.byref(d), 64, 100, C.byref(hi), C.byref(lo), C.byref(ld)) == -1
    assert L.s2vt_split_grad_dlogits_planes(None, 64, 320, C.byref(hi), C.byref(lo), C.byref(ld)) == -1


def test_fused_entries_reject_bad_arguments():
    from s2vt_amd import ops
    L = ops.lib()
    d = ops.make_dims(128, 260, 32, 64, 5, 8)
    assert L.s2vt_softmax_nll_fwd_bwd_split(None, 260, 8, 260, None, None, 0.0, None, None, None, C.byref(d), 64, 320, None, 0, None) == -1
    assert L.s2vt_gemm_bf16x3_tn(None, None, 64, None, None, 64, None, 8, 8, 8, 64, 0, None, None, 0, None) == -1
    # a backward without dlogits is the fused split form's alone: the fp32 body (<= 256 rows) refuses it
    args = [C.byref(d), None, None, None, 4, 8, None, 8, None, 0, 1.0, 0, None, None, None, 0, 0, C.c_void_p(256), 0, None]
    assert L.s2vt_bptt_bwd_split(*args) == -1
    for name in ("s2vt_gemm_bf16x3_tn", "s2vt_split_grad_active", "s2vt_softmax_nll_fwd_bwd_split", "s2vt_split_grad_dlogits_planes"):
        assert name in ops._lib.SIGNATURES
