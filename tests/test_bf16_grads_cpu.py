"""The bf16 gradient mode's host side, no GPU: the grad_precision attribute and its environment default, the scratch size and
the argument checks of s2vt_bptt_bwd_bf16."""
import ctypes as C

import pytest


def test_grad_precision_env_default(monkeypatch):
    from s2vt_amd import model as M
    monkeypatch.delenv("S2VT_GRAD_PRECISION", raising=False)
    assert M.grad_precision_from_env() == "fp32"
    for v in ("fp32", "bf16"):
        monkeypatch.setenv("S2VT_GRAD_PRECISION", v)
        assert M.grad_precision_from_env() == v
    for bad in ("", "fp16", "BF16", "bfloat16"):
        monkeypatch.setenv("S2VT_GRAD_PRECISION", bad)
        with pytest.raises(ValueError):
            M.grad_precision_from_env()


def test_grad_precision_attribute():
    from s2vt_amd import model as M, multitask as MT
    m = M.Video_Caption_Generator.__new__(M.Video_Caption_Generator)      # (no device needed for the attribute)
    for v in ("bf16", "fp32"):
        m.grad_precision = v
        assert m.grad_precision == v
    with pytest.raises(ValueError):
        m.grad_precision = "fp16"
    assert m.grad_precision == "fp32"
    assert MT.Video_Caption_Generator.grad_precision is M.Video_Caption_Generator.grad_precision     # inherited
    from s2vt_amd import attention as A
    assert not hasattr(A.Attention_Caption_Generator, "grad_precision")


def test_bf16_workspace_bytes():
    from s2vt_amd import ops
    L = ops.lib()
    good = ops.make_dims(1536, 12000, 500, 1000, 5, 20)
    assert L.s2vt_bf16_grad_workspace_bytes(C.byref(good), 64, 320) > 0
    assert L.s2vt_bf16_grad_workspace_bytes(C.byref(good), 64, 320) > L.s2vt_bf16_grad_workspace_bytes(C.byref(good), 64, 64)
    assert L.s2vt_bf16_grad_workspace_bytes(None, 64, 320) == 0
    assert L.s2vt_bf16_grad_workspace_bytes(C.byref(good), 64, 100) == 0            # N not a multiple of B
    assert L.s2vt_bf16_grad_workspace_bytes(C.byref(good), 0, 64) == 0
    bad = ops.make_dims(1536, 0, 500, 1000, 5, 20)
    assert L.s2vt_bf16_grad_workspace_bytes(C.byref(bad), 64, 320) == 0


def test_bptt_bwd_bf16_rejects_null_arguments():
    from s2vt_amd import ops
    L = ops.lib()
    d = ops.make_dims(128, 260, 32, 64, 5, 8)
    args = [C.byref(d), None, None, None, 4, 8, None, 8, None, 0, 1.0, 0, None, None, None, 0, 0, None, 0, None]
    assert L.s2vt_bptt_bwd_bf16(*args) == -1
    args[0] = None
    assert L.s2vt_bptt_bwd_bf16(*args) == -1
    assert L.s2vt_gemm_bf16_nt(None, 64, None, 64, None, 8, 8, 8, 64, 0, 0, None) == -1
    assert L.s2vt_cast_bf16(None, 8, None, 8, 8, 0, None, 64, 0, None, None, 0, None, 0, None) == -1
