"""Inputs for the tests of the one-product pick screen (csrc/pick_screen.hip: L1 = bf16(h) . bf16(W) in fp32; the product's own bound C1
and the screen's margin m1, built from what the two casts miss) -- a plain
helper module shared by tests/test_pick_screen1_cases_cpu.py (numpy only: each family has the property that makes it discriminate) and
tests/test_gpu_pick_screen1.py (the product entry s2vt_gemm_bf16x1_nt and the sampler on the default path)."""
import os
import re

import numpy as np

from pick_margin_cases import ALL_ONES, bf16_rne, product_scale

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multitask-end-to-end-video-captioning_amd", "csrc")

C3 = 2.0 ** -10                                   # the three-product screen's constant: what a build that forgot to switch would use
PRODUCT_R, PRODUCT_V = 65, 300                    # one row past a 64-row block; a 44-column tile edge at 96-column tiles
PRODUCT_K = [1024, 1028, 2048]                    # the last K of C1 x 1, the first of C1 x 2 (a padded K step), all of C1 x 2
FAMILIES = ["uniform", "all-ones", "worst-cast"]
# an fp32 value a bf16 cast loses the most of: the bf16 mantissa (fraction bits 22 .. 16) zero, the low 16 bits 0x7fff -- RNE rounds DOWN by just
# under half an ulp of a value just above a power of two, 0.996 x 2^-8 of it
WORST_CAST_FRACTION = 0x7FFF


def c1():
    """C1 = 2^-7 + 2^-11 per 1024 reduction steps: what bounds the one product on ANY operands (two casts of up to 2^-8 each, 2^-11 for the
    accumulation) -- the promise of s2vt_gemm_bf16x1_nt in include/s2vt.h."""
    return 2.0 ** -7 + 2.0 ** -11


def bound(K):
    return c1() * ((K + 1023) // 1024)


def acc1():
    """The accumulation share of the screen's margin as csrc/pick_screen.hip states it (kPickAcc1), per 1024 reduction steps."""
    m = re.search(r"constexpr\s+float\s+kPickAcc1\s*=\s*([0-9.eE+-]+)f?\s*;", open(os.path.join(CSRC, "pick_screen.hip")).read())
    assert m, "kPickAcc1 not found in pick_screen.hip"
    return float(m.group(1))


def margin_m1(h, W):
    """What the resolve kernel's m1 promises per output, with each column's own norms in place of the maxima over columns (so no larger
    than the kernel's m1): acc1 ceil(K / 1024) |h| |w| + |h - bf16(h)| |w| + (1 + 2^-8) |h| |w - bf16(w)|, float64."""
    h64, W64 = h.astype(np.float64), W.astype(np.float64)
    nh, nw = np.linalg.norm(h64, axis=1)[:, None], np.linalg.norm(W64, axis=0)[None, :]
    dh = np.linalg.norm(h64 - bf16_rne(h).astype(np.float64), axis=1)[:, None]
    dw = np.linalg.norm(W64 - bf16_rne(W).astype(np.float64), axis=0)[None, :]
    return acc1() * ((h.shape[1] + 1023) // 1024) * nh * nw + dh * nw + (1.0 + 2.0 ** -8) * nh * dw


def product_inputs(family, R, K, V):
    """h [R, K] and W [K, V], fp32.
    "uniform": zero-mean, as tests/test_gpu_pick_screen.py's.
    "all-ones": every entry positive with all 24 mantissa bits set over three adjacent exponents (bf16 rounds it UP to the next power of
        two, by 2^-24 of it: nothing cancels, what it stresses is the accumulation).
    "worst-cast": every entry positive, fraction WORST_CAST_FRACTION, the same exponents: both casts of every term round down by nearly
        2^-8 of the operand, all errors have one sign and add up over k -- just under 2^-7 of sum |h_k w_k|."""
    rng = np.random.default_rng(1000 + R + K)
    if family == "uniform":
        return rng.uniform(-1.0, 1.0, (R, K)).astype(np.float32), rng.uniform(-0.1, 0.1, (K, V)).astype(np.float32)
    eh, ew = rng.integers(-2, 1, (R, K)), rng.integers(-6, -3, (K, V))
    if family == "all-ones":
        return np.ldexp(ALL_ONES, eh).astype(np.float32), np.ldexp(ALL_ONES, ew).astype(np.float32)
    assert family == "worst-cast"
    x = np.array([0x3F800000 | WORST_CAST_FRACTION], np.uint32).view(np.float32)[0]
    return np.ldexp(x, eh).astype(np.float32), np.ldexp(x, ew).astype(np.float32)


def product_emulated(h, W):
    """bf16(h) . bf16(W) with the products exact and the sum in float64: the one-product screen without its accumulation roundings."""
    return bf16_rne(h).astype(np.float64) @ bf16_rne(W).astype(np.float64)


def ratios(approx, h, W):
    """(max |approx - L| / (|h| |w|), max |approx - L| / sum |h_k w_k|) against the float64 product L of the fp32 operands."""
    true = h.astype(np.float64) @ W.astype(np.float64)
    err = np.abs(np.asarray(approx, np.float64) - true)
    mass = np.abs(h.astype(np.float64)) @ np.abs(W.astype(np.float64))
    return float((err / product_scale(h, W)).max()), float((err / mass).max())


def apply_worst_cast(p):
    """A sampler case from the worst-cast family: every entry of embed_word_W keeps its sign, exponent and bf16 mantissa and takes the low
    16 bits 0x7fff (a change of under 2^-7 relative) -- every cast of W then rounds towards zero by just under half a bf16 ulp.  The
    decode's h is what it is."""
    W = p["embed_word_W"]
    b = W.view(np.uint32)
    b[:] = (b & np.uint32(0xFFFF0000)) | np.uint32(WORST_CAST_FRACTION)
