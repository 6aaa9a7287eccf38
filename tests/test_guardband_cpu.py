"""tests/guardband.py on CPU tensors: an untouched buffer passes, one planted element in the lead, the tail or a row pad fails and is
located, the window round-trips, and lead % 4 == 1 really gives a 4-byte but not 16-byte aligned window.  Then GuardedWorkspace, the
byte window of a driver's workspace, and the four workspace checks of tests/workspace_contract.py on fake drivers."""
import numpy as np
import pytest
import torch

import workspace_contract as wc
from guardband import SENTINEL16, SENTINEL32, SENTINEL64, Guarded, GuardedWorkspace


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.bfloat16])
def test_untouched_buffer_is_intact_and_holds_the_sentinel(dtype):
    g = Guarded(5, 7, ld=10, dtype=dtype, lead=65, tail=70, device="cpu")
    g.assert_intact()
    assert g._buf.numel() == 65 + 5 * 10 + 70
    if dtype == torch.bfloat16:
        assert (g._ibuf == SENTINEL16).all() and torch.isnan(g._buf.float()).all()
    else:
        assert (g._ibuf == SENTINEL32).all()
    if dtype == torch.float32:
        assert torch.isnan(g._buf).all()                              # an out-of-window read poisons a result


def test_writes_inside_the_window_are_not_reported():
    g = Guarded(4, 6, ld=9, device="cpu")
    g.view.zero_()
    g.view[3, 5] = float("nan")
    g.assert_intact()


@pytest.mark.parametrize("where", ["lead", "tail", "pad", "last_pad", "first", "last"])
def test_one_planted_element_is_found(where):
    g = Guarded(4, 6, ld=9, lead=64, tail=64, device="cpu")
    g.fill(np.arange(24, dtype=np.float32).reshape(4, 6))
    off = {"lead": 63, "tail": 64 + 4 * 9 + 5, "pad": 64 + 2 * 9 + 6, "last_pad": 64 + 3 * 9 + 8, "first": 0, "last": 64 + 36 + 63}[where]
    g._buf[off] = 1.0
    with pytest.raises(AssertionError) as e:
        g.assert_intact()
    msg = str(e.value)
    assert f"flat offset {off} " in msg
    assert {"lead": "lead guard, 1 element", "first": "lead guard, 64 element", "tail": "tail guard, 5 element", "last": "tail guard, 63 element",
            "pad": "pad of row 2, column 6", "last_pad": "pad of row 3, column 8"}[where] in msg


def test_a_changed_nan_payload_is_a_write():
    """The comparison is on bits: another NaN in a guard is a write, too."""
    g = Guarded(2, 3, device="cpu")
    g._ibuf[10] = 0x7FC00000
    with pytest.raises(AssertionError):
        g.assert_intact()
    h = Guarded(2, 3, dtype=torch.int32, device="cpu")
    h._ibuf[64 + 6] = 0
    with pytest.raises(AssertionError):
        h.assert_intact()


def test_window_round_trips():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((5, 7)).astype(np.float32)
    g = Guarded.of(a, ld=12, lead=65, device="cpu")
    assert g.view.shape == (5, 7) and g.view.stride() == (12, 1) and g.ld == 12
    assert np.array_equal(g.numpy(), a) and np.array_equal(g.bits(), a.view(np.int32))
    g.assert_intact()
    i = Guarded.of(np.arange(9, dtype=np.int32), device="cpu")
    assert i.view.shape == (1, 9) and i.dtype == torch.int32 and i.numpy().tolist() == [list(range(9))]
    b = Guarded.of(torch.tensor([[1.0, -2.5], [0.0, 3.0]], dtype=torch.bfloat16), ld=4, device="cpu")
    assert b.view.float().tolist() == [[1.0, -2.5], [0.0, 3.0]] and b.numpy().dtype == np.uint16
    b.assert_intact()


def test_lead_sets_the_alignment():
    a = Guarded(3, 4, lead=64, device="cpu")
    m = Guarded(3, 4, lead=65, device="cpu")
    assert a.view.data_ptr() % 16 == 0 and a.aligned16
    assert m.view.data_ptr() % 16 == 4 and m.view.data_ptr() % 4 == 0 and not m.aligned16
    assert m.ptr.value == m.view.data_ptr() == m._buf.data_ptr() + 65 * 4


def test_guards_have_a_minimum():
    with pytest.raises(AssertionError):
        Guarded(2, 2, lead=8, device="cpu")
    with pytest.raises(AssertionError):
        Guarded(2, 2, ld=1, device="cpu")


def test_index_arrays_are_guarded_by_a_valid_index():
    """fill=: the guards of an index array hold an in-range index, a change of one of them is still found, and reset() restores it."""
    idx = np.array([3, 0, 6, 6, 1], np.int32)
    g = Guarded.of(idx, tail=256, fill=6, device="cpu")
    assert g._buf.numel() == 64 + 5 + 256 and g.numpy().tolist() == [idx.tolist()]
    outside = torch.cat([g._buf[:64], g._buf[64 + 5:]])
    assert (outside == 6).all() and int(g._buf.min()) >= 0 and int(g._buf.max()) <= 6       # nothing a kernel could follow out of range
    g.assert_intact()
    g._buf[64 + 5 + 200] = 7
    with pytest.raises(AssertionError) as e:
        g.assert_intact()
    assert "tail guard, 200 element" in str(e.value)
    g.reset()
    g.assert_intact()
    assert (g._buf == 6).all()
    with pytest.raises(AssertionError):
        Guarded(1, 4, fill=1, device="cpu")                           # float windows keep the NaN sentinel


def test_eight_byte_windows():
    """int64 (the packed pick words): both halves of every guard element hold the 32-bit sentinel, and a write of either half is found."""
    g = Guarded(1, 5, dtype=torch.int64, device="cpu", name="packed")
    assert (g._ibuf == SENTINEL64).all() and (g._buf.view(torch.int32) == SENTINEL32).all()
    g.view.zero_()
    g.assert_intact()
    assert g.bits().tolist() == [[0] * 5] and g.view.data_ptr() % 16 == 0
    g._buf.view(torch.int32)[2 * (64 + 5) + 1] = 0                    # the high half of the first tail element
    with pytest.raises(AssertionError) as e:
        g.assert_intact()
    assert "tail guard, 0 element" in str(e.value) and "packed" in str(e.value)


def test_reset_poisons_the_window():
    g = Guarded.of(np.ones((2, 3), np.float32), ld=5, device="cpu")
    g.reset()
    assert (g.bits() == SENTINEL32).all() and np.isnan(g.numpy()).all()
    g.assert_intact()


@pytest.mark.parametrize("dtype,ld", [(torch.float32, 9), (torch.int32, 6), (torch.int64, 16)])
def test_image_is_the_whole_allocation_after_writing_some_rows(dtype, ld):
    """image(rows, values): those rows of the window, the sentinel everywhere else -- the window's other rows included; assert_image
    passes on exactly that and names a row that was written though it is not listed, a listed row that was not, and a guard."""
    cols = 6 if dtype != torch.int64 else 1
    g = Guarded(5, cols, ld=ld, dtype=dtype, lead=65, device="cpu")
    vals = np.arange(2 * cols).reshape(2, cols).astype({torch.float32: np.float32, torch.int32: np.int32, torch.int64: np.int64}[dtype])
    img = g.image([1, 3], vals)
    assert img.numel() == g._buf.numel() and int((img != g._sentinel).sum()) == 2 * cols
    assert torch.equal(g.image(), torch.full_like(g._ibuf, g._sentinel)) and torch.equal(g.image([], vals[:0]), g.image())
    g.reset()
    g.assert_image(g.image())
    g.view[torch.tensor([1, 3])] = torch.as_tensor(vals)
    g.assert_image(img)
    g.assert_intact()
    g.view[4, 0] = 7                                                   # a row that is not listed
    with pytest.raises(AssertionError, match="window row 4, column 0"):
        g.assert_image(img)
    g.reset()
    g.view[1] = torch.as_tensor(vals[0])                               # row 3 was never written
    with pytest.raises(AssertionError, match="window row 3, column 0"):
        g.assert_image(img)
    g.view[3] = torch.as_tensor(vals[1])
    g._ibuf[64] = 0                                                    # the last guard element in front of the window
    with pytest.raises(AssertionError, match="lead guard, 1 element"):
        g.assert_image(img)


# ---- GuardedWorkspace: the byte window of a driver's `void* workspace, size_t bytes`
def test_workspace_window_is_exact_aligned_and_between_two_guards():
    g = GuardedWorkspace(768, device="cpu", name="ws")
    assert g.nbytes == 768 and g.as_uint8().numel() == 768 and g.as_uint8().dtype == torch.uint8
    assert g.ptr.value == g.as_uint8().data_ptr() and g.ptr.value % 256 == 0
    assert g.lead >= 256 and g.tail >= 4096 and g._buf.numel() == g.lead + 768 + g.tail
    assert g.window.data_ptr() == g._buf.data_ptr() + g.lead
    assert (g._front == SENTINEL32).all() and (g._back == SENTINEL32).all() and g._front.numel() * 4 == g.lead
    g.assert_intact()
    g.window.fill_(0xFF)                                               # the window is the caller's to dirty
    g.assert_intact()
    assert g.as_uint8(512).numel() == 512 and g.as_uint8(512).data_ptr() == g.ptr.value
    for bad in (0, 100, 257):
        with pytest.raises(AssertionError):
            GuardedWorkspace(bad, device="cpu")


@pytest.mark.parametrize("word,where", [(0, "0 byte(s) behind the window's end"), (1023, "4092 byte(s) behind"), (-1, "4 byte(s) in front of the window")])
def test_workspace_guard_writes_are_located(word, where):
    g = GuardedWorkspace(512, device="cpu", name="ws")
    (g._back if word >= 0 else g._front)[word] = 0
    with pytest.raises(AssertionError) as e:
        g.assert_intact()
    assert where in str(e.value) and "ws" in str(e.value)


def test_workspace_snapshot_compares_a_byte_range():
    g = GuardedWorkspace(1024, device="cpu", name="ws")
    g.window.copy_(torch.arange(1024) % 251)
    snap = g.snapshot()
    g.assert_unchanged(snap, 0, 1024)
    g.window[300] ^= 1
    g.assert_unchanged(snap, 0, 300); g.assert_unchanged(snap, 301, 1024); g.assert_unchanged(snap, 512)
    with pytest.raises(AssertionError, match=r"first at window offset 300 \(44 past 256\)"):
        g.assert_unchanged(snap, 256, 1024, "tail")
    assert snap.data_ptr() != g.window.data_ptr()


# ---- the four workspace checks (tests/workspace_contract.py) on fake drivers: half-built ones are rejected, the correct one passes
class _Refused(Exception):
    pass


def _declared(n):
    return (4 * n + 255) // 256 * 256


def _word(ws, byte_off):
    """One int32 at byte_off from the start of the view `ws`, outside it if byte_off says so (what a kernel's stray store does)."""
    base = ws.view(torch.int32)
    return base.as_strided((1,), (1,), base.storage_offset() + byte_off // 4)


def _fake_driver(bug=None):
    """out[j] = 2 * sum_i x[i, j], accumulated in the workspace: it zeroes its n accumulators, adds the rows, doubles.  declared = 4 n bytes
    rounded up to 256."""
    def driver(x, out, ws):
        n = x.shape[1]
        stray = n == SMALL_N                                            # the stray stores: a tail that only this width has
        if bug == "zeroes_before_refusing":
            ws.zero_()
        if ws.numel() < _declared(n) and bug != "never_refuses":
            raise _Refused
        acc = ws.view(torch.float32)[:n] if ws.numel() >= 4 * n else torch.zeros(n)
        if bug != "no_zeroing":
            acc.zero_()
        for row in x:
            acc += row
        if bug == "stores_at_end" and stray:
            _word(ws, _declared(n)).fill_(7)
        if bug == "stores_in_front" and stray:
            _word(ws, -4).fill_(7)
        if bug == "stores_inside_rounding" and stray:                          # past 4 n bytes, inside the declared 256-byte rounding: no overrun
            _word(ws, 4 * n).fill_(7)
        if bug == "stores_past_declared" and stray:                            # 8 bytes behind the declared end
            _word(ws, _declared(n) + 8).fill_(7)
        out.copy_(2 * acc)
    return driver


class _FakeFamily:
    def __init__(self, bug=None):
        self.driver = _fake_driver(bug)
        self.stages = [self.stage]

    def inputs(self, n, variant):
        return (torch.arange(3 * n, dtype=torch.float32).reshape(3, n) + 1) * (1 + 2 * variant)

    def stage(self, env, n, x, state):
        out = env.empty(n)
        self.driver(x, out, env.ws(_declared(n), "fake"))
        state["out"] = out

    def check(self, n, x, state):
        assert torch.equal(state["out"], 2 * x.double().sum(0).float())

    def refused(self, e):
        return isinstance(e, _Refused)


SMALL_N, LARGE_N = 100, 400      # 400 of 512 declared bytes; 1600 of 1792


def _all_checks(fam):
    wc.exact_and_dirty(fam, SMALL_N, "cpu")
    wc.shrink(fam, SMALL_N, LARGE_N, "cpu")
    wc.containment(fam, SMALL_N, LARGE_N, "cpu")
    wc.refusal(fam, SMALL_N, "cpu")


def test_workspace_checks_accept_a_correct_driver():
    _all_checks(_FakeFamily())
    _all_checks(_FakeFamily("stores_inside_rounding"))                 # its own bytes


@pytest.mark.parametrize("bug,check,message", [
    ("stores_at_end", "A", r"window offset 512 \(0 byte\(s\) behind the window's end\)"),
    ("stores_in_front", "A", r"4 byte\(s\) in front of the window"),
    ("stores_past_declared", "A", r"8 byte\(s\) behind the window's end"),
    ("stores_at_end", "C", r"first at window offset 512 \(0 past 512\)"),
    ("stores_past_declared", "C", r"byte\(s\) of \[512, 1792\) changed, the first at window offset 520"),
    ("no_zeroing", "A", None), ("no_zeroing", "B", None), ("no_zeroing", "C", None),
    ("never_refuses", "D", r"accepted fake with 256 of 512 bytes"),
    ("zeroes_before_refusing", "D", r"after stage 0 refused fake: \d+ byte\(s\) of \[0, 512\) changed"),
])
def test_workspace_checks_reject_a_half_built_driver(bug, check, message):
    fam = _FakeFamily(bug)
    run = {"A": lambda: wc.exact_and_dirty(fam, SMALL_N, "cpu"), "B": lambda: wc.shrink(fam, SMALL_N, LARGE_N, "cpu"),
           "C": lambda: wc.containment(fam, SMALL_N, LARGE_N, "cpu"), "D": lambda: wc.refusal(fam, SMALL_N, "cpu")}[check]
    with pytest.raises(AssertionError, match=message):
        run()


def test_a_store_inside_the_larger_window_is_invisible_to_shrink_but_not_to_containment():
    """B hands the driver the larger byte count, so a store 8 bytes past the smaller shape's declared end is inside what it was given;
    only C, which declares the smaller size on the same window, sees it."""
    fam = _FakeFamily("stores_past_declared")
    wc.shrink(fam, SMALL_N, LARGE_N, "cpu")
    with pytest.raises(AssertionError, match="behind the 512 bytes declared for the smaller shape"):
        wc.containment(fam, SMALL_N, LARGE_N, "cpu")


def test_a_scratch_documented_as_unused_must_be_accepted_and_left_alone():
    """unused(shape): check D then wants the short buffer accepted and not one byte of it written"""
    class Unused(_FakeFamily):
        def unused(self, n):
            return {"fake"}
    wc.refusal(Unused("never_refuses"), SMALL_N, "cpu")                # (short of its accumulators it works beside the buffer)
    with pytest.raises(_Refused):
        wc.refusal(Unused(), SMALL_N, "cpu")

    class Touches(Unused):
        def stage(self, env, n, x, state):
            ws = env.ws(_declared(n), "fake")
            if ws.numel() < _declared(n):
                ws[:4] = 0
            state["out"] = env.empty(n)
    with pytest.raises(AssertionError, match="documented as unused in this form"):
        wc.refusal(Touches("never_refuses"), SMALL_N, "cpu")


def test_a_smaller_shape_that_needs_more_bytes_gets_a_regrown_window_of_stale_data():
    """a size function need not grow with the shape: B and C then run on a new exact window that holds the old one's bytes, repeated"""
    class Inverted(_FakeFamily):
        def stage(self, env, n, x, state):                             # the fewer columns, the more bytes
            out = env.empty(n)
            self.driver(x, out, env.ws(_declared(n) + (2048 if n == SMALL_N else 0), "fake")[:_declared(n)])
            state["out"] = out
    for check in (wc.shrink, wc.containment):
        env = check(Inverted(), SMALL_N, LARGE_N, "cpu")
        assert env.regrown == {"fake"} and env.windows["fake"].nbytes == _declared(SMALL_N) + 2048
        env.assert_intact()
    with pytest.raises(AssertionError):                                # stale data is still stale there
        wc.shrink(Inverted("no_zeroing"), SMALL_N, LARGE_N, "cpu")


def test_refusal_check_sees_an_output_written_by_a_refusing_driver():
    class Writes(_FakeFamily):
        def stage(self, env, n, x, state):
            out = env.empty(n)
            ws = env.ws(_declared(n), "fake")
            if ws.numel() < _declared(n):
                out[0] = 0
            self.driver(x, out, ws)
            state["out"] = out
    wc.exact_and_dirty(Writes(), SMALL_N, "cpu")
    with pytest.raises(AssertionError, match="wrote an output"):
        wc.refusal(Writes(), SMALL_N, "cpu")
