"""tests/guardband.py on CPU tensors: an untouched buffer passes, one planted element in the lead, the tail or a row pad fails and is
located, the window round-trips, and lead % 4 == 1 really gives a 4-byte but not 16-byte aligned window."""
import numpy as np
import pytest
import torch

from guardband import SENTINEL16, SENTINEL32, SENTINEL64, Guarded


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
