"""Guard bands for kernel tests: a [rows, cols] window with row stride ld inside ONE flat allocation whose every other element --
the lead in front of the window, the tail behind it and the ld - cols pad of every row -- holds a NaN sentinel written through
an integer view.  A kernel that stores outside its output changes a sentinel and assert_intact() names the first such element; a
kernel that loads outside its input reads a NaN, which poisons the result the test compares with its reference.

    out = Guarded(R, V, ld=V + 5, lead=65, device="cuda")     # lead % 4 == 1: 4-byte, not 16-byte aligned
    rc = L.s2vt_...(src.ptr, ..., out.ptr, out.ld, ...)
    got = out.numpy(); out.assert_intact()

Index arrays that a kernel follows to an address (rowidx, video_id, sample_id) take `fill=<a valid index>`: their guards then hold
that in-range integer instead of the NaN bits, so that a read past the array can never become a wild address; assert_intact()
compares with the same value.  int64 windows (the packed pick words) are guarded with the 32-bit sentinel in both halves.
reset() puts the sentinel back into the window as well, for an output that several launches write in turn; image(rows, values) is
then what the whole allocation must hold after a launch that writes those rows of the window only, and assert_image() compares with it
in one go (rows the launch must leave alone, pads and guards alike).

GuardedWorkspace is the byte form for a driver's `void* workspace, size_t bytes`: a 256-byte aligned window of exactly nbytes between
two SENTINEL32 guards.  Its window is NOT pre-filled: a workspace holds index arrays and counters, and by the rule above a place an
index could be read from must hold a valid index -- so a test dirties the window with a real call of the same driver on other inputs,
and then runs the call under test on it.  snapshot() / assert_unchanged() compare a byte range of the window bit for bit.

A plain module (not a conftest, no fixtures); works on CPU tensors as well, where tests/test_guardband_cpu.py checks it."""
import ctypes

import numpy as np
import torch

SENTINEL32 = 0x7FC5A5A5          # an fp32 quiet NaN with a payload; the same bits serve int32 outputs
SENTINEL16 = 0x7FC5              # a bf16 (and fp16) quiet NaN with a payload
SENTINEL64 = (SENTINEL32 << 32) | SENTINEL32      # 8-byte elements: the 32-bit sentinel twice
MIN_GUARD = 64                   # elements in front of and behind the window, at least

_INT_VIEW = {8: (torch.int64, SENTINEL64), 4: (torch.int32, SENTINEL32), 2: (torch.int16, SENTINEL16)}


class Guarded:
    def __init__(self, rows, cols, ld=None, dtype=torch.float32, lead=MIN_GUARD, tail=MIN_GUARD, device="cuda", name="buffer", fill=None):
        ld = cols if ld is None else int(ld)
        assert rows >= 1 and cols >= 1 and ld >= cols, (rows, cols, ld)
        assert lead >= MIN_GUARD and tail >= MIN_GUARD, "guards are at least 64 elements"
        self.rows, self.cols, self.ld, self.lead, self.tail, self.dtype, self.name = rows, cols, ld, int(lead), int(tail), dtype, name
        self._itype, self._sentinel = _INT_VIEW[torch.empty(0, dtype=dtype).element_size()]
        if fill is not None:                                             # an index array: guards of a valid index, not of NaN bits
            assert dtype in (torch.int32, torch.int64) and int(fill) == fill, "fill= is for integer index arrays"
            self._sentinel = int(fill)
        n = self.lead + rows * ld + self.tail
        self._buf = torch.empty(n, dtype=dtype, device=device)
        assert self._buf.data_ptr() % 16 == 0, "the allocator's base is 16-byte aligned: `lead` alone sets the window's alignment"
        self._ibuf = self._buf.view(self._itype)
        self._ibuf.fill_(self._sentinel)
        self.view = self._buf[self.lead:self.lead + rows * ld].view(rows, ld)[:, :cols]
        self._iview = self._ibuf[self.lead:self.lead + rows * ld].view(rows, ld)[:, :cols]

    @classmethod
    def of(cls, array, ld=None, **kw):
        """A guarded copy of a 1-D ([1, n] window) or 2-D array / tensor (inputs are guarded the same way as outputs)."""
        t = torch.as_tensor(np.ascontiguousarray(array) if isinstance(array, np.ndarray) else array)
        t = t.reshape(1, -1) if t.dim() <= 1 else t.reshape(t.shape[0], -1)
        g = cls(t.shape[0], t.shape[1], ld=ld, dtype=kw.pop("dtype", t.dtype), **kw)
        g.fill(t)
        return g

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    @property
    def aligned16(self):
        return self.view.data_ptr() % 16 == 0

    def fill(self, array):
        """Write the window only."""
        t = torch.as_tensor(np.ascontiguousarray(array) if isinstance(array, np.ndarray) else array)
        self.view.copy_(t.reshape(self.rows, self.cols).to(self.dtype))
        return self

    def reset(self):
        """The sentinel everywhere, the window included: an element the next launch does not write then shows in bits()."""
        self._ibuf.fill_(self._sentinel)
        return self

    def numpy(self):
        """The window as a host array (bf16 as its uint16 bits)."""
        if self.dtype == torch.bfloat16:
            return self._iview.cpu().numpy().view(np.uint16)
        return self.view.cpu().numpy()

    def bits(self):
        """The window's bit patterns as a host integer array."""
        return self._iview.cpu().numpy()

    def image(self, rows=None, values=None):
        """The bits of the WHOLE allocation after reset() and a launch that wrote `values` ([len(rows), cols] floats, or integers given as
        their bits) into the window's `rows` and nothing else -- sentinels everywhere else, the window's other rows included."""
        img = torch.full_like(self._ibuf, self._sentinel)
        if rows is not None and len(rows):
            v = np.ascontiguousarray(values)
            itype = {8: np.int64, 4: np.int32, 2: np.int16}[img.element_size()]
            v = v.view(itype) if v.dtype.itemsize == img.element_size() else v.astype(itype)
            v = torch.as_tensor(v).reshape(len(rows), self.cols).to(img.device)
            win = img[self.lead:self.lead + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]
            win[torch.as_tensor(np.asarray(rows, np.int64), device=img.device)] = v
        return img

    def assert_image(self, img, what=""):
        """The allocation holds exactly img (one comparison on the device); names the first element that does not."""
        if torch.equal(self._ibuf, img):
            return
        diff = self._ibuf != img
        off = int(diff.nonzero()[0, 0])
        rel = off - self.lead
        inside = 0 <= rel < self.rows * self.ld and rel % self.ld < self.cols
        where = f"window row {rel // self.ld}, column {rel % self.ld}" if inside else self._where(off)
        raise AssertionError(f"{self.name} {what}: {int(diff.sum())} element(s) differ, the first at flat offset {off}: {where}; "
                             f"bits {int(self._ibuf[off]):#x}, expected {int(img[off]):#x} (sentinel {self._sentinel:#x})")

    def _where(self, off):
        if off < self.lead:
            return f"lead guard, {self.lead - off} element(s) in front of the window"
        rel = off - self.lead
        if rel >= self.rows * self.ld:
            return f"tail guard, {rel - self.rows * self.ld} element(s) behind the last row's pad"
        return f"pad of row {rel // self.ld}, column {rel % self.ld} (cols = {self.cols}, ld = {self.ld})"

    def assert_intact(self):
        """Every element outside the window still holds the sentinel bits."""
        changed = self._ibuf != self._sentinel
        changed[self.lead:self.lead + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = False
        if bool(changed.any()):
            off = int(changed.nonzero()[0, 0])
            got = int(self._ibuf[off]) & {torch.int64: 0xFFFFFFFFFFFFFFFF, torch.int32: 0xFFFFFFFF, torch.int16: 0xFFFF}[self._itype]
            raise AssertionError(f"{self.name}: write outside the window at flat offset {off} (window starts at {self.lead}): "
                                 f"{self._where(off)}; bits {got:#x}, sentinel {self._sentinel:#x}; {int(changed.sum())} element(s) changed")


WS_ALIGN = 256                   # what every driver asks of its workspace pointer (S2VT_E_ALIGN otherwise)
WS_MIN_LEAD = 256                # guard bytes in front of the window, at least
WS_MIN_TAIL = 4096               # guard bytes behind it, at least


class GuardedWorkspace:
    """One flat uint8 allocation: [lead guard | window of exactly nbytes, 256-byte aligned | tail guard], guards of SENTINEL32 words."""

    def __init__(self, nbytes, device="cuda", name="workspace", tail=WS_MIN_TAIL):
        nbytes = int(nbytes)
        assert nbytes > 0 and nbytes % WS_ALIGN == 0, f"{name}: a workspace size is a positive multiple of 256 bytes, got {nbytes}"
        assert tail >= WS_MIN_TAIL and tail % 4 == 0
        self.nbytes, self.name, self.tail = nbytes, name, int(tail)
        self._buf = torch.empty(WS_MIN_LEAD + WS_ALIGN + nbytes + self.tail, dtype=torch.uint8, device=device)
        base = self._buf.data_ptr()
        assert base % 4 == 0
        self.lead = WS_MIN_LEAD + (-(base + WS_MIN_LEAD)) % WS_ALIGN          # the lead that puts the window on a 256-byte boundary
        self._buf = self._buf[:self.lead + nbytes + self.tail]
        self._front = self._buf[:self.lead].view(torch.int32)
        self._back = self._buf[self.lead + nbytes:].view(torch.int32)
        self._front.fill_(SENTINEL32)
        self._back.fill_(SENTINEL32)
        self.window = self._buf[self.lead:self.lead + nbytes]
        assert self.window.data_ptr() % WS_ALIGN == 0 and self.lead >= WS_MIN_LEAD and self.window.numel() == nbytes

    @property
    def ptr(self):
        return ctypes.c_void_p(self.window.data_ptr())

    def as_uint8(self, nbytes=None):
        """The window (or its first nbytes) as a uint8 tensor: what the ws= parameters of ops take, numel() being the byte count they pass."""
        return self.window if nbytes is None else self.window[:int(nbytes)]

    def assert_intact(self):
        """Both guards still hold the sentinel; names the byte offset, relative to the window, of the first word that does not."""
        for words, start, label in ((self._back, self.nbytes, "behind the window's end"), (self._front, -self.lead, "in front of the window")):
            bad = words != SENTINEL32
            if bool(bad.any()):
                i = int(bad.nonzero()[0, 0])
                off = start + 4 * i
                dist = off - self.nbytes if start >= 0 else -off
                raise AssertionError(f"{self.name}: write outside the {self.nbytes}-byte window at window offset {off} ({dist} byte(s) {label}); "
                                     f"bits {int(words[i]) & 0xFFFFFFFF:#x}, sentinel {SENTINEL32:#x}; {int(bad.sum())} word(s) changed")

    def snapshot(self):
        return self.window.clone()

    def assert_unchanged(self, snapshot, lo=0, hi=None, what=""):
        """Bytes [lo, hi) of the window equal the snapshot's (one comparison on the device); names the first offset that differs."""
        hi = self.nbytes if hi is None else int(hi)
        assert 0 <= lo <= hi <= self.nbytes and snapshot.numel() == self.nbytes
        if lo == hi or torch.equal(self.window[lo:hi], snapshot[lo:hi]):
            return
        diff = self.window[lo:hi] != snapshot[lo:hi]
        off = lo + int(diff.nonzero()[0, 0])
        raise AssertionError(f"{self.name} {what}: {int(diff.sum())} byte(s) of [{lo}, {hi}) changed, the first at window offset {off} "
                             f"({off - lo} past {lo}): {int(self.window[off]):#04x}, was {int(snapshot[off]):#04x}")
