"""Guard bands around caller-owned device buffers (a helper of tests/test_gpu_guard_caller.py, imported like
reduce_numpy.py and prox_numpy.py).

An Arena is ONE float64 device tensor filled with the sentinel 0x7FF8A5A5A5A5A5A5 -- a quiet NaN with a payload, compared
through an int64 view and never as a float.  carve / carve2d cut the buffers of a call out of it, each with a band of
sentinel in front of it and behind it, at a chosen 16-byte phase; the gap columns [cols, ld) of a matrix hold the
sentinel too.  snapshot() before the call, check() behind it: every double of the arena outside the views named writable
must still have the bits it had -- bands, gaps and the inputs alike -- and an output that its entry point writes whole
must hold no sentinel any more.  A store past a buffer shows up as a damaged band; a load past a buffer that reaches the
result shows up as a NaN or as bits that differ from the same call on plain tensors.  Nothing here can fault: every
band lies inside the arena's own allocation.
"""
import numpy as np
import torch

SENTINEL_U64 = 0x7FF8A5A5A5A5A5A5
SENTINEL = SENTINEL_U64 - (1 << 64) if SENTINEL_U64 >= (1 << 63) else SENTINEL_U64     # as the int64 view shows it
VEC_BAND = 1024


def matrix_band(ld):
    """a whole stray 64-row tile row of a matrix with this leading dimension, and the vector band"""
    return 64 * int(ld) + VEC_BAND


def _fill(t, data):
    """copy an input (a NumPy array or a tensor on either side) into a carved view"""
    if data is None:
        return
    src = data if isinstance(data, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(data, dtype=np.float64))
    assert src.dtype == torch.float64 and src.numel() == t.numel()
    t.copy_(src.reshape(t.shape))


class View:
    """One carved buffer: `t` is the tensor handed to the call (1-D of `count`, or rows x cols with stride ld)."""

    def __init__(self, name, off, rows, cols, ld, band, t):
        self.name, self.off, self.rows, self.cols, self.ld, self.band, self.t = name, off, rows, cols, ld, band, t
        self.span = (rows - 1) * ld + cols          # doubles from the first element to the last

    @property
    def ptr(self):
        return self.t.data_ptr()

    def mask_into(self, mask, value):
        """mark the view's own elements (not its gaps)"""
        if self.ld == self.cols or self.rows == 1:
            mask[self.off:self.off + self.span] = value
        else:
            m = torch.as_strided(mask, (self.rows, self.cols), (self.ld, 1), self.off)
            m[...] = value


class GuardError(AssertionError):
    def __init__(self, msg, name=None, side=None, offset=None):
        super().__init__(msg)
        self.name, self.side, self.offset = name, side, offset


class Arena:
    """Arena(doubles): allocated at once, the views are usable as they are carved.  Arena(): sized by its carves -- the
    offsets are laid out as the carves come, the tensor is allocated, filled and the inputs copied in by snapshot(),
    and only from then on do the views have a tensor and an address."""

    def __init__(self, doubles=None, device="cuda"):
        self.device = device
        self.buf = self.bits = self.snap = None
        self.cursor = 0
        self.views = []
        self.pending = []                           # (view, data) of a lazily sized arena
        if doubles is not None:
            self._allocate(int(doubles))

    def _allocate(self, doubles):
        self.buf = torch.empty(doubles + 2, dtype=torch.float64, device=self.device)
        assert self.buf.data_ptr() % 16 == 0
        self.bits = self.buf.view(torch.int64)
        self.bits.fill_(SENTINEL)

    # ------------------------------------------------------------------ carving
    def _place(self, span, skew, band, name):
        assert skew in (0, 1) and band >= VEC_BAND
        start = self.cursor + band
        start += (start & 1) ^ skew                 # even offset: 16-byte boundary; odd: 8 modulo 16
        end = start + span + band
        assert self.bits is None or end <= self.bits.numel(), \
            "arena too small for %s: %d > %d" % (name, end, self.bits.numel())
        self.cursor = end
        return start

    def _attach(self, v, skew, data):
        if self.buf is None:
            self.pending.append((v, skew, data))
        else:
            v.t = self.buf[v.off:v.off + v.cols] if v.rows == 1 else \
                torch.as_strided(self.buf, (v.rows, v.cols), (v.ld, 1), v.off)
            assert v.t.data_ptr() % 16 == 8 * skew
            _fill(v.t, data)
        self.views.append(v)
        return v

    def carve(self, count, data=None, skew=0, band=VEC_BAND, name=None):
        """a view of `count` doubles (data copied in, else left as sentinel) between two bands of >= `band` doubles"""
        count = int(count)
        name = name or "view%d" % len(self.views)
        band = max(int(band), VEC_BAND)
        off = self._place(count, skew, band, name)
        return self._attach(View(name, off, 1, count, count, band, None), skew, data)

    def carve2d(self, rows, cols, ld, data=None, skew=0, band=None, name=None):
        """rows x cols with leading dimension ld >= cols; the gap columns keep the sentinel and count as band"""
        rows, cols, ld = int(rows), int(cols), int(ld)
        assert ld >= cols >= 1 and rows >= 1
        name = name or "view%d" % len(self.views)
        band = max(int(band or 0), matrix_band(ld))
        off = self._place((rows - 1) * ld + cols, skew, band, name)
        return self._attach(View(name, off, rows, cols, ld, band, None), skew, data)

    # ------------------------------------------------------------------ checking
    def snapshot(self):
        if self.buf is None:                        # sized by its carves: everything is carved by now
            self._allocate(self.cursor)
            pending, self.pending, self.views = self.pending, [], []
            for v, skew, data in pending:
                self._attach(v, skew, data)
        torch.cuda.synchronize()
        self.snap = self.bits.clone()

    def _locate(self, idx):
        """(view, side, offset from the view's first double) of arena index idx"""
        for v in self.views:
            if v.off <= idx < v.off + v.span:
                col = (idx - v.off) % v.ld
                return v, ("gap" if col >= v.cols else "inside"), idx - v.off
        best = None
        for v in self.views:
            if idx < v.off:
                cand = (v.off - idx, v, "front")
            else:
                cand = (idx - (v.off + v.span) + 1, v, "behind")
            if best is None or cand[0] < best[0]:
                best = cand
        if best is None:
            return None, "arena", idx
        return best[1], best[2], idx - best[1].off

    def damage(self, writable=()):
        """None, or (view name, side, offset, arena index, count) of the first double outside the writable views
        that no longer has its snapshot bits.  side: front / behind / gap / inside (a view not named writable)."""
        assert self.snap is not None, "snapshot() first"
        torch.cuda.synchronize()
        changed = self.bits != self.snap
        for v in writable:
            v.mask_into(changed, False)
        count = int(changed.sum().item())
        if count == 0:
            return None
        idx = int(torch.nonzero(changed)[0].item())
        v, side, off = self._locate(idx)
        return (v.name if v is not None else None), side, off, idx, count

    def check(self, writable=(), whole=()):
        """raise GuardError unless only `writable` views changed and every view in `whole` lost all its sentinels"""
        d = self.damage(writable)
        if d is not None:
            name, side, off, idx, count = d
            v = next((x for x in self.views if x.name == name), None)
            where = ""
            if v is not None and v.rows > 1 and side in ("gap", "inside"):
                where = " (row %d, column %d of %d x %d, ld %d)" % (off // v.ld, off % v.ld, v.rows, v.cols, v.ld)
            raise GuardError("guard: %d double(s) changed outside the writable views; first: view %r, %s, offset %+d from "
                             "its first double%s: bits %016x -> %016x"
                             % (count, name, side, off, where, self.snap[idx].item() & (2 ** 64 - 1),
                                self.bits[idx].item() & (2 ** 64 - 1)), name, side, off)
        for v in whole:
            left = v.t.view(torch.int64) if v.rows == 1 else \
                torch.as_strided(self.bits, (v.rows, v.cols), (v.ld, 1), v.off)
            hit = left == SENTINEL
            n = int(hit.sum().item())
            if n:
                first = torch.nonzero(hit.reshape(-1))[0].item()
                r, c = divmod(int(first), v.cols)
                raise GuardError("guard: view %r is written whole by its entry point, but %d sentinel(s) remain; first at "
                                 "offset %d (row %d, column %d)" % (v.name, n, r * v.ld + c, r, c),
                                 v.name, "unwritten", r * v.ld + c)

    def row(self, v, i):
        """row i of a carved matrix as a view of its own (to name single rows writable)"""
        return View("%s[%d]" % (v.name, i), v.off + i * v.ld, 1, v.cols, v.cols, v.band, v.t[i])

    def bits_of(self, v):
        return bits_of(v)


def bits_of(v):
    """host int64 copy of a view's elements, row after row (bit-for-bit comparisons)"""
    torch.cuda.synchronize()
    t = v.t if v.rows == 1 else v.t.contiguous()
    return t.view(torch.int64).reshape(-1).cpu().numpy().copy()


class Plain:
    """The same interface on ordinary torch allocations, one per buffer, always 16-byte aligned, with nothing checked:
    the unbanded call that the arena's results are compared with.  Outputs and gaps start as the sentinel here too, so
    that a double no call writes compares equal."""

    def __init__(self, device="cuda"):
        self.device = device
        self.views = []

    def carve(self, count, data=None, skew=0, band=VEC_BAND, name=None):
        return self.carve2d(1, count, count, data, 0, band, name)

    def carve2d(self, rows, cols, ld, data=None, skew=0, band=None, name=None):
        rows, cols, ld = int(rows), int(cols), int(ld)
        span = (rows - 1) * ld + cols
        buf = torch.empty(span, dtype=torch.float64, device=self.device)
        buf.view(torch.int64).fill_(SENTINEL)
        t = buf if rows == 1 else torch.as_strided(buf, (rows, cols), (ld, 1), 0)
        _fill(t, data)
        v = View(name or "view%d" % len(self.views), 0, rows, cols, ld, 0, t)
        self.views.append(v)
        return v

    def row(self, v, i):
        return View("%s[%d]" % (v.name, i), i * v.ld, 1, v.cols, v.cols, 0, v.t[i])

    def snapshot(self):
        pass

    def check(self, writable=(), whole=()):
        torch.cuda.synchronize()

    def bits_of(self, v):
        return bits_of(v)
