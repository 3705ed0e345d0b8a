"""Device-resident siblings of guarded.In / guarded.Out for operands of gigabytes (tests/test_hip_address_limits.py): the same contract — NaN
(inputs) or the sentinel (outputs) in the guards in front of and behind the buffer and in the gaps between the rows of a pitched tensor, the
data in a column window of every row, every element outside the window bit-identical after a launch — with everything on the device:

  * the whole extent is allocated and filled there (torch.full), the window columns are written through a strided view of it;
  * value() fetches the window alone;
  * check() compares on the device, in chunks of at most CHUNK elements, every element outside the window with the fill's bit pattern (a
    refused launch: the window too, with what it held);
  * the host never holds more than the window.

BigIn / BigOut ARE guarded.In / guarded.Out (subclasses), so guarded.call, guarded.call_desc and guarded.settle take them as they are, next
to host-built buffers for the small operands of the same launch."""
import torch

import guarded
from guarded import GUARD, SENT, _dev

CHUNK = 1 << 28                  # elements compared at a time (256 M: a 1 GB slice and its 256 MB of verdicts)


def _pattern(value):
    """the int32 bit pattern of an fp32 fill value"""
    return int(torch.tensor([value], dtype=torch.float32).view(torch.int32))


def nbytes(rows, ld):
    """device bytes of a Big buffer of `rows` rows at pitch `ld`, guards included"""
    return 4 * (2 * GUARD + rows * ld)


def _window(dev, rows, ld, col0, cols):
    return dev[GUARD:GUARD + rows * ld].view(rows, ld)[:, col0:col0 + cols]


def _outside_intact(dev, rows, ld, col0, cols, pattern):
    """(in front, gaps, behind): does every element outside the column window [col0, col0 + cols) still hold `pattern`?  On the device, at
    most CHUNK elements at a time."""
    bits = dev.view(torch.int32)
    front = bool((bits[:GUARD] == pattern).all())
    behind = bool((bits[GUARD + rows * ld:] == pattern).all())
    gaps = True
    step = max(1, CHUNK // ld)
    body = bits[GUARD:GUARD + rows * ld].view(rows, ld)
    for r0 in range(0, rows, step):
        part = body[r0:r0 + step]
        for c0, c1 in ((0, col0), (col0 + cols, ld)):
            for k0 in range(c0, c1, CHUNK):              # (a single row longer than a chunk: by columns)
                gaps = gaps and bool((part[:, k0:min(k0 + CHUNK, c1)] == pattern).all())
    return front, gaps, behind


class BigIn(guarded.In):
    """device input [rows][cols] at pitch ld, built on the device: NaN in the gaps between rows and in the guards; `data` (host, any float
    dtype) are the column window [col0, col0 + cols) and the pointer is the window's"""

    def __init__(self, data, ld, col0=0):
        data = data.reshape(1, -1) if data.dim() == 1 else data.reshape(-1, data.shape[-1])
        self.rows, self.cols, self.ld, self.col0 = data.shape[0], data.shape[1], ld, col0
        assert col0 + self.cols <= ld
        self.dev = torch.full((2 * GUARD + self.rows * ld,), float("nan"), dtype=torch.float32, device=_dev())
        _window(self.dev, self.rows, ld, col0, self.cols).copy_(data.to(torch.float32).to(_dev()))
        self.ptr = self.dev.data_ptr() + 4 * (GUARD + col0)
        self.sent = data.to(torch.float32).contiguous()

    def check(self, what):
        """inputs are read only: the window still holds the data, everything else its NaN"""
        pat = _pattern(float("nan"))
        assert all(_outside_intact(self.dev, self.rows, self.ld, self.col0, self.cols, pat)), "%s wrote around an input" % what
        got = _window(self.dev, self.rows, self.ld, self.col0, self.cols).cpu()
        assert torch.equal(got.view(torch.int32), self.sent.view(torch.int32)), "%s wrote into an input" % what


class BigOut(guarded.Out):
    """device output: columns [col0, col0 + cols) of [rows] rows at pitch ld, built on the device; everything else (guards, gaps) is
    sentinel and must stay so.  prefill (host): what the window holds before the launch, else sentinel."""

    def __init__(self, rows, cols, ld, col0=0, prefill=None, at_window=False):
        self.rows, self.cols, self.ld, self.col0 = rows, cols, ld, col0
        assert col0 + cols <= ld
        self.off, self.frozen, self._host = GUARD, False, None
        self.dev = torch.full((2 * GUARD + rows * ld,), SENT, dtype=torch.float32, device=_dev())
        self.before = None                      # (the window before the launch: a host copy of the window alone, None = sentinel)
        if prefill is not None:
            self.before = prefill.reshape(rows, cols).to(torch.float32).contiguous()
            _window(self.dev, rows, ld, col0, cols).copy_(self.before.to(_dev()))
        self.ptr = self.dev.data_ptr() + 4 * (GUARD + (col0 if at_window else 0))

    def freeze(self):
        raise NotImplementedError("frozen buffers are small: guarded.Out")

    def value(self):
        return _window(self.dev, self.rows, self.ld, self.col0, self.cols).cpu()

    def check(self, what, untouched=False):
        front, gaps, behind = _outside_intact(self.dev, self.rows, self.ld, self.col0, self.cols, _pattern(SENT))
        assert front, "%s wrote in front of an output" % what
        assert behind, "%s wrote behind an output" % what
        assert gaps, "%s wrote into the gap of a pitched output" % what
        if untouched:
            got = self.value().view(torch.int32)
            ref = torch.full_like(got, _pattern(SENT)) if self.before is None else self.before.view(torch.int32)
            assert torch.equal(got, ref), "%s launched although it refused its arguments" % what
