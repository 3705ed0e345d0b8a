"""The guarded call of the direct kernel tests (tests/test_hip_pointwise.py, tests/test_hip_reductions.py, tests/test_hip_conv_launch.py, tests/test_hip_voxel_launch.py, tests/test_hip_grad_loss_launch.py, tests/test_hip_augment_launch.py, tests/test_hip_metric_launch.py): device buffers between
sentinel / NaN guards, the one way to an entry point of the C ABI, and the comparison rules of profiles/pointwise_tests_notes.md §1.

`dtype`: float32 (default), float64 (`stats`, `part`, `mean`, `rstd`), int64 (`num_batches_tracked`) or uint8 (masks: `In(..., fill=SENT_BYTE,
dtype=torch.uint8)`; workspaces: `workspace`), guards and gaps in that dtype.
`skew`: elements by which the usable pointer is moved off the 16-byte alignment that every torch allocation has."""
import ctypes as C

import torch

from rpg_ramnet_amd import _hip

F64 = torch.float64
U = 2.0 ** -24
GUARD = 256                      # elements in front of and behind every buffer
SENT = -1.2345678e29             # what outputs hold before a launch (nothing a kernel computes here)
SENT_INT = -1234567890123        # the same for integer outputs
SENT_BYTE = 0xA5                 # the same for byte buffers (masks, workspaces): non-zero, so a mask guard reads as "inside"
BADARG = 10001
TRIP2 = 524288 + 777             # items: 2048 workgroups x 256 threads = the first trip of every grid-stride loop, and a ragged second one
# maximum absolute error against float64 of sigmoidf_ over [-16, 16] and tanhf_ over [-8, 8], measured on the MI355X through
# ramnet_pred_sigmoid_fwd / ramnet_lstm_bwd (test_intrinsic_errors; profiles/pointwise_tests_notes.md)
SIGMOID_ERR = 1.07e-7            # measured 1.0601e-07
TANH_ERR = 2.18e-7               # measured 2.1799e-07
SIG_RANGE, TANH_RANGE = 16.0, 8.0


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous() if t.element_size() == 1 else t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _sentinel(dtype):
    return SENT if dtype.is_floating_point else SENT_BYTE if dtype == torch.uint8 else SENT_INT


class In:
    """device input [rows][cols] at pitch ld: NaN in the gaps between rows and in the guards"""

    def __init__(self, data, ld=None, fill=float("nan"), dtype=torch.float32, skew=0, col0=0):
        """col0: the data are the column window [col0, col0 + cols) of the rows, and the pointer is the window's"""
        data = data.reshape(1, -1) if data.dim() == 1 else data.reshape(-1, data.shape[-1])
        rows, cols = data.shape
        ld = cols if ld is None else ld
        off = GUARD + skew
        host = torch.full((2 * GUARD + skew + rows * ld,), fill, dtype=dtype)
        host[off:off + rows * ld].view(rows, ld)[:, col0:col0 + cols] = data.to(dtype)
        self.dev = host.to(_dev())
        self.ptr = self.dev.data_ptr() + host.element_size() * (off + col0)


class Out:
    """device output: columns [col0, col0 + cols) of [rows] rows at pitch ld; everything else (guards, gaps) is sentinel and must stay so.
    prefill: what the valid region holds before the launch (`+=` outputs, in-place operands); else sentinel."""

    def __init__(self, rows, cols, ld=None, col0=0, prefill=None, dtype=torch.float32, skew=0, at_window=False):
        self.rows, self.cols, self.ld, self.col0 = rows, cols, cols if ld is None else ld, col0
        self.off = GUARD + skew
        host = torch.full((2 * GUARD + skew + rows * self.ld,), _sentinel(dtype), dtype=dtype)
        if prefill is not None:
            host[self.off:self.off + rows * self.ld].view(rows, self.ld)[:, col0:col0 + cols] = prefill.reshape(rows, cols).to(dtype)
        self.before = host
        self.dev = host.to(_dev())
        self.ptr = self.dev.data_ptr() + host.element_size() * (self.off + (col0 if at_window else 0))     # (at_window: the window's own pointer)
        self._host, self.frozen = None, False

    def freeze(self):
        """what the buffer holds now (packed weights, a zeroed workspace) is what later launches must leave in place, guards and gaps included"""
        self.before = self.dev.cpu()
        self._host, self.frozen = None, True
        return self

    def _fetch(self):
        if self._host is None:
            self._host = self.dev.cpu()
        return self._host

    def value(self):
        body = self._fetch()[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)
        return body[:, self.col0:self.col0 + self.cols].contiguous()

    def check(self, what, untouched=False):
        got, ref = _bits(self._fetch()), _bits(self.before)
        n, off = self.rows * self.ld, self.off
        assert torch.equal(got[:off], ref[:off]), "%s wrote in front of an output" % what
        assert torch.equal(got[off + n:], ref[off + n:]), "%s wrote behind an output" % what
        keep = torch.ones(self.rows, self.ld, dtype=torch.bool)
        if not untouched and not self.frozen:
            keep[:, self.col0:self.col0 + self.cols] = False
        assert torch.equal(got[off:off + n].view(self.rows, self.ld)[keep], ref[off:off + n].view(self.rows, self.ld)[keep]), \
            "%s wrote into the gap of a pitched output" % what if not untouched and not self.frozen else "%s changed a frozen buffer" % what if not untouched else "%s launched although it refused its arguments" % what


def pointer_table(bufs, through_kernel=False, tail=0):
    """A device table of device pointers (`bufs`: In / Out objects or raw addresses) as a frozen int64 Out between sentinel guards: every
    later launch through `call` must leave it, its `tail` spare entries and its guards as they are.  Written by a host copy, or
    (through_kernel) by ramnet_fill_pointer_table."""
    ptrs = [b.ptr if isinstance(b, (In, Out)) else int(b) for b in bufs]
    if through_kernel:
        tab = Out(1, len(ptrs) + tail, dtype=torch.int64)
        call("ramnet_fill_pointer_table", tab, (C.c_void_p * max(len(ptrs), 1))(*ptrs), len(ptrs))
        got = tab.value().view(-1)
        assert got[:len(ptrs)].tolist() == ptrs and bool((got[len(ptrs):] == SENT_INT).all()), "ramnet_fill_pointer_table: the table is not the host array"
        return tab.freeze()
    pre = torch.full((len(ptrs) + tail,), SENT_INT, dtype=torch.int64)
    pre[:len(ptrs)] = torch.tensor(ptrs, dtype=torch.int64)
    return Out(1, len(ptrs) + tail, dtype=torch.int64, prefill=pre).freeze()


def workspace(nbytes, ticket_bytes, pattern=0xC3):
    """A workspace of EXACTLY nbytes between byte guards, 256-byte aligned: the ticket bytes zero (all a caller owes), everything behind them
    `pattern` (non-zero: a call has to write whatever else it reads).  `call` checks the guards; `tickets_zero` the tickets."""
    pre = torch.full((nbytes,), pattern, dtype=torch.uint8)
    pre[:ticket_bytes] = 0
    ws = Out(1, nbytes, dtype=torch.uint8, prefill=pre)
    assert ws.ptr % 256 == 0, "the allocator's alignment changed: the workspace is off 256 bytes"
    ws.ticket_bytes = ticket_bytes
    return ws


def tickets_zero(ws):
    return not bool(ws.value()[0, :ws.ticket_bytes].any())


def call(name, *args, rc=0, stream=None, defer=False):
    """The one way to an entry point: Buf -> pointer, NULL stream (or `stream`, a raw handle), synchronise, return code, guards and gaps.
    defer: launch only (inside a stream capture, where nothing may synchronise); `settle` does the rest after the replay."""
    L = _hip.lib()
    raw = [C.c_void_p(a.ptr) if isinstance(a, (In, Out)) else C.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a for a in args]      # (ctypes arrays, numbers, None: as they are)
    got = getattr(L, name)(*raw, None if stream is None else C.c_void_p(stream))
    if defer:
        assert got == rc, (name, got, L.ramnet_last_error())
        return
    settle(name, *args, rc=rc, got=got)


def call_desc(name, cls, fields, rc=0, also=()):
    """A descriptor entry point (ramnet_conv_launch, ramnet_conv_launch_multi, ramnet_wgrad_launch): `fields` = {field of the ctypes struct
    `cls` of rpg_ramnet_amd/_hip.py: value}, pointer fields as In / Out objects, arrays as lists; a list of such dicts = the descriptor
    array of a _multi call.  Fills the struct(s), launches on the NULL stream, synchronises and checks the return code and the guards and gaps
    of every Out among the fields and in `also`, as `call` does.  Returns the struct(s)."""
    many = isinstance(fields, (list, tuple))
    arr = (cls * (len(fields) if many else 1))()
    bufs = list(also)
    for i, f in enumerate(fields if many else [fields]):
        for k, v in f.items():
            if isinstance(v, (In, Out)):
                if isinstance(v, Out) and not any(v is b for b in bufs):
                    bufs.append(v)
                v = v.ptr
            if isinstance(v, (list, tuple)):
                a = getattr(arr[i], k)
                for j, e in enumerate(v):
                    a[j] = e
            else:
                setattr(arr[i], k, v)
    fn = getattr(_hip.lib(), name)
    got = fn(arr, len(fields), None) if many else fn(C.byref(arr[0]), None)
    settle(name, *bufs, rc=rc, got=got)
    return arr if many else arr[0]


def settle(name, *args, rc=0, got=0):
    L = _hip.lib()
    torch.cuda.synchronize()
    assert got == rc, (name, got, L.ramnet_last_error())
    if rc != 0:
        assert b"bad argument" in L.ramnet_last_error()
    for a in args:
        if isinstance(a, Out):
            a._host = None
            a.check(name, untouched=rc != 0)


def rn(*shape, seed, scale=1.0):
    """random normal, fp32-representable, as float64"""
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(F64)


def ri(*shape, seed, m):
    """integer-valued in [-m, m], as float64"""
    return torch.randint(-m, m + 1, shape, generator=torch.Generator().manual_seed(seed)).to(F64)


def assert_bits(got, ref, what):
    """the fp32 rounding of the float64 statement, bit for bit"""
    ref = ref.reshape(got.shape).to(got.dtype)
    bad = _bits(got) != _bits(ref)
    assert not bool(bad.any()), "%s: %d of %d elements differ, first at %s" % (what, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())


def assert_exact(got, ref, what, abs_sum=None):
    """integer-valued data: the float64 statement is a multiple of 1/16 with every partial sum below 2^24 (abs_sum: the statement on
    absolute values), so the fp32 result equals it exactly (an fp64 result: below 2^53)"""
    ref = ref.reshape(got.shape)
    top = ref.abs() if abs_sum is None else abs_sum
    limit = 2 ** 24 if got.dtype == torch.float32 else 2 ** 53
    assert float(top.max()) * 16 < limit and torch.equal(ref * 16, (ref * 16).round()), "%s: the case is not exact in fp32" % what
    bad = got.double() != ref
    assert not bool(bad.any()), "%s: %d of %d elements differ, first at %s: %r != %r" % (
        what, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), float(got[bad][0]), float(ref[bad][0]))


def assert_within(got, ref, bound, what):
    ref, bound = ref.reshape(got.shape), bound.reshape(got.shape)
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s: max |err| %.3e, max err / bound %.3f" % (what, float(err.max()) if err.numel() else 0.0, ratio))
    assert bool((err <= bound).all()) and bool(torch.isfinite(got).all()), "%s: error %.3f x its bound" % (what, ratio)
