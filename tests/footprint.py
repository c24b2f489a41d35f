"""Helpers of the memory-footprint tests (tests/test_footprint_host.py, tests/test_gpu_footprint.py):
canary-guarded allocations, byte snapshots of read-only operands and the poison patterns a
workspace is filled with before a call.  numpy and torch only; nothing here needs a GPU.

A guard is memory the test owns around the range a kernel may write, filled with CANARY: a
kernel that overruns its range changes a canary instead of someone else's memory, and the
report says where."""
import numpy as np
import torch

CANARY = 0xA5
GUARD = 65536


# --- byte ranges -------------------------------------------------------------------------------

def guarded_bytes(nbytes, shift, device, guard=GUARD):
    """One uint8 allocation filled with CANARY and the view of exactly `nbytes` bytes of it
    that starts `shift` (0..255) bytes past a 256-byte boundary, at least `guard` bytes in from
    each end: (buffer, view).  ``view.data_ptr()`` is the pointer to pass; the view's offset in
    the buffer is ``offset_in(buf, view)``."""
    assert 0 <= shift < 256 and nbytes >= 0 and guard >= 0
    buf = torch.full((guard + 256 + shift + nbytes + guard,), CANARY, dtype=torch.uint8,
                     device=device)
    lo = guard + (-(buf.data_ptr() + guard)) % 256 + shift
    view = buf[lo:lo + nbytes]
    assert (buf.data_ptr() + lo - shift) % 256 == 0 and lo + nbytes + guard <= buf.numel()
    return buf, view


def offset_in(buf, view):
    """Byte offset of `view` (a slice of `buf`) from the start of `buf`."""
    return view.data_ptr() - buf.data_ptr() if view.numel() else int(view.storage_offset())


def guards_intact(buf, lo, hi):
    """(ok, first, last): ok is True if every byte of `buf` outside [lo, hi) still holds
    CANARY.  Otherwise first and last are the first and last changed byte, relative to the
    owned range: -k is the k-th byte in front of `lo` (-1: the byte just before it), +k the
    k-th byte past the end (+1: the byte at `hi`)."""
    b = buf.reshape(-1).view(torch.uint8)
    bad = b != CANARY
    bad[lo:hi] = False
    where = torch.nonzero(bad).reshape(-1)
    if where.numel() == 0:
        return True, None, None

    def rel(o):
        return o - lo if o < lo else o - hi + 1

    return False, rel(int(where[0])), rel(int(where[-1]))


def overrun(first, last):
    """The assertion message of a guards_intact failure."""
    def say(o):
        return f"{-o} bytes before the start" if o < 0 else f"+{o} bytes past the end"

    return f"guard bytes changed from {say(first)} to {say(last)}"


def assert_guards(buf, view, what=""):
    lo = offset_in(buf, view)
    ok, first, last = guards_intact(buf, lo, lo + view.numel())
    assert ok, f"{what}: {overrun(first, last)}"


# --- matrices ----------------------------------------------------------------------------------

def guarded_matrix(rows, cols, dtype, device, pad_cols=7, guard_rows=1, ld=None, left=None):
    """A (rows, cols) strided view inside a CANARY-filled 2-D buffer: `guard_rows` rows above
    and below, `pad_cols` elements on each side of every row (row stride cols + 2 * pad_cols).
    `left` and `ld` choose the left pad and the row stride instead (a 16-byte aligned view
    with a stride that is a multiple of 16 bytes takes the kernels' vector stores).
    Returns (buffer, view, intact); intact() is (ok, where), where naming the first changed
    guard byte as (buffer row, byte column)."""
    left = pad_cols if left is None else left
    ld = cols + 2 * pad_cols if ld is None else ld
    assert ld >= left + cols
    buf = torch.empty((rows + 2 * guard_rows, ld), dtype=dtype, device=device)
    buf.view(torch.uint8).fill_(CANARY)
    view = buf[guard_rows:guard_rows + rows, left:left + cols]
    es = buf.element_size()

    def intact():
        b = buf.view(torch.uint8).view(rows + 2 * guard_rows, ld * es)
        bad = b != CANARY
        bad[guard_rows:guard_rows + rows, left * es:(left + cols) * es] = False
        where = torch.nonzero(bad)
        if where.numel() == 0:
            return True, None
        return False, (int(where[0, 0]), int(where[0, 1]))

    return buf, view, intact


# --- read-only operands ------------------------------------------------------------------------

def _bytes(t):
    if isinstance(t, np.ndarray):
        return np.ascontiguousarray(t).tobytes()
    if t.numel() == 0:
        return b""
    return t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()


def snapshot(t):
    """The bytes of a tensor (or numpy array), element by element in index order."""
    return _bytes(t)


def unchanged(t, snap):
    return _bytes(t) == snap


# --- poisons -----------------------------------------------------------------------------------

def _fill(value):
    def poison(view, leftover=None):
        view.fill_(value)

    return poison


def _random(view, leftover=None):
    g = torch.Generator().manual_seed(view.numel() + 12345)
    r = torch.randint(0, 256, (view.numel(),), dtype=torch.uint8, generator=g)
    view.copy_(r.to(view.device))


def _leftover(view, leftover=None):
    """`leftover(view)` runs the entry under test once on another problem with `view` as its
    workspace and leaves what it wrote."""
    assert leftover is not None, "the leftover poison needs the call that leaves it"
    leftover(view)


# name -> poison(view, leftover=None): fills the uint8 view in place
POISONS = {
    "zero": _fill(0x00),        # what a kernel relying on cleared slots hopes for
    "ones": _fill(0xFF),        # every counter huge, every key or index UINT32_MAX
    "canary": _fill(CANARY),
    "random": _random,
    "leftover": _leftover,
}
