"""The footprint helpers can fail, and the host side of the workspace contract.

Part 1: every helper of tests/footprint.py rejects a one-byte (or one-bit) violation, on CPU
tensors.  Part 2: the "workspace one byte short" rule for the entries tests/test_abi.py and
tests/test_adagrad_host.py leave out: et_index_build, et_ragged_sgd, et_weighted_sgd,
et_sparse_sgd_snap and the two phase flags.  As there, the status codes come back before any
device work, so the dummy pointers are never dereferenced."""
import ctypes
import re

import numpy as np
import pytest
import torch

import footprint as fp

CPU = torch.device("cpu")


# --- 1. the helpers ---------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [0, 4, 100, 255])
def test_guarded_bytes_layout(shift):
    buf, view = fp.guarded_bytes(1000, shift, CPU, guard=4096)
    lo = fp.offset_in(buf, view)
    assert view.numel() == 1000 and view.data_ptr() % 256 == shift
    assert lo >= 4096 and buf.numel() - (lo + 1000) >= 4096
    assert bool((buf == fp.CANARY).all())
    assert fp.guards_intact(buf, lo, lo + 1000) == (True, None, None)
    view.fill_(0)  # the owned range may hold anything
    assert fp.guards_intact(buf, lo, lo + 1000)[0]
    fp.assert_guards(buf, view)


def test_guards_intact_reports_one_flipped_byte():
    buf, view = fp.guarded_bytes(512, 100, CPU, guard=1024)
    lo = fp.offset_in(buf, view)
    hi = lo + 512
    end = buf.numel()
    # the four borders: the buffer's first and last byte, the byte just before lo and the byte
    # at hi; and the alignment slack in front of a shifted workspace (the 100 bytes between the
    # 256-byte boundary and lo)
    cases = {0: -lo, end - 1: end - hi, lo - 1: -1, hi: 1, lo - 100: -100, lo - 57: -57,
             hi + 11: 12}
    for o, rel in cases.items():
        old = int(buf[o])
        buf[o] = old ^ 1
        ok, first, last = fp.guards_intact(buf, lo, hi)
        assert not ok and first == last == rel, (o, first, last)
        with pytest.raises(AssertionError, match="guard bytes changed"):
            fp.assert_guards(buf, view, "case")
        buf[o] = old
        assert fp.guards_intact(buf, lo, hi)[0]
    # the first and last owned byte are no violation
    buf[lo] = 0
    buf[hi - 1] = 0
    assert fp.guards_intact(buf, lo, hi)[0]
    # two violations: the first and the last are named
    buf[lo - 3] = 0
    buf[hi + 11] = 0
    assert fp.guards_intact(buf, lo, hi) == (False, -3, 12)
    assert fp.overrun(-3, 12) == ("guard bytes changed from 3 bytes before the start to "
                                  "+12 bytes past the end")


def test_guarded_matrix_reports_a_pad_column_inside_the_rows():
    # dim 20 in rows of ld 24, 16-byte aligned: the sixth 16-byte store of a row that rounds
    # dim up to 24 writes elements 20..23, the pad
    buf, view, intact = fp.guarded_matrix(5, 20, torch.float32, CPU, guard_rows=2, ld=24, left=0)
    assert view.shape == (5, 20) and view.stride() == (24, 1) and buf.shape == (9, 24)
    assert intact() == (True, None)
    view.fill_(1.0)
    assert intact()[0]
    raw = buf.view(torch.uint8).view(9, 96)
    raw[4, 80] ^= 1  # row 2 of the view, element 20: the first pad byte
    assert intact() == (False, (4, 80))
    raw[4, 80] ^= 1
    for r, c in ((1, 5), (7, 0), (2, 95), (6, 80), (0, 0), (8, 95)):  # guard rows, pads, corners
        raw[r, c] ^= 0x80
        assert intact() == (False, (r, c))
        raw[r, c] ^= 0x80
    assert intact()[0]
    # the symmetric form: 7 elements on each side, one guard row
    buf, view, intact = fp.guarded_matrix(3, 20, torch.float16, CPU)
    assert buf.shape == (5, 34) and view.data_ptr() - buf.data_ptr() == (34 + 7) * 2
    raw = buf.view(torch.uint8).view(5, 68)
    for r, c in ((1, 13), (1, 54), (3, 67), (0, 30), (4, 30)):
        raw[r, c] = 0
        assert intact() == (False, (r, c))
        raw[r, c] = fp.CANARY
    assert intact()[0]


def test_poisons_produce_what_they_claim():
    assert list(fp.POISONS) == ["zero", "ones", "canary", "random", "leftover"]
    buf, view = fp.guarded_bytes(4096, 4, CPU, guard=256)
    lo = fp.offset_in(buf, view)
    for name, value in (("zero", 0), ("ones", 0xFF), ("canary", 0xA5)):
        fp.POISONS[name](view)
        assert bool((view == value).all()), name
    assert int(view.view(torch.int32)[5]) & 0xFFFFFFFF == 0xA5A5A5A5
    fp.POISONS["ones"](view)
    assert int(view.view(torch.int32)[0]) == -1  # UINT32_MAX as a counter, a key, an index
    fp.POISONS["random"](view)
    first = view.clone()
    counts = torch.bincount(view.to(torch.int64), minlength=256)
    assert int((counts > 0).sum()) > 250 and int(counts.max()) < 64  # no constant fill
    fp.POISONS["zero"](view)
    fp.POISONS["random"](view)
    assert torch.equal(view, first)  # seeded
    seen = []

    def other_problem(v):
        seen.append((v.data_ptr(), v.numel()))
        v[:100] = 7

    fp.POISONS["leftover"](view, other_problem)
    assert seen == [(view.data_ptr(), 4096)]
    assert bool((view[:100] == 7).all()) and torch.equal(view[100:], first[100:])
    with pytest.raises(AssertionError):
        fp.POISONS["leftover"](view)
    assert fp.guards_intact(buf, lo, lo + 4096)[0]  # a poison fills its range only


def test_unchanged_rejects_one_bit():
    t = torch.arange(24, dtype=torch.float32).reshape(4, 6)[:, 1:5]  # a strided view
    snap = fp.snapshot(t)
    assert fp.unchanged(t, snap)
    t.view(torch.int32)[2, 3] ^= 1
    assert not fp.unchanged(t, snap)
    t.view(torch.int32)[2, 3] ^= 1
    assert fp.unchanged(t, snap)
    h = torch.zeros(3, dtype=torch.bfloat16)
    snap = fp.snapshot(h)
    h.view(torch.int16)[1] = -32768  # -0.0: equal as a number, not as bytes
    assert bool((h == 0).all()) and not fp.unchanged(h, snap)
    a = np.zeros(5, np.int64)
    snap = fp.snapshot(a)
    a[4] = 1
    assert not fp.unchanged(a, snap)


# --- 2. one byte short, and NULL, for the entries the other host tests leave out ----------------

P = 1 << 20  # dummy device addresses
BASES = ((1 << 24, 0), ((1 << 24) + 1, 255), ((1 << 24) + 192, 64))  # (workspace, pad to 256)


def _expect_workspace_error(L, call, size):
    """`call(ptr, nbytes)`: a workspace `pad` bytes before a 256-byte boundary needs
    size - 256 + pad bytes; one less is ET_ERR_WORKSPACE naming that number; so is NULL."""
    for base, pad in BASES:
        need = size - 256 + pad
        assert call(ctypes.c_void_p(base), need - 1) == -3, (base, L.et_last_error())
        assert re.search(rb"\b%d bytes" % need, L.et_last_error()), (base, need, L.et_last_error())
        assert call(ctypes.c_void_p(base), 0) == -3
    assert call(None, size) == -3 and b"workspace" in L.et_last_error()
    assert call(None, 1 << 40) == -3


def test_index_build_workspace_one_byte_short():
    from embtab import _lib

    L = _lib.load()
    for pool, batch in ((1, 1), (1, 1000), (20, 300), (3, 4097)):
        nb = ctypes.c_int64(0)
        assert L.et_index_workspace_size(pool * batch, ctypes.byref(nb)) == 0

        def call(ws, nbytes):
            return L.et_index_build(P, pool, pool, batch, 500, 2 * P, 3 * P, 4 * P, 5 * P, ws,
                                    nbytes, None)

        _expect_workspace_error(L, call, nb.value)


def _ragged_descs(_lib, weighted, shapes):
    cls = _lib.WeightedUpdateDesc if weighted else _lib.RaggedUpdateDesc
    arr = (cls * len(shapes))()
    for t, (nrows, dim, nnz, batch) in enumerate(shapes):
        args = [P, dim, nrows, dim, 0, 2 * P, dim, 3 * P, nnz, 4 * P, batch, 0]
        arr[t] = cls(*(args + [5 * P, 0] if weighted else args))
    return arr


RAGGED_SHAPES = {
    "one entry": [(10, 16, 1, 1)],
    "one table": [(700, 128, 3000, 257)],
    "two tables, one without entries": [(700, 20, 5000, 300), (50, 7, 0, 300)],
    "three tables": [(100, 64, 257, 64), (1000, 16, 4096, 1000), (5, 128, 8193, 2)],
}


@pytest.mark.parametrize("weighted", [False, True])
def test_ragged_and_weighted_sgd_workspace_one_byte_short(weighted):
    from embtab import _lib

    L = _lib.load()
    size_of = L.et_weighted_sgd_workspace_size if weighted else L.et_ragged_sgd_workspace_size
    entry = L.et_weighted_sgd if weighted else L.et_ragged_sgd
    for name, shapes in RAGGED_SHAPES.items():
        d = _ragged_descs(_lib, weighted, shapes)
        nb = ctypes.c_int64(0)
        assert size_of(ctypes.addressof(d), len(shapes), ctypes.byref(nb)) == 0, name
        # the two entries share one layout: the same sizes cost the same
        other = _ragged_descs(_lib, not weighted, shapes)
        nb2 = ctypes.c_int64(0)
        f2 = L.et_ragged_sgd_workspace_size if weighted else L.et_weighted_sgd_workspace_size
        assert f2(ctypes.addressof(other), len(shapes), ctypes.byref(nb2)) == 0
        assert nb.value == nb2.value > 4 * sum(s[2] for s in shapes)
        for dtype in (_lib.ET_F32, _lib.ET_BF16):
            for flags in (0, _lib.ET_FLAG_NONTEMPORAL | _lib.ET_FLAG_SGD_UNFUSED):
                def call(ws, nbytes):
                    return entry(dtype, ctypes.addressof(d), len(shapes), 0.1, flags, ws, nbytes,
                                 None)

                _expect_workspace_error(L, call, nb.value)


SGD_SHAPES = {
    "early-chain rows beside a regular table": [(100, 16, 3, 1000), (3000, 64, 20, 128)],
    "hot-shaped": [(1000, 128, 20, 1500)],
    "one occurrence": [(10, 8, 1, 1)],
}


def _sgd_descs(_lib, shapes, delta=2 * P):
    return (_lib.UpdateDesc * len(shapes))(*[
        _lib.UpdateDesc(P, dim, nrows, dim, pool, delta, dim, 3 * P, pool, batch, 0)
        for nrows, dim, pool, batch in shapes])


def test_snap_and_phase_flags_workspace_one_byte_short():
    from embtab import _lib

    L = _lib.load()
    for name, shapes in SGD_SHAPES.items():
        n = len(shapes)
        d = _sgd_descs(_lib, shapes)
        nb = ctypes.c_int64(0)
        assert L.et_sgd_workspace_size(ctypes.addressof(d), n, ctypes.byref(nb)) == 0
        snaps = (ctypes.c_void_p * n)(*[6 * P + t * P for t in range(n)])
        nosnaps = (ctypes.c_void_p * n)()
        for mode in (0, _lib.ET_FLAG_EXACT_UPDATE, _lib.ET_FLAG_SGD_HOT_PASS):
            for sn in (snaps, nosnaps):
                def call(ws, nbytes):
                    return L.et_sparse_sgd_snap(_lib.ET_F32, ctypes.addressof(d), n, 0.1, mode,
                                                ctypes.addressof(sn), ws, nbytes, None)

                _expect_workspace_error(L, call, nb.value)
            for phase in (_lib.ET_FLAG_SGD_INDEX_ONLY, _lib.ET_FLAG_SGD_APPLY_ONLY):
                def call(ws, nbytes):
                    return L.et_sparse_sgd(_lib.ET_F32, ctypes.addressof(d), n, 0.1, mode | phase,
                                           ws, nbytes, None)

                _expect_workspace_error(L, call, nb.value)

                def call_snap(ws, nbytes):
                    return L.et_sparse_sgd_snap(_lib.ET_F32, ctypes.addressof(d), n, 0.1,
                                                mode | phase, ctypes.addressof(snaps), ws, nbytes,
                                                None)

                _expect_workspace_error(L, call_snap, nb.value)
        # the index phase takes a NULL gradient and needs the same workspace
        d0 = _sgd_descs(_lib, shapes, delta=0)

        def call_null(ws, nbytes):
            return L.et_sparse_sgd(_lib.ET_F32, ctypes.addressof(d0), n, 0.1,
                                   _lib.ET_FLAG_SGD_INDEX_ONLY, ws, nbytes, None)

        _expect_workspace_error(L, call_null, nb.value)
    # a NULL snapshot list is an argument error, before the workspace is looked at
    d = _sgd_descs(_lib, SGD_SHAPES["one occurrence"])
    assert L.et_sparse_sgd_snap(_lib.ET_F32, ctypes.addressof(d), 1, 0.1, 0, None, None, 0,
                                None) == -1
