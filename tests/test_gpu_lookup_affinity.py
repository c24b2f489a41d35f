"""The queued pooled lookup with two class queues per XCD (k_pooled_vec_queued, "CU affinity").

An XCD's items are split into a FABRIC class (tables above 4 MiB, whose rows cross the fabric)
and a CACHE class (tables an XCD's L2 holds); a workgroup claims from the class it prefers and
falls back through the other heads (csrc/et_lookup.hip).  Which workgroup sums which bags must
never change a result, so every case is compared bit for bit with oracle.maplookup_prealloc —
no tolerance.  Everything goes through et_maplookup_prealloc_q on a caller-owned queue block,
whose 128 bytes must read back zero after every launch (the reset covers the whole block: both
heads of every XCD, the done counter and the padding).

With 512-byte rows "fabric" is more than 8,192 rows and "cache" at most 8,192.  The small
batches leave most XCD queues empty, so every fallback step of the claim order is taken; the odd
batches end chunks early."""
import ctypes

import numpy as np
import pytest
import torch

import embtab as et
from embtab import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

MIXED_ROWS = [8200, 20000, 9000, 4099, 300, 50, 7, 1]
ET_CODE = {np.dtype(np.float32): _lib.ET_F32, np.dtype(np.float16): _lib.ET_F16,
           np.dtype(np.float64): _lib.ET_F64}


def _tables(rows, D, dtype, seed):
    rng = np.random.default_rng(seed)
    hs = [rng.standard_normal((r, D)).astype(dtype) for r in rows]
    return hs, [torch.from_numpy(h).to(DEV) for h in hs]


def _indices(rows, B, P, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(1, r + 1, (B, P)) for r in rows]


def _block():
    return torch.zeros(_lib.ET_LOOKUP_QUEUE_BYTES // 4, dtype=torch.int32, device=DEV)


def _block_is_zero(q):
    return q.cpu().numpy().tobytes() == bytes(_lib.ET_LOOKUP_QUEUE_BYTES)


class Launch:
    """One et_maplookup_prealloc_q call over device tables `tabs` and host indices `hidx`
    (et_maplookup_prealloc when called without a queue block)."""

    def __init__(self, tabs, hidx):
        self.tabs = tabs
        self.idx = [torch.from_numpy(np.ascontiguousarray(i)).to(DEV) for i in hidx]
        self.n, self.D = len(tabs), tabs[0].shape[1]
        self.B = hidx[0].shape[0]
        self.descs = (_lib.LookupDesc * self.n)()
        for t, (A, I) in enumerate(zip(tabs, self.idx)):
            self.descs[t] = _lib.LookupDesc(A.data_ptr(), self.D, A.shape[0], self.D, I.shape[1],
                                            I.data_ptr(), I.shape[1], t * self.D, 0)
        self.code = _lib.TORCH_TO_ET[tabs[0].dtype]

    def new_dst(self):
        return torch.full((self.B, self.D * self.n), float("nan"), dtype=self.tabs[0].dtype,
                          device=DEV)

    def __call__(self, q, dst=None):
        dst = self.new_dst() if dst is None else dst
        args = (self.code, ctypes.addressof(self.descs), self.n, self.B, dst.data_ptr(),
                self.D * self.n, 0)
        if q is None:
            _lib.check(_lib.load().et_maplookup_prealloc(*args, _lib.stream_handle()))
        else:
            _lib.check(_lib.load().et_maplookup_prealloc_q(*args, q.data_ptr(),
                                                           _lib.stream_handle()))
        return dst


def _same(got, ref):
    return got.cpu().numpy().tobytes() == np.ascontiguousarray(ref).tobytes()


def _check(oracle, hs, tabs, hidx):
    q = _block()
    et.check_errors()
    got = Launch(tabs, hidx)(q)
    torch.cuda.synchronize()
    assert _block_is_zero(q)
    assert et.check_errors() == 0
    assert _same(got, oracle.maplookup_prealloc(hs, hidx))


@pytest.fixture(scope="module")
def mixed():
    return _tables(MIXED_ROWS, 128, np.float32, 70)


@pytest.mark.parametrize("B", [1, 3, 65, 257, 2000, 4099])
@pytest.mark.parametrize("P", [13, 20])
def test_mixed_classes(oracle, mixed, P, B):
    """Three fabric and five cache tables in one launch."""
    hs, tabs = mixed
    _check(oracle, hs, tabs, _indices(MIXED_ROWS, B, P, 100 * P + B))


@pytest.mark.parametrize("rows", [[1, 50, 300, 4099], [8200, 20000]], ids=["cache", "fabric"])
def test_one_class_empty(oracle, rows):
    """Only one class: no preference is possible, the one-queue schedule runs."""
    hs, tabs = _tables(rows, 128, np.float32, 71)
    _check(oracle, hs, tabs, _indices(rows, 257, 13, 72))


def test_two_tables(oracle):
    rows = [8200, 300]
    hs, tabs = _tables(rows, 128, np.float32, 73)
    _check(oracle, hs, tabs, _indices(rows, 257, 13, 74))


def test_max_tables_per_launch(oracle):
    """ET_MAX_TABLES_PER_LAUNCH = 32 tables: 6 fabric and 26 cache."""
    rows = [8200 + 100 * k for k in range(6)] + [1 + 157 * k for k in range(26)]
    assert len(rows) == _lib.ET_MAX_TABLES_PER_LAUNCH and max(rows[6:]) <= 8192
    hs, tabs = _tables(rows, 128, np.float32, 75)
    _check(oracle, hs, tabs, _indices(rows, 300, 13, 76))


def test_queue_block_reused_back_to_back(oracle, mixed):
    """20 launches on one stream with one block, five at a time without a synchronise between
    them: the block is zero and every result right after each synchronise."""
    hs, tabs = mixed
    hidx = _indices(MIXED_ROWS, 257, 13, 77)
    ref = oracle.maplookup_prealloc(hs, hidx)
    run, q = Launch(tabs, hidx), _block()
    for _ in range(4):
        outs = [run(q) for _ in range(5)]
        torch.cuda.synchronize()
        assert _block_is_zero(q)
        assert all(_same(o, ref) for o in outs)


def test_two_streams_two_blocks(oracle, mixed):
    """Two streams, each with its own block, launched alternately so that they overlap."""
    hs, tabs = mixed
    hidx = _indices(MIXED_ROWS, 2000, 13, 78)
    ref = oracle.maplookup_prealloc(hs, hidx)
    run = Launch(tabs, hidx)
    streams = [torch.cuda.Stream(DEV) for _ in range(2)]
    blocks = [_block() for _ in range(2)]
    outs = [[run.new_dst() for _ in range(10)] for _ in range(2)]
    torch.cuda.synchronize()
    for k in range(10):
        for s in range(2):
            with torch.cuda.stream(streams[s]):
                run(blocks[s], outs[s][k])
    torch.cuda.synchronize()
    assert all(_block_is_zero(b) for b in blocks)
    assert all(_same(o, ref) for per in outs for o in per)


@pytest.mark.parametrize("dtype,D,rows", [
    (np.float16, 256, MIXED_ROWS),   # the other scalar-addressed 512-byte rows
    (np.float64, 64, MIXED_ROWS),
    # 256-byte rows (k_pooled_vec_queued<SG = false>): the fabric class starts above 16,384 rows
    (np.float32, 64, [16400, 40000, 18000, 4099, 300, 50, 7, 1]),
    (np.float16, 128, [16400, 40000, 18000, 4099, 300, 50, 7, 1]),
], ids=["f16x256", "f64x64", "f32x64", "f16x128"])
def test_other_element_paths(oracle, dtype, D, rows):
    hs, tabs = _tables(rows, D, dtype, 79)
    _check(oracle, hs, tabs, _indices(rows, 257, 13, 80))


ROWS_256B = [(np.float32, 64), (np.float16, 128)]  # 256-byte rows: always the per-lane loop


@pytest.mark.parametrize("dtype,D", ROWS_256B, ids=["f32x64", "f16x128"])
def test_256_byte_rows_static_stripes(oracle, dtype, D):
    """No queue block: k_pooled_vec_striped<SG = false>.  One table above 4 MiB (16,384 rows)."""
    rows = [16400, 300, 7]
    hs, tabs = _tables(rows, D, dtype, 82)
    hidx = _indices(rows, 65, 5, 83)
    et.check_errors()
    got = Launch(tabs, hidx)(None)
    assert et.check_errors() == 0
    assert _same(got, oracle.maplookup_prealloc(hs, hidx))


@pytest.mark.parametrize("dtype,D", ROWS_256B, ids=["f32x64", "f16x128"])
def test_256_byte_rows_single_table(oracle, dtype, D):
    """One table: the linear k_pooled_vec<SG = false>."""
    hs, tabs = _tables([300], D, dtype, 84)
    hidx = _indices([300], 9, 3, 85)
    et.check_errors()
    got = Launch(tabs, hidx)(None)
    assert et.check_errors() == 0
    assert _same(got, oracle.pooled_sum(hs[0], hidx[0]))


def test_out_of_range_indices(oracle, mixed):
    """Out-of-range indices in a fabric table, a cache table and the one-row table: each is
    counted exactly once and contributes a zero row."""
    hs, tabs = mixed
    B, P = 257, 13
    hidx = _indices(MIXED_ROWS, B, P, 81)
    bad = [i.copy() for i in hidx]
    edits = [(0, B - 1, 12, MIXED_ROWS[0] + 1), (2, 0, 0, 0), (7, B // 2, 5, -1)]
    for t, j, k, v in edits:
        bad[t][j, k] = v
    q = _block()
    et.check_errors()
    got = Launch(tabs, bad)(q)
    assert et.check_errors() == len(edits)
    assert _block_is_zero(q)
    ref = oracle.maplookup_prealloc(hs, hidx)
    for t, j, k, _ in edits:
        keep = np.delete(hidx[t][j:j + 1], k, axis=1)
        ref[j, 128 * t:128 * (t + 1)] = oracle.pooled_sum(hs[t], keep)[0]
    assert _same(got, ref)
