"""Item order of the queued pooled lookup's class queues (csrc/et_lookup_order.h, DESIGN §4
"L2 order"): whatever order an XCD's queues hand their items out in, every item is claimed
exactly once, so every case is compared bit for bit with oracle.maplookup_prealloc.  The
destination is pre-filled with NaN (an unclaimed item shows), the caller's 128-byte queue block
must be zero after every launch, and check_errors() == 0.

Shapes: the smallest where a table-major or two-phase order differs from the static one and every
phase exists.  fp32 x 128 (512-byte rows): 524,300 rows is above 256 MiB (non-temporal phase),
20,000 / 9,000 / 8,200 rows are the allocating fabric tables, 4,099 and 3,000 rows are cache
tables above 1 MiB and 50 and 3 rows below.  B = 4099 gives stripe_chunks = 65 with empty slots in
the last stripe; the small batches leave most queues empty, so every fallback claim is taken."""
import ctypes

import numpy as np
import pytest
import torch

import embtab as et
from embtab import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

ROWS = [524300, 20000, 9000, 8200, 4099, 3000, 50, 3]


def _tables(rows, D, dtype, seed):
    rng = np.random.default_rng(seed)
    hs = [(rng.random((r, D), dtype=np.float32) - 0.5).astype(dtype, copy=False) for r in rows]
    return hs, [torch.from_numpy(h).to(DEV) for h in hs]


def _indices(rows, B, P, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(1, r + 1, (B, P)) for r in rows]


def _block():
    return torch.zeros(_lib.ET_LOOKUP_QUEUE_BYTES // 4, dtype=torch.int32, device=DEV)


def _block_is_zero(q):
    return q.cpu().numpy().tobytes() == bytes(_lib.ET_LOOKUP_QUEUE_BYTES)


class Launch:
    """One et_maplookup_prealloc_q call over device tables `tabs` and host indices `hidx`."""

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

    def __call__(self, q):
        dst = torch.full((self.B, self.D * self.n), float("nan"), dtype=self.tabs[0].dtype,
                         device=DEV)
        _lib.check(_lib.load().et_maplookup_prealloc_q(
            self.code, ctypes.addressof(self.descs), self.n, self.B, dst.data_ptr(),
            self.D * self.n, 0, q.data_ptr(), _lib.stream_handle()))
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
def phases():
    return _tables(ROWS, 128, np.float32, 90)


@pytest.mark.parametrize("B", [1, 65, 257, 4099])
@pytest.mark.parametrize("P", [13, 20])
def test_every_phase(oracle, phases, P, B):
    """One non-temporal and three allocating fabric tables, four cache tables."""
    hs, tabs = phases
    _check(oracle, hs, tabs, _indices(ROWS, B, P, 1000 * P + B))


@pytest.mark.parametrize("rows", [[4099, 3000, 50, 3], [524300, 20000, 9000, 8200]],
                         ids=["cache", "fabric"])
def test_one_class_empty(oracle, phases, rows):
    """Only one class: the one-queue schedule runs, in the static order."""
    hs, tabs = phases
    sel = [ROWS.index(r) for r in rows]
    _check(oracle, [hs[k] for k in sel], [tabs[k] for k in sel], _indices(rows, 257, 13, 91))


def test_max_tables_per_launch(oracle, phases):
    """32 tables: 6 fabric (one of them non-temporal) and 26 cache."""
    rows = [8200 + 100 * k for k in range(5)] + [1 + 157 * k for k in range(26)]
    hs, tabs = _tables(rows, 128, np.float32, 92)
    rows, hs, tabs = ROWS[:1] + rows, phases[0][:1] + hs, phases[1][:1] + tabs
    assert len(rows) == _lib.ET_MAX_TABLES_PER_LAUNCH and max(rows[6:]) <= 8192 < min(rows[:6])
    _check(oracle, hs, tabs, _indices(rows, 300, 13, 93))


def test_fp16_x_256(oracle):
    """The other scalar-addressed type: 512-byte fp16 rows, same classes as ROWS."""
    hs, tabs = _tables(ROWS, 256, np.float16, 94)
    _check(oracle, hs, tabs, _indices(ROWS, 257, 13, 95))


def test_back_to_back_on_one_block(oracle, phases):
    """20 launches on one stream and one block without a synchronise between them."""
    hs, tabs = phases
    hidx = _indices(ROWS, 257, 13, 96)
    ref = oracle.maplookup_prealloc(hs, hidx)
    run, q = Launch(tabs, hidx), _block()
    et.check_errors()
    outs = [run(q) for _ in range(20)]
    torch.cuda.synchronize()
    assert _block_is_zero(q)
    assert et.check_errors() == 0
    assert all(_same(o, ref) for o in outs)
