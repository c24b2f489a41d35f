"""Column quarters of the pooled lookup (csrc/et_lookup_order.h, DESIGN §4 "Column quarters"): a
contiguous table of 512-byte rows above 4 MiB and up to 16 MiB is cut by columns, XCD x summing the
128-byte line x % 4 of every row for the bags of batch half x / 4.  A pooled sum is independent per
column, so every case is compared bit for bit with the oracle.  The destination is pre-filled with
NaN (an unclaimed item or quarter shows), the caller's queue block must be zero after every launch
and check_errors() == 0 unless the case plants bad indices.

Shapes: fp32 x 128, 8,192 rows is exactly 4 MiB (whole rows, a cache table), 8,193, 20,000 and
32,768 rows (exactly 16 MiB) are quartered, 32,769 rows is not; 524,300 rows is above 256 MiB
(non-temporal), 3,000 and 3 rows are cache tables.  The quarter loop takes 32 bags per round and
reads a bag's indices in chunks of 8: B in {1, 31, 33, 257, 4099} and P in {1, 7, 8, 9, 20} sit on
both sides of each (B = 4099 gives stripe_chunks = 65 and rounds = 1; both batch halves hold
bags only from B = 2081 on, so the smaller batches leave the second half's items empty)."""
import ctypes

import numpy as np
import pytest
import torch

import embtab as et
from embtab import _lib

import footprint as fp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

ROWS = [8192, 8193, 20000, 32768, 32769, 524300, 3000, 3]
QUARTERED = [8193, 20000, 32768]


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
    """One et_maplookup_prealloc_q call over device tables `tabs` (2-D, possibly strided views) and
    host indices `hidx`; q = None is the entry without a queue block (the static stripe kernel)."""

    def __init__(self, tabs, hidx, prepend=0, flags=0, code=None):
        self.tabs = tabs
        self.idx = [torch.from_numpy(np.ascontiguousarray(i)).to(DEV) for i in hidx]
        self.n, self.D = len(tabs), tabs[0].shape[1]
        self.B = hidx[0].shape[0]
        self.prepend, self.flags = prepend, flags
        self.descs = (_lib.LookupDesc * self.n)()
        for t, (A, I) in enumerate(zip(tabs, self.idx)):
            self.descs[t] = _lib.LookupDesc(A.data_ptr(), A.stride(0), A.shape[0], self.D,
                                            I.shape[1], I.data_ptr(), I.shape[1],
                                            prepend + t * self.D, 0)
        self.code = _lib.TORCH_TO_ET[tabs[0].dtype] if code is None else code
        self.width = prepend + self.D * self.n

    def into(self, ptr, ld, q):
        _lib.check(_lib.load().et_maplookup_prealloc_q(
            self.code, ctypes.addressof(self.descs), self.n, self.B, ptr, ld, self.flags,
            q.data_ptr() if q is not None else None, _lib.stream_handle()))

    def __call__(self, q):
        dst = torch.full((self.B, self.width), float("nan"), dtype=self.tabs[0].dtype, device=DEV)
        self.into(dst.data_ptr(), self.width, q)
        return dst


def _same(got, ref):
    return got.cpu().numpy().tobytes() == np.ascontiguousarray(ref).tobytes()


def _check(oracle, hs, tabs, hidx, queue=True, **ref_args):
    q = _block() if queue else None
    et.check_errors()
    got = Launch(tabs, hidx)(q)
    torch.cuda.synchronize()
    assert q is None or _block_is_zero(q)
    assert et.check_errors() == 0
    assert _same(got, oracle.maplookup_prealloc(hs, hidx, **ref_args))


@pytest.fixture(scope="module")
def mix():
    return _tables(ROWS, 128, np.float32, 110)


def _pick(mix, rows):
    sel = [ROWS.index(r) for r in rows]
    return [mix[0][k] for k in sel], [mix[1][k] for k in sel]


@pytest.mark.parametrize("B", [1, 31, 33, 257, 4099])
@pytest.mark.parametrize("P", [1, 7, 8, 9, 20])
def test_both_sides_of_every_threshold(oracle, mix, P, B):
    hs, tabs = mix
    _check(oracle, hs, tabs, _indices(ROWS, B, P, 1000 * P + B))


@pytest.mark.parametrize("B", [1, 31, 33, 257, 4099])
@pytest.mark.parametrize("P", [1, 7, 8, 9, 20])
def test_static_stripe_kernel(oracle, mix, P, B):
    """No queue block: k_pooled_vec_striped runs the same entries."""
    hs, tabs = mix
    _check(oracle, hs, tabs, _indices(ROWS, B, P, 2000 * P + B), queue=False)


@pytest.mark.parametrize("queue", [True, False], ids=["queued", "static"])
def test_only_quartered_tables(oracle, mix, queue):
    """One class is empty whichever class the quartered entries join: the one-queue schedule."""
    hs, tabs = _pick(mix, QUARTERED)
    _check(oracle, hs, tabs, _indices(QUARTERED, 4099, 9, 111), queue=queue)


def test_destination_block_starts_mid_row(oracle, mix):
    """PreallocationStrategy(16): 16 prepended fp32 columns, so every table's block (and every
    quarter's 128 bytes) starts 64 bytes into a 128-byte line of the destination."""
    hs, tabs = mix
    hidx = _indices(ROWS, 257, 9, 112)
    q = _block()
    et.check_errors()
    got = Launch(tabs, hidx, prepend=16)(q)
    assert _block_is_zero(q) and et.check_errors() == 0
    ref = oracle.maplookup_prealloc(hs, hidx, prependrows=16)
    assert _same(got[:, 16:], ref[:, 16:])
    assert bool(torch.isnan(got[:, :16]).all())  # the prepended columns are not touched


def test_strided_table_view(oracle, mix):
    """ld_table > dim: a 20,000-row view of a wider matrix is not quartered (not contiguous) and
    runs whole rows beside the quartered tables."""
    rows = [20000, 8193, 20000, 3000]
    hs, tabs = _pick(mix, rows)
    wide = torch.full((20000, 160), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, 16:144] = tabs[0]
    tabs = [wide[:, 16:144]] + tabs[1:]
    assert tabs[0].stride(0) == 160 and tabs[0].data_ptr() % 16 == 0
    _check(oracle, hs, tabs, _indices(rows, 257, 9, 113))


def test_out_of_range_indices_in_quartered_tables(oracle, mix):
    """One index past the end and one index 0 in quartered tables: each adds a zero row in all
    four quarters and is counted once, not once per quarter."""
    hs, tabs = mix
    B, P = 257, 9
    hidx = _indices(ROWS, B, P, 114)
    bad = [i.copy() for i in hidx]
    edits = [(ROWS.index(20000), B - 1, 8, 20001), (ROWS.index(8193), 40, 0, 0)]
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


TYPE_ROWS = [8193, 32768, 3000, 32769]


@pytest.mark.parametrize("kind", ["f16", "f16_fp32_acc", "bf16", "f64"])
def test_other_512_byte_row_types(oracle, kind):
    """fp16 x 256 with and without fp32 accumulation, bf16 x 256 and f64 x 64."""
    rng = np.random.default_rng(115)
    D = 64 if kind == "f64" else 256
    raw = [rng.random((r, D), dtype=np.float32) - 0.5 for r in TYPE_ROWS]
    ref_args, flags = {}, 0
    if kind == "bf16":
        hs = [oracle.f32_to_bf16(x) for x in raw]
        tabs = [torch.from_numpy(h.view(np.int16)).to(DEV).view(torch.bfloat16) for h in hs]
        ref_args = {"bf16": True}
    else:
        hs = [x.astype(np.float64 if kind == "f64" else np.float16) for x in raw]
        tabs = [torch.from_numpy(h).to(DEV) for h in hs]
    if kind == "f16_fp32_acc":
        flags, ref_args = _lib.ET_FLAG_F16_FP32_ACC, {"f16_fp32_acc": True}
    hidx = _indices(TYPE_ROWS, 257, 9, 116)
    for q in (_block(), None):
        et.check_errors()
        run = Launch(tabs, hidx, flags=flags)
        if kind == "bf16":
            dst = torch.full((257, run.width), -1, dtype=torch.int16, device=DEV)
            run.into(dst.data_ptr(), run.width, q)
            got = dst
        else:
            got = run(q)
        torch.cuda.synchronize()
        assert q is None or _block_is_zero(q)
        assert et.check_errors() == 0
        assert _same(got, oracle.maplookup_prealloc(hs, hidx, **ref_args))


def test_max_tables_six_quartered(oracle, mix):
    """32 tables in a launch: six quartered, one whole-row fabric table, 25 cache tables."""
    qrows = [8193 + 3000 * k for k in range(6)]
    rows = qrows + [32769] + [1 + 157 * k for k in range(25)]
    assert len(rows) == _lib.ET_MAX_TABLES_PER_LAUNCH and max(qrows) <= 32768
    hs, tabs = _tables(rows, 128, np.float32, 117)
    _check(oracle, hs, tabs, _indices(rows, 300, 9, 118))


def test_back_to_back_on_one_block(oracle, mix):
    """Two launches on one stream and one queue block without a synchronise between them."""
    hs, tabs = mix
    hidx = _indices(ROWS, 4099, 7, 119)
    ref = oracle.maplookup_prealloc(hs, hidx)
    run, q = Launch(tabs, hidx), _block()
    et.check_errors()
    outs = [run(q) for _ in range(2)]
    torch.cuda.synchronize()
    assert _block_is_zero(q)
    assert et.check_errors() == 0
    assert all(_same(o, ref) for o in outs)


@pytest.mark.parametrize("queue", [True, False], ids=["queued", "static"])
def test_quarter_stores_tile_the_block(oracle, mix, queue):
    """A canary-guarded destination: the four quarters' 128-byte stores fill each table's block
    and change nothing around the destination or in the padding of its rows."""
    rows = [8193, 32768, 3000]
    hs, tabs = _pick(mix, rows)
    B = 257
    hidx = _indices(rows, B, 9, 120)
    run = Launch(tabs, hidx)
    buf, view, intact = fp.guarded_matrix(B, run.width, torch.float32, DEV, left=4,
                                          ld=run.width + 8)
    assert view.data_ptr() % 16 == 0
    q = _block() if queue else None
    et.check_errors()
    run.into(view.data_ptr(), buf.stride(0), q)
    torch.cuda.synchronize()
    assert et.check_errors() == 0
    ok, where = intact()
    assert ok, f"guard byte changed at (buffer row, byte column) {where}"
    assert _same(view.contiguous(), oracle.maplookup_prealloc(hs, hidx))
