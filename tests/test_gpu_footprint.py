"""Where the kernels read and write: workspace size and alignment, independence from stale
workspace bytes, and the footprints of destinations, tables, states and index outputs.

Every entry that takes a caller-owned workspace (et_sparse_sgd / _snap and its two phases,
et_index_build, et_ragged_sgd, et_weighted_sgd, et_sparse_adagrad) is called through the C ABI
with EXACTLY the bytes its ``*_workspace_size`` asks for, cut out of a canary-filled allocation
(tests/footprint.py) at a 0, 4 or 100 byte offset from a 256-byte boundary and pre-filled with
an adversarial pattern.  The tables, optimiser states, snapshots and index outputs of these
calls live in canary-guarded memory too (rows wider than ``dim``, guard rows above and below),
so each case checks the result against the family's own reference, every guard, and that the
read-only operands keep their bytes.

No tolerance is introduced here: results are compared byte for byte with the reference where
the mode is exact and between poison patterns otherwise; where a family's own test compares
within a bound (split-mode long columns and the hot pass: tests/test_gpu_update.py; row-wise
AdaGrad: tests/test_gpu_adagrad.py; the weight gradient: tests/test_gpu_weighted.py) that
test's helper and bound are used unchanged.

Nothing here passes more workspace bytes than it owns or fewer than the ABI asks for."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import embtab as et
import footprint as fp
import quant_ref as qr
import weighted_ref as wr
from embtab import _lib
from embtab import update as upd
from test_gpu_adagrad import (KINDS, lists_fixed, lists_ragged, make_indices, ragged_case,
                              ref_step, rowwise_bounds)
from test_gpu_ragged import colptr_of, expect_lookup, hot_case, mix_lengths, ranges_of
from test_gpu_update import _fp64_update_and_scale

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHUNK = _lib.ET_SGD_CHUNK
NT = _lib.ET_FLAG_NONTEMPORAL
EXACT = _lib.ET_FLAG_EXACT_UPDATE
ETA = 0.1
SHIFTS = [0, 4, 100]
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16,
         "f64": torch.float64}


def orc():
    import oracle

    oracle.lib()
    return oracle


def dev(x, kind="f32"):
    x = np.ascontiguousarray(x)
    if kind == "bf16":
        return torch.from_numpy(x.view(np.int16)).to(DEV).view(torch.bfloat16)
    return torch.from_numpy(x).to(DEV)


def host(t):
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def typed(x, kind):
    return wr.typed(x, kind)[0]


def zipf_idx(rng, R, shape, a=1.2):
    z = np.minimum(rng.zipf(a, shape), R)
    return (rng.permutation(R) + 1)[z - 1].astype(np.int64)


def uniform_idx(rng, R, shape):
    return rng.integers(1, R + 1, shape).astype(np.int64)


class Guarded:
    """A (rows, cols) matrix in canary-guarded device memory holding `base`.  layout "vec":
    a 16-byte aligned view in rows a multiple of 16 bytes wide (the kernels' vector loads and
    stores apply) with at least 4 pad elements behind every row; "pad7": 7 elements on each
    side (element-aligned, the generic kernels)."""

    def __init__(self, base, kind="f32", layout="vec", guard_rows=2):
        self.base, self.kind = np.ascontiguousarray(base), kind
        R, D = base.shape
        kw = dict(ld=-(-(D + 12) // 8) * 8, left=8) if layout == "vec" else {}
        self.buf, self.view, self.intact = fp.guarded_matrix(R, D, TORCH[kind], DEV,
                                                             guard_rows=guard_rows, **kw)
        self.ld = self.view.stride(0)
        assert self.ld > D
        if layout == "vec":
            assert self.view.data_ptr() % 16 == 0 and self.ld * self.view.element_size() % 16 == 0
        self.restore()

    def restore(self):
        self.buf.view(torch.uint8).fill_(fp.CANARY)
        self.view.copy_(dev(self.base, self.kind))

    @property
    def ptr(self):
        return self.view.data_ptr()

    def host(self):
        return host(self.view)

    def check(self, what):
        ok, where = self.intact()
        assert ok, f"{what}: guard byte changed at buffer (row, byte) {where}"


class GuardedVec:
    """`count` elements of `dtype` between canaries (exactly count * itemsize bytes owned)."""

    def __init__(self, count, dtype=torch.int64):
        self.count, self.dtype = count, dtype
        es = torch.empty(0, dtype=dtype).element_size()
        self.buf, self.raw = fp.guarded_bytes(count * es, 0, DEV)

    def restore(self):
        self.buf.fill_(fp.CANARY)

    @property
    def ptr(self):
        return self.raw.data_ptr()

    def host(self):
        return self.raw.cpu().numpy().view({torch.int64: np.int64, torch.float32: np.float32,
                                            torch.float64: np.float64}[self.dtype])

    def check(self, what):
        fp.assert_guards(self.buf, self.raw, what)


def check_sgd_table(got, base, delta, I, exact, what):
    """One Float32 table against the oracle as tests/test_gpu_update.py compares it: bit for
    bit in the exact mode and for every column of at most ET_SGD_CHUNK occurrences, longer
    columns of the split mode / hot pass within 1e-6 of |w| + eta * sum|delta| of the fp64
    update.  Returns the occurrence counts per column."""
    R = base.shape[0]
    I2 = I.reshape(I.shape[0], -1)
    ref = base.copy()
    orc().sgd(ref, delta, I, ETA, fused=True)
    counts = np.bincount(I2.ravel(), minlength=R + 1)[1:]
    short = np.ones(R, bool) if exact else counts <= CHUNK
    assert same(got[short], ref[short]), what
    if not short.all():
        upd64, scale = _fp64_update_and_scale(base, delta, I2, ETA)
        assert np.all(np.abs(got.astype(np.float64) - upd64) <= 1e-6 * scale), what
    assert not same(got, base), f"{what}: nothing was updated"
    return counts


# --- the cases: one ABI call each ---------------------------------------------------------------

class Case:
    oob = 0

    def size(self):
        nb = ctypes.c_int64(0)
        _lib.check(self.size_fn()(ctypes.addressof(self.descs), len(self.descs), ctypes.byref(nb)))
        return nb.value

    def restore(self):
        for g in self.guarded:
            g.restore()

    def check_guards(self, what):
        for i, g in enumerate(self.guarded):
            g.check(f"{what}: guarded operand {i}")

    def results(self):
        return [g.host().tobytes() for g in self.guarded]


class SgdCase(Case):
    """et_sparse_sgd / et_sparse_sgd_snap (or INDEX_ONLY then APPLY_ONLY) over Float32 tables
    `specs` = [(rows, dim, pool)], every table and snapshot in guarded memory."""

    def __init__(self, specs, B, flags, idx=zipf_idx, snap=False, phased=False, seed=1,
                 layout="vec", indices=None, need_long=CHUNK):
        rng = np.random.default_rng(seed)
        self.specs, self.B, self.flags, self.idx_fn = specs, B, flags, idx
        self.snap, self.phased, self.seed, self.layout = snap, phased, seed, layout
        self.exact = bool(flags & EXACT)
        self.need_long = need_long
        self.bases = [rng.standard_normal((R, D)).astype(np.float32) for R, D, P in specs]
        self.I = indices or [idx(rng, R, (B, P)) for R, D, P in specs]
        self.deltas = [rng.standard_normal((B, D)).astype(np.float32) for R, D, P in specs]
        self.tabs = [Guarded(b, layout=layout) for b in self.bases]
        self.dI = [dev(i) for i in self.I]
        self.dd = [dev(d) for d in self.deltas]
        self.snaps = [GuardedVec(B * P) for R, D, P in specs] if snap else []
        self.guarded = self.tabs + self.snaps
        self.readonly = self.dI + self.dd
        self.descs = (_lib.UpdateDesc * len(specs))(*[
            _lib.UpdateDesc(t.ptr, t.ld, R, D, P, d.data_ptr(), D, i.data_ptr(), P, B, 0)
            for (R, D, P), t, d, i in zip(specs, self.tabs, self.dd, self.dI)])
        self.sarr = (ctypes.c_void_p * len(specs))(*[s.ptr for s in self.snaps]) if snap else None

    def size_fn(self):
        return _lib.load().et_sgd_workspace_size

    def call(self, ptr, nbytes):
        L = _lib.load()
        a, n, st = ctypes.addressof(self.descs), len(self.descs), _lib.stream_handle()
        phases = ([_lib.ET_FLAG_SGD_INDEX_ONLY, _lib.ET_FLAG_SGD_APPLY_ONLY] if self.phased
                  else [0])
        for k, ph in enumerate(phases):
            if self.snap and k == 0:
                _lib.check(L.et_sparse_sgd_snap(_lib.ET_F32, a, n, ETA, self.flags | ph,
                                                ctypes.addressof(self.sarr), ptr, nbytes, st))
            else:
                _lib.check(L.et_sparse_sgd(_lib.ET_F32, a, n, ETA, self.flags | ph, ptr, nbytes,
                                           st))

    def check(self, what):
        longest = 0
        for t, (tab, base, d, I) in enumerate(zip(self.tabs, self.bases, self.deltas, self.I)):
            counts = check_sgd_table(tab.host(), base, d, I, self.exact, f"{what}: table {t}")
            longest = max(longest, int(counts.max()))
        # a chain (exact) or a multi-chunk column (split, hot pass); 32768: an early hot column
        assert longest > self.need_long, what
        for s, I in zip(self.snaps, self.I):
            assert same(s.host(), I.reshape(-1)), f"{what}: snapshot"

    def leftover(self):
        """The same entry on a larger problem with uniform instead of skewed indices."""
        return SgdCase(self.specs, self.B + self.B // 4 + 77, self.flags, uniform_idx, self.snap,
                       self.phased, self.seed + 1000, self.layout, need_long=0)


def eh_indices(rng, R, shape):
    """Column 7 in 17 of every bag's 20 slots: 34816 of 40960 occurrences, above the 32768 the
    early hot-column list asks of a candidate, so that list (carved last without a hot-shaped
    table) is live in the exact mode."""
    I = uniform_idx(rng, R, shape)
    I[:, :17] = 7
    return I


SGD_CASES = {
    # exact: one table of more than 128 rows with an early hot column; a chain of 34816
    "exact": lambda: SgdCase([(300, 64, 20)], 2048, NT | EXACT, eh_indices, need_long=32768),
    "split": lambda: SgdCase([(700, 64, 20)], 1000, NT),
    # an early-chain table (<= 128 rows) beside a regular one, through the snapshot entry
    "exact multi snap": lambda: SgdCase([(100, 16, 3), (3000, 64, 20)], 500, NT | EXACT,
                                        snap=True),
    "split multi snap": lambda: SgdCase([(100, 16, 3), (3000, 64, 20)], 500, NT, snap=True),
    # hot pass: dim 128, pool <= 32, a batch that is no multiple of the 1024-bag window
    "hot pass": lambda: SgdCase([(400, 128, 20)], 1500, NT | _lib.ET_FLAG_SGD_HOT_PASS,
                                functools.partial(zipf_idx, a=1.1)),
    "two-phase exact": lambda: SgdCase([(700, 64, 20), (90, 32, 5)], 600, NT | EXACT,
                                       phased=True),
    "two-phase split": lambda: SgdCase([(700, 64, 20), (90, 32, 5)], 600, NT, phased=True),
}


class IndexCase(Case):
    """et_index_build with outputs of exactly n + 1, n + 1, n and 1 Int64 entries."""
    exact = True

    def __init__(self, I, nrows):
        self.I, self.nrows = I, nrows
        B = I.shape[0]
        P = 1 if I.ndim == 1 else I.shape[1]
        self.B, self.P, self.n = B, P, B * P
        self.dI = dev(I)
        self.cc, self.co = GuardedVec(self.n + 1), GuardedVec(self.n + 1)
        self.map, self.nu = GuardedVec(self.n), GuardedVec(1)
        self.guarded = [self.cc, self.co, self.map, self.nu]
        self.readonly = [self.dI]

    def size(self):
        nb = ctypes.c_int64(0)
        _lib.check(_lib.load().et_index_workspace_size(self.n, ctypes.byref(nb)))
        return nb.value

    def call(self, ptr, nbytes):
        _lib.check(_lib.load().et_index_build(self.dI.data_ptr(), self.P, self.P, self.B,
                                              self.nrows, self.cc.ptr, self.co.ptr, self.map.ptr,
                                              self.nu.ptr, ptr, nbytes, _lib.stream_handle()))

    def results(self):
        # include/embtab.h defines entries [0, U] of the cumulative arrays and says nothing of
        # the entries past the terminator, so only the defined entries are compared.  Observed
        # (printed by check): entries U + 1 .. n are left as they were, the fill survives.
        # That is not asserted: they are inside the owned n + 1 entries either way.
        U = int(self.nu.host()[0])
        assert 0 < U <= self.n
        return [self.cc.host()[:U + 1].tobytes(), self.co.host()[:U + 1].tobytes(),
                self.map.host().tobytes(), U]

    def check(self, what):
        cum, mp = orc().index_build(self.I, self.nrows)
        cc, co, m, U = self.results()
        assert U == cum.shape[0] - 1 and cc == cum[:, 0].tobytes() and co == cum[:, 1].tobytes(), what
        assert m == mp.tobytes(), what
        assert U > 1 and self.n > U, f"{what}: no repeated column"
        tail = np.concatenate([self.cc.host()[U + 1:], self.co.host()[U + 1:]])
        print(f"{what}: entries past the terminator "
              f"{'untouched' if same(tail, np.full(len(tail), 0xA5A5A5A5A5A5A5A5, np.uint64).view(np.int64)) else 'written'}")

    def leftover(self):
        rng = np.random.default_rng(self.n)
        return IndexCase(uniform_idx(rng, 5000, (self.n + self.n // 3 + 11,)), 5000)


class RaggedCase(Case):
    """et_ragged_sgd or et_weighted_sgd over one or two tables; `tables` = [(rows, dim, L,
    values)] with a capacity tail of `tail` entries no bag covers."""
    exact = True

    def __init__(self, tables, weighted, kind="f32", seed=3, tail=50, layout="vec"):
        rng = np.random.default_rng(seed)
        self.weighted, self.kind, self.seed, self.layout = weighted, kind, seed, layout
        self.bf16 = kind == "bf16"
        self.t = []
        descs = []
        cls = _lib.WeightedUpdateDesc if weighted else _lib.RaggedUpdateDesc
        self.guarded, self.readonly = [], []
        for R, D, L, values in tables:
            used = int(L.sum())
            assert len(values) == used
            cap = used + (tail if used else 0)
            vals = np.concatenate([values, uniform_idx(rng, R, (cap - used,))]).astype(np.int64)
            cp = colptr_of(L)
            B = len(L)
            base = typed(rng.standard_normal((R, D)), kind)
            delta = typed(0.25 * rng.standard_normal((B, D)), kind)
            w = rng.standard_normal(cap).astype(np.float32)
            w[used:] = np.nan  # never read
            tab = Guarded(base, kind, layout)
            dv, dc, dd, dw = dev(vals), dev(cp), dev(delta, kind), dev(w)
            args = [tab.ptr, tab.ld, R, D, 0, dd.data_ptr(), D, dv.data_ptr() if cap else None,
                    cap, dc.data_ptr(), B, 0]
            descs.append(cls(*(args + [dw.data_ptr(), None] if weighted else args)))
            self.t.append(dict(R=R, D=D, L=L, vals=vals, cp=cp, used=used, cap=cap, base=base,
                               delta=delta, w=w, tab=tab))
            self.guarded.append(tab)
            self.readonly += [dv, dc, dd] + ([dw] if weighted else [])
        self.descs = (cls * len(descs))(*descs)

    def size_fn(self):
        L = _lib.load()
        return L.et_weighted_sgd_workspace_size if self.weighted else L.et_ragged_sgd_workspace_size

    def call(self, ptr, nbytes):
        L = _lib.load()
        f = L.et_weighted_sgd if self.weighted else L.et_ragged_sgd
        _lib.check(f(_lib.TORCH_TO_ET[TORCH[self.kind]], ctypes.addressof(self.descs),
                     len(self.descs), ETA, NT, ptr, nbytes, _lib.stream_handle()))

    def reference(self, t):
        base, delta, vals, cp, used = t["base"], t["delta"], t["vals"], t["cp"], t["used"]
        if not used:
            return base
        if not self.weighted:
            ref = base.copy()
            orc().sgd(ref, delta[np.repeat(np.arange(len(t["L"])), t["L"])], vals[:used], ETA,
                      fused=True, bf16=self.bf16)
            return ref
        if self.kind == "f32":
            E, cov = wr.expanded_gradient(delta, t["w"], cp, t["cap"])
            ref = base.copy()
            orc().sgd(ref, E[cov], vals[cov], ETA, fused=True)
            return ref
        return wr.sgd(base.copy(), delta, vals, cp, t["w"], ETA, fused=True, bf16=self.bf16,
                      nnz=t["cap"])

    def check(self, what):
        for k, t in enumerate(self.t):
            if "ref" not in t:
                t["ref"] = self.reference(t)
            assert same(t["tab"].host(), t["ref"]), f"{what}: table {k}"
        assert any(not same(t["ref"], t["base"]) for t in self.t), f"{what}: nothing was updated"

    def leftover(self):
        rng = np.random.default_rng(self.seed + 500)
        tabs = []
        for t in self.t:
            L = rng.integers(0, 9, len(t["L"]) * 2 + 100).astype(np.int64)
            tabs.append((t["R"], t["D"], L, uniform_idx(rng, t["R"], (int(L.sum()),))))
        return RaggedCase(tabs, self.weighted, self.kind, self.seed + 500, 300, self.layout)


def hot_ragged(weighted, kind, dim, layout="vec"):
    """The ragged family's hot case: the length mix, ten bags of 300 entries of one column
    (a serial list of 3000 entries, well past ET_SGD_CHUNK)."""
    rng = np.random.default_rng(7)
    L, values, rows40 = hot_case(257, rng)
    assert (values == rows40[0]).sum() >= 3000 > CHUNK
    return RaggedCase([(700, dim, L, values)], weighted, kind, layout=layout)


class AdaCase(Case):
    """et_sparse_adagrad over a fixed-pool table (dim 128, the test_gpu_adagrad.py indices: a
    column of 2307 occurrences, ten chunks of partials) and a ragged one (dim 20, a list
    longer than a chunk with uncovered entries) in one call; tables and states guarded."""

    def __init__(self, rowwise, seed=41, layout="vec", dims=(128, 20), big=False):
        rng = np.random.default_rng(seed)
        self.rowwise, self.seed, self.layout, self.dims = rowwise, seed, layout, dims
        self.exact = not rowwise
        self.kind = KINDS["f32"]
        R = 300
        I = make_indices(rng)
        if big:  # the leftover problem: more and differently placed occurrences
            I = np.concatenate([I, uniform_idx(rng, R, (700, I.shape[1]))])
        Lr, values, colptr = ragged_case(rng, head=90 if big else 40, tail=900 if big else 600)
        self.lists = [lists_fixed(I), lists_ragged(values, colptr)]
        assert max(len(v) for v in self.lists[0].values()) > 4 * CHUNK
        assert len(self.lists[1][13]) > CHUNK
        self.bases = [rng.standard_normal((R, d)).astype(np.float32) for d in dims]
        self.states0 = [(rng.random(R) if rowwise else rng.random((R, d))).astype(np.float32)
                        for d in dims]
        self.deltas = [rng.standard_normal((I.shape[0], dims[0])).astype(np.float32),
                       rng.standard_normal((len(Lr), dims[1])).astype(np.float32)]
        self.tabs = [Guarded(b, layout=layout) for b in self.bases]
        if rowwise:
            self.states = [GuardedVec(R, torch.float32) for _ in dims]
        else:
            self.states = [Guarded(s, layout=layout) for s in self.states0]
        self.guarded = self.tabs + self.states
        dI, dv, dc = dev(I), dev(values), dev(colptr)
        dd = [dev(d) for d in self.deltas]
        self.readonly = [dI, dv, dc] + dd
        A = _lib.AdaGradDesc
        lds = [1, 1] if rowwise else [s.ld for s in self.states]
        self.descs = (A * 2)(
            A(self.tabs[0].ptr, self.tabs[0].ld, R, dims[0], I.shape[1], dd[0].data_ptr(), dims[0],
              dI.data_ptr(), I.shape[1], I.shape[0], 0, None, 0, self.states[0].ptr, lds[0]),
            A(self.tabs[1].ptr, self.tabs[1].ld, R, dims[1], 1, dd[1].data_ptr(), dims[1],
              dv.data_ptr(), 1, len(Lr), 0, dc.data_ptr(), len(values), self.states[1].ptr, lds[1]))

    def size_fn(self):
        return _lib.load().et_adagrad_workspace_size

    def restore(self):
        super().restore()
        if self.rowwise:
            for s, s0 in zip(self.states, self.states0):
                s.raw.copy_(dev(s0).view(torch.uint8))

    def call(self, ptr, nbytes):
        flags = NT | (_lib.ET_FLAG_ADAGRAD_ROWWISE if self.rowwise else 0)
        _lib.check(_lib.load().et_sparse_adagrad(_lib.ET_F32, ctypes.addressof(self.descs), 2,
                                                 ETA, 1e-8, flags, ptr, nbytes,
                                                 _lib.stream_handle()))

    def check(self, what):
        for k in range(2):
            got_t, got_s = self.tabs[k].host(), self.states[k].host()
            if self.rowwise:  # the family's bound (tests/test_gpu_adagrad.py rowwise_bounds)
                rs, rw = rowwise_bounds(self.kind, self.bases[k], self.states0[k], self.deltas[k],
                                        self.lists[k], got_t, got_s, ETA, 1e-8)
                assert rs <= 1.0 and rw <= 1.0, (what, k, rs, rw)
            else:
                if not hasattr(self, "refs"):
                    self.refs = {}
                if k not in self.refs:
                    t, s = self.bases[k].copy(), self.states0[k].copy()
                    ref_step(self.kind, t, s, self.deltas[k], self.lists[k], ETA, 1e-8)
                    self.refs[k] = (t, s)
                assert same(got_t, self.refs[k][0]) and same(got_s, self.refs[k][1]), (what, k)
            assert not same(got_t, self.bases[k]) and not same(got_s, self.states0[k]), what

    def leftover(self):
        return AdaCase(self.rowwise, self.seed + 7, self.layout, self.dims, big=True)


class AdaVecCase(Case):
    """et_sparse_adagrad, element-wise, one Float32 table under the vector index `I`."""
    exact = True

    def __init__(self, I, R, dim=16, seed=0):
        rng = np.random.default_rng(seed)
        self.I, self.R = I, R
        self.base = rng.standard_normal((R, dim)).astype(np.float32)
        self.state0 = rng.random((R, dim)).astype(np.float32)
        self.delta = rng.standard_normal((len(I), dim)).astype(np.float32)
        self.tab, self.st = Guarded(self.base), Guarded(self.state0)
        self.guarded = [self.tab, self.st]
        dI, dd = dev(I), dev(self.delta)
        self.readonly = [dI, dd]
        A = _lib.AdaGradDesc
        self.descs = (A * 1)(A(self.tab.ptr, self.tab.ld, R, dim, 1, dd.data_ptr(), dim,
                               dI.data_ptr(), 1, len(I), 0, None, 0, self.st.ptr, self.st.ld))

    def size_fn(self):
        return _lib.load().et_adagrad_workspace_size

    def call(self, ptr, nbytes):
        _lib.check(_lib.load().et_sparse_adagrad(_lib.ET_F32, ctypes.addressof(self.descs), 1,
                                                 ETA, 1e-8, NT, ptr, nbytes,
                                                 _lib.stream_handle()))

    def check(self, what):
        t2, s2 = self.base.copy(), self.state0.copy()
        ref_step(KINDS["f32"], t2, s2, self.delta, lists_fixed(self.I, self.R), ETA, 1e-8)
        assert same(self.tab.host(), t2) and same(self.st.host(), s2), what
        assert not same(t2, self.base), f"{what}: nothing was updated"


def index_case():
    rng = np.random.default_rng(5)
    return IndexCase(zipf_idx(rng, 900, (1500, 7)), 900)


CASES = dict(SGD_CASES)
CASES.update({
    "index": index_case,
    "ragged f32": lambda: hot_ragged(False, "f32", 20),
    "ragged bf16": lambda: hot_ragged(False, "bf16", 64),
    "weighted f32": lambda: hot_ragged(True, "f32", 20),
    "weighted bf16": lambda: hot_ragged(True, "bf16", 64),
    "adagrad": lambda: AdaCase(False),
    "adagrad rowwise": lambda: AdaCase(True),
})


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


FILLS = {"zero": 0x00, "ones": 0xFF, "canary": fp.CANARY}


def run(c, shift, poison, what):
    """One call of `c` on an exact-size workspace at `shift`, pre-filled with `poison`; checks
    the workspace guards (the 0..255 slack bytes in front included), the guarded operands, the
    read-only operands and the out-of-range count; returns the results."""
    nb = c.size()
    other = c.leftover() if poison == "leftover" else None
    cap = max(nb, other.size()) if other else nb
    buf, whole = fp.guarded_bytes(cap, shift, DEV)

    def leave(v):
        other.restore()
        other.call(v.data_ptr(), other.size())
        torch.cuda.synchronize()

    fp.POISONS[poison](whole, leave)
    c.restore()
    snaps = [fp.snapshot(t) for t in c.readonly]
    ws = whole[:nb]
    c.call(ws.data_ptr(), nb)
    torch.cuda.synchronize()
    assert et.check_errors() == c.oob, what
    fp.assert_guards(buf, whole, f"{what}: workspace of {nb} bytes at shift {shift}")
    if poison in FILLS:
        # the layout starts at the first 256-byte boundary and needs nb - 256 + skip bytes: the
        # bytes it skips in front and the rest of the slack behind it keep the fill
        skip = (256 - shift) % 256
        used = nb - 256 + skip
        assert bool((whole[:skip] == FILLS[poison]).all()), f"{what}: wrote in front of the layout"
        assert bool((whole[used:nb] == FILLS[poison]).all()), f"{what}: wrote past the bytes needed"
    c.check_guards(what)
    for i, (t, s) in enumerate(zip(c.readonly, snaps)):
        assert fp.unchanged(t, s), f"{what}: read-only operand {i} changed"
    return c.results()


# --- 3a. exact-size workspaces between canaries --------------------------------------------------

@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", list(CASES))
def test_exact_size_workspace(name, shift):
    c = case(name)
    what = f"{name}, shift {shift}"
    run(c, shift, "ones", what)
    c.check(what)


# --- 3c. stale workspace bytes -------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_result_is_independent_of_stale_workspace_bytes(name):
    c = case(name)
    res = {}
    for poison in fp.POISONS:
        res[poison] = run(c, 0, poison, f"{name}, poison {poison}")
        if c.exact:
            c.check(f"{name}, poison {poison}")
    c.check(name)
    for poison, r in res.items():
        assert r == res["zero"], f"{name}: the result under poison {poison!r} differs from 'zero'"


# --- 3b. shapes that saturate the interior bounds -------------------------------------------------

def saturating(pattern, n):
    """(index vector, rows): n occurrences as a vector index."""
    rng = np.random.default_rng(n)
    if pattern == "distinct":     # U = n: the most chunk records, segment starts, nch entries
        return (rng.permutation(n) + 1).astype(np.int64), n
    if pattern == "same":         # one list of n: the most chain entries, padding and tiles
        return np.full(n, 3, np.int64), 200
    if pattern == "mixed":        # half in one column, the rest distinct
        I = (rng.permutation(n) + 1).astype(np.int64)
        I[rng.permutation(n)[:n // 2]] = 1
        return I, n
    assert pattern == "multichunk"  # n / (chunk + 1) columns of exactly chunk + 1 occurrences
    assert n % (CHUNK + 1) == 0
    return (rng.permutation(n) % (n // (CHUNK + 1)) + 1).astype(np.int64), 300


SATURATING = ([(p, n) for n in (255, 256, 257, 4095, 4096, 4097, 8193)
               for p in ("distinct", "same", "mixed")]
              + [("multichunk", 16 * (CHUNK + 1)), ("same", 1)])


@pytest.mark.parametrize("pattern,n", SATURATING)
def test_saturating_shapes(pattern, n):
    I, R = saturating(pattern, n)
    counts = np.bincount(I)
    if pattern == "distinct":
        assert counts.max() == 1 and len(np.unique(I)) == n
    elif pattern == "same" or pattern == "mixed":
        assert counts.max() >= max(n // 2, 1)
    else:
        assert (counts[1:n // (CHUNK + 1) + 1] == CHUNK + 1).all()
    long = CHUNK if counts.max() > CHUNK else 0
    what = f"{pattern} n={n}"
    for flags in (NT | EXACT, NT):
        c = SgdCase([(R, 16, 1)], n, flags, indices=[I], need_long=long, seed=n)
        run(c, 4, "ones", f"sgd {flags} {what}")
        c.check(f"sgd {flags} {what}")
    # ragged: the same entries in bags of 4 (the last one shorter)
    L = np.full(-(-n // 4), 4, np.int64)
    L[-1] = n - 4 * (len(L) - 1)
    c = RaggedCase([(R, 16, L, I)], False, seed=n, tail=5)
    run(c, 4, "ones", f"ragged {what}")
    c.check(f"ragged {what}")
    # AdaGrad, element-wise, a vector index: byte equality with the family's reference
    c = AdaVecCase(I, R, seed=n + 1)
    run(c, 4, "ones", f"adagrad {what}")
    c.check(f"adagrad {what}")


def test_ragged_call_with_an_empty_table():
    """Two tables, nnz 0 for the second: it takes no part and is not written."""
    rng = np.random.default_rng(2)
    L = mix_lengths(60, rng)
    empty = np.zeros(60, np.int64)
    for weighted in (False, True):
        c = RaggedCase([(200, 16, L, uniform_idx(rng, 200, (int(L.sum()),))),
                        (50, 8, empty, np.zeros(0, np.int64))], weighted)
        run(c, 100, "ones", "empty second table")
        c.check("empty second table")
        assert same(c.t[1]["tab"].host(), c.t[1]["base"])


# --- 3c, through the Python API: the cached workspaces, poisoned ----------------------------------

BIG = 1 << 23
API_POISONS = ["zero", "ones", "canary", "random"]


def poison_cache(keys, poison):
    """Fill the cache's own buffer of every key with the poison; returns the buffers."""
    out = []
    for key in keys:
        ws = upd._workspace(BIG, DEV, key)  # may be a larger leftover of an earlier test
        assert ws.numel() >= BIG
        fp.POISONS[poison](ws[:BIG])        # the layouts here start at its head and fit
        out.append(ws)
    return out


def api_problem():
    rng = np.random.default_rng(77)
    R, D, B, P = 700, 64, 600, 20
    base = rng.standard_normal((R, D)).astype(np.float32)
    small = rng.standard_normal((90, 32)).astype(np.float32)
    I, Is = zipf_idx(rng, R, (B, P)), zipf_idx(rng, 90, (B, 5))
    delta = rng.standard_normal((B, D)).astype(np.float32)
    dsmall = rng.standard_normal((B, 32)).astype(np.float32)
    assert np.bincount(I.ravel()).max() > CHUNK
    Lr, values, _ = hot_case(257, np.random.default_rng(7))
    return dict(R=R, D=D, B=B, P=P, base=base, small=small, I=I, Is=Is, delta=delta,
                dsmall=dsmall, L=Lr, values=values,
                rdelta=rng.standard_normal((257, D)).astype(np.float32),
                w=rng.standard_normal(len(values)).astype(np.float32))


def api_paths(p):
    """name -> (workspace keys of embtab/update.py, callable returning the result tensors)."""
    St = et.Static(p["D"])

    def table():
        return et.SimpleEmbedding(dev(p["base"]), St)

    def fixed(A):
        return et.SparseEmbeddingUpdate(A.lookup_type, dev(p["delta"]), dev(p["I"]))

    def descent(exact):
        A = table()
        et.update_(et.Descent(ETA), A, fixed(A), exact=exact)
        return [A.data]

    def rag(weighted):
        A = table()
        Rg = et.RaggedIndices(dev(p["values"]), dev(colptr_of(p["L"])))
        g = et.SparseEmbeddingUpdate(A.lookup_type, dev(p["rdelta"]), Rg,
                                     dev(p["w"]) if weighted else None)
        et.update_(et.Descent(ETA), A, g)
        return [A.data]

    def ada(rowwise):
        A = table()
        opt = et.AdaGrad(ETA, 1e-8, rowwise=rowwise)
        et.update_(opt, A, fixed(A))
        return [A.data, opt.state(A)]

    def two_tables():
        A, S = table(), et.SimpleEmbedding(dev(p["small"]), et.Static(32))
        g = [fixed(A), et.SparseEmbeddingUpdate(S.lookup_type, dev(p["dsmall"]), dev(p["Is"]))]
        return [A, S], g

    def multi(telemetry):
        tabs, g = two_tables()
        et.update_(et.Descent(ETA), tabs, g, [et.Indexer(), et.Indexer()],
                   telemetry_cb=(lambda: None) if telemetry else None)
        return [t.data for t in tabs]

    def indexer():
        ix = et.index_(et.Indexer(), dev(p["I"]), p["R"])
        return [ix.cumulative, ix.map]

    return {
        "descent exact": (["sgd"], lambda: descent(True)),
        "descent split": (["sgd"], lambda: descent(False)),
        "ragged": (["ragged_sgd"], lambda: rag(False)),
        "weighted": (["weighted_sgd"], lambda: rag(True)),
        "adagrad": (["adagrad0"], lambda: ada(False)),
        "adagrad rowwise": (["adagrad0"], lambda: ada(True)),
        # Static(64) and Static(32) Float32 tables are one (path, eltype) group: one call
        "multi-table": (["sgd0"], lambda: multi(False)),
        "multi-table two calls": (["sgd0"], lambda: multi(True)),
        "index_": (["index"], indexer),
    }


API_NAMES = ["descent exact", "descent split", "ragged", "weighted", "adagrad",
             "adagrad rowwise", "multi-table", "multi-table two calls", "index_"]


@pytest.mark.parametrize("name", API_NAMES)
def test_cached_workspace_poisoned_through_the_python_api(name):
    p = api_problem()
    keys, f = api_paths(p)[name]
    res = {}
    for poison in API_POISONS:
        bufs = poison_cache(keys, poison)
        out = f()
        torch.cuda.synchronize()
        res[poison] = [fp.snapshot(t) for t in out]
        for key, ws in zip(keys, bufs):  # the call used the poisoned buffer, not a new one
            assert upd._workspace(1, DEV, key) is ws
            if poison != "random":
                assert not bool((ws[:BIG] == ws[0]).all()), f"{name}: workspace {key!r} unused"
    assert et.check_errors() == 0
    for poison in API_POISONS:
        assert res[poison] == res["zero"], f"{name}: poison {poison!r} changed the result"
    # and the result is the reference's where the path is exact
    if name in ("descent exact", "descent split"):
        got = np.frombuffer(res["zero"][0], np.float32).reshape(p["base"].shape)
        check_sgd_table(got, p["base"], p["delta"], p["I"], name == "descent exact", name)
    if name == "index_":
        cum, mp = orc().index_build(p["I"], p["R"])
        assert res["zero"] == [cum.tobytes(), mp.tobytes()]
    if name.startswith("multi-table"):
        for k, (b, d, I) in enumerate(((p["base"], p["delta"], p["I"]),
                                       (p["small"], p["dsmall"], p["Is"]))):
            got = np.frombuffer(res["zero"][k], np.float32).reshape(b.shape)
            check_sgd_table(got, b, d, I, True, f"{name} table {k}")


@pytest.mark.parametrize("exact", [True, False])
def test_phased_update_with_poisoned_workspaces(exact):
    p = api_problem()
    res = {}
    for poison in API_POISONS:
        A = et.SimpleEmbedding(dev(p["base"]), et.Static(p["D"]))
        S = et.SimpleEmbedding(dev(p["small"]), et.Static(32))
        grads = [et.SparseEmbeddingUpdate(A.lookup_type, dev(p["delta"]), dev(p["I"])),
                 et.SparseEmbeddingUpdate(S.lookup_type, dev(p["dsmall"]), dev(p["Is"]))]
        ph = et.PhasedUpdate([A, S], grads, exact=exact)
        assert ph._calls
        for call in ph._calls:  # between construction and index_
            fp.POISONS[poison](call[4])
        ph.index_()
        ph.update_(et.Descent(ETA))
        torch.cuda.synchronize()
        res[poison] = [fp.snapshot(A.data), fp.snapshot(S.data)]
    assert et.check_errors() == 0
    for poison in API_POISONS:
        assert res[poison] == res["zero"], f"poison {poison!r} changed the result"
    for k, (b, d, I) in enumerate(((p["base"], p["delta"], p["I"]),
                                   (p["small"], p["dsmall"], p["Is"]))):
        got = np.frombuffer(res["zero"][k], np.float32).reshape(b.shape)
        check_sgd_table(got, b, d, I, exact, f"phased table {k}")


# --- 3d. destinations ----------------------------------------------------------------------------

DIMS = [20, 24, 80, 7, 128]
LAYOUTS = ["pad7", "vec"]


def guarded_dst(B, cols, kind, layout):
    kw = dict(ld=-(-(cols + 12) // 8) * 8, left=8) if layout == "vec" else {}
    return fp.guarded_matrix(B, cols, TORCH[kind], DEV, pad_cols=7, guard_rows=1, **kw)


def check_dst(intact, what):
    ok, where = intact()
    assert ok, f"{what}: wrote outside the destination at buffer (row, byte) {where}"


@functools.lru_cache(maxsize=None)
def lookup_inputs(dim):
    rng = np.random.default_rng(900 + dim)
    B = 131
    L = mix_lengths(B, rng)
    values = uniform_idx(rng, 700, (int(L.sum()),))
    table = rng.standard_normal((700, dim)).astype(np.float32)
    w = rng.standard_normal(len(values)).astype(np.float32)
    cp = colptr_of(L)
    ragged_ref = expect_lookup(orc(), table, values, ranges_of(cp, len(values)))
    return dict(B=B, L=L, values=values, table=table, w=w, cp=cp, ragged=ragged_ref,
                weighted=wr.forward(table, values, cp, w)[0],
                mean=wr.forward(table, values, cp, None, "mean")[0])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dim", DIMS)
def test_ragged_weighted_and_mean_lookup_destinations(dim, layout):
    q = lookup_inputs(dim)
    A = et.SimpleEmbedding(dev(q["table"]))
    Rg = et.RaggedIndices(dev(q["values"]), dev(q["cp"]))
    dw = dev(q["w"])
    kinds = {"ragged": Rg, "weighted": et.WeightedIndices(Rg, dw),
             "mean": et.WeightedIndices(Rg, mode="mean")}
    before = [fp.snapshot(t) for t in (A.data, Rg.values, Rg.colptr, dw)]
    for name, I in kinds.items():
        buf, dst, intact = guarded_dst(q["B"], dim, "f32", layout)
        et.lookup_(dst, A, I)
        assert same(host(dst), q[name]), name
        check_dst(intact, f"{name} dim {dim}")
        assert not same(q[name], np.zeros_like(q[name]))
    # maplookup_ with 3 prepended rows: the three kinds side by side, the prepended rows kept
    k = 3
    for name, I in kinds.items():
        buf, dst, intact = guarded_dst(q["B"], k + 2 * dim, "f32", layout)
        dst.fill_(-3.0)
        et.maplookup_(et.PreallocationStrategy(k), dst, [A, A], [I, I])
        h = host(dst)
        assert (h[:, :k] == -3.0).all(), name
        assert same(h[:, k:k + dim], q[name]) and same(h[:, k + dim:], q[name]), name
        check_dst(intact, f"maplookup_ {name} dim {dim}")
    for t, s in zip((A.data, Rg.values, Rg.colptr, dw), before):
        assert fp.unchanged(t, s), "a lookup changed its table, indices or weights"
    assert et.check_errors() == 0


QUANT = [(8, 128, False), (8, 20, False), (8, 24, True), (4, 80, False), (4, 128, True),
         (4, 24, False)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bits,dim,split", QUANT)
def test_quantised_lookup_destinations(bits, dim, split, layout):
    rng = np.random.default_rng(bits * 1000 + dim)
    R, B, P = 300, 77, 5
    x = rng.standard_normal((R, dim)).astype(np.float32)
    ldb = et.quant.default_ld_bytes(dim, bits, split)
    rows, hdr = qr.build_rows(x, bits, ldb, split, fill=0xA5)
    packed = dev(rows)
    dh = dev(hdr) if split else None
    Q = et.QuantizedEmbedding(packed, dim, bits, dh)
    T = qr.dequantize(*qr.split_rows(rows, dim, bits, hdr))
    idx = uniform_idx(rng, R, (B, P))
    L = mix_lengths(B, rng)
    values = uniform_idx(rng, R, (int(L.sum()),))
    cp = colptr_of(L)
    acc_fixed = qr.pooled_matrix(T, idx)
    acc_ragged = expect_lookup(orc(), T, values, ranges_of(cp, len(values)))
    dI, Rg = dev(idx), et.RaggedIndices(dev(values), dev(cp))
    before = [fp.snapshot(t) for t in (packed, dI, Rg.values, Rg.colptr)] + (
        [fp.snapshot(dh)] if split else [])
    for out in ("f32", "f16", "bf16"):
        for I, acc in ((dI, acc_fixed), (Rg, acc_ragged)):
            buf, dst, intact = guarded_dst(B, dim, out, layout)
            et.lookup_(dst, Q, I)
            want = qr.store(acc, out)
            assert fp.snapshot(dst) == want.tobytes(), (out, type(I).__name__)
            check_dst(intact, f"INT{bits} dim {dim} -> {out}")
    after = [packed, dI, Rg.values, Rg.colptr] + ([dh] if split else [])
    for t, s in zip(after, before):
        assert fp.unchanged(t, s), "a quantised lookup changed its table, headers or indices"
    assert acc_fixed.any() and et.check_errors() == 0


@pytest.mark.parametrize("dim,kind", [(20, "f32"), (128, "f32"), (7, "f32"), (24, "bf16"),
                                      (80, "f64")])
def test_weight_gradient_footprint(dim, kind):
    """dw into a guarded vector of exactly nnz entries (a capacity tail of 9 included): the
    family's bound on the values (tests/test_gpu_weighted.py), +0 in the tail, canaries intact,
    table, gradient and indices unchanged."""
    from embtab.weighted import weight_grad

    table, delta, values, colptr, bf16 = wr.wgrad_case(dim, kind, B=131)
    vals = np.concatenate([values, values[:9]])
    A = et.SimpleEmbedding(dev(table, kind))
    dd = dev(delta, kind)
    Rg = et.RaggedIndices(dev(vals), dev(colptr))
    C = torch.float64 if kind == "f64" else torch.float32
    g = GuardedVec(len(vals), C)
    out = g.raw.view(C)
    before = [fp.snapshot(t) for t in (A.data, dd, Rg.values, Rg.colptr)]
    weight_grad(A, dd, Rg, out=out)
    torch.cuda.synchronize()
    g.check(f"dw dim {dim} {kind}")
    dw = g.host()
    assert same(dw[len(values):], np.zeros(9, dw.dtype))
    ref, mag = wr.weight_grad_f64(table, delta, values, colptr, bf16)
    u = 2.0 ** -53 if kind == "f64" else 2.0 ** -24
    assert (np.abs(dw[:len(values)].astype(ref.dtype) - ref) <= wr.gamma(dim + 1, u) * mag).all()
    assert dw[:len(values)].any()
    for t, s in zip((A.data, dd, Rg.values, Rg.colptr), before):
        assert fp.unchanged(t, s)
    assert et.check_errors() == 0


# --- 3d. updated tables and states: pad columns and guard rows --------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dim", DIMS)
def test_updated_table_footprints(dim, layout):
    """Every update family on a table with ld_table > dim between guard rows (and, for
    AdaGrad, a state with ld_state > dim): exact SGD through a chain of 340 occurrences, split
    SGD, ragged and weighted SGD, element-wise and row-wise AdaGrad."""
    rng = np.random.default_rng(dim)
    R, B, P = 150, 170, 4

    def chain_idx(rng_, R_, shape):
        I = uniform_idx(rng_, R_, shape)
        I[:, :2] = 11  # 340 occurrences: a hand-scheduled chain in the exact mode
        return I

    for flags in (NT | EXACT, NT, EXACT):
        c = SgdCase([(R, dim, P)], B, flags, chain_idx, seed=dim, layout=layout)
        assert np.bincount(c.I[0].ravel())[11] >= 340
        run(c, 0, "ones", f"sgd flags {flags} dim {dim}")
        c.check(f"sgd flags {flags} dim {dim} {layout}")
    L = mix_lengths(B, rng, extra=[300])
    values = uniform_idx(rng, R, (int(L.sum()),))
    j = int(np.nonzero(L == 300)[0][0])
    cp = colptr_of(L)
    values[cp[j] - 1:cp[j + 1] - 1] = 11
    for weighted in (False, True):
        c = RaggedCase([(R, dim, L, values)], weighted, seed=dim, layout=layout)
        run(c, 0, "ones", f"ragged weighted={weighted} dim {dim}")
        c.check(f"ragged weighted={weighted} dim {dim} {layout}")
    for rowwise in (False, True):
        c = AdaCase(rowwise, seed=dim, layout=layout, dims=(dim, dim))
        run(c, 0, "ones", f"adagrad rowwise={rowwise} dim {dim}")
        c.check(f"adagrad rowwise={rowwise} dim {dim} {layout}")


@pytest.mark.parametrize("exact", [True, False])
def test_paged_table_last_page_footprint(exact):
    """A paged table (cols_per_page 64, 150 columns: the last page holds 22) whose pages lie
    in one guarded allocation, guard rows after the partly filled last page."""
    rng = np.random.default_rng(64)
    R, D, cpp, B, P = 150, 64, 64, 170, 4
    base = rng.standard_normal((R, D)).astype(np.float32)
    I = uniform_idx(rng, R, (B, P))
    I[:, 0] = 150   # the last column of the last page, 170 occurrences
    I[:, 1:3] = 140  # a chain of 340 in the last page
    delta = rng.standard_normal((B, D)).astype(np.float32)
    # pages back to back would hide an overrun of one page in the next: each page gets its
    # own guarded matrix, the last one only 22 rows
    pages = [Guarded(base[s:s + cpp], layout="vec") for s in range(0, R, cpp)]
    assert pages[-1].view.shape[0] == 22
    # a paged table's columns are ld_table apart within a page: all pages share one ld
    ld = pages[0].ld
    ptrs = torch.tensor([p.ptr for p in pages], dtype=torch.int64, device=DEV)
    dI, dd = dev(I), dev(delta)
    descs = (_lib.UpdateDesc * 1)(_lib.UpdateDesc(ptrs.data_ptr(), ld, R, D, P, dd.data_ptr(), D,
                                                  dI.data_ptr(), P, B, cpp))
    Lb = _lib.load()
    nb = ctypes.c_int64(0)
    _lib.check(Lb.et_sgd_workspace_size(ctypes.addressof(descs), 1, ctypes.byref(nb)))
    buf, ws = fp.guarded_bytes(nb.value, 100, DEV)
    ws.fill_(0xFF)
    before = [fp.snapshot(t) for t in (ptrs, dI, dd)]
    _lib.check(Lb.et_sparse_sgd(_lib.ET_F32, ctypes.addressof(descs), 1, ETA,
                                NT | (EXACT if exact else 0), ws.data_ptr(), nb.value,
                                _lib.stream_handle()))
    torch.cuda.synchronize()
    assert et.check_errors() == 0
    fp.assert_guards(buf, ws, "paged workspace")
    for k, p in enumerate(pages):
        p.check(f"page {k}")
    got = np.concatenate([p.host() for p in pages])
    check_sgd_table(got, base, delta, I, exact, "paged table")
    for t, s in zip((ptrs, dI, dd), before):
        assert fp.unchanged(t, s)


@pytest.mark.parametrize("dim", DIMS)
def test_updated_table_footprints_through_the_python_objects(dim):
    """The same footprints through et.update_: SimpleEmbedding and AdaGrad.set_state take a
    strided view, so the guarded table (and state) is handed over as it is."""
    rng = np.random.default_rng(300 + dim)
    R, B, P = 150, 170, 4
    base = rng.standard_normal((R, dim)).astype(np.float32)
    I = uniform_idx(rng, R, (B, P))
    I[:, :2] = 11
    delta = rng.standard_normal((B, dim)).astype(np.float32)
    L = mix_lengths(B, rng, extra=[300])
    values = uniform_idx(rng, R, (int(L.sum()),))
    cp = colptr_of(L)
    w = rng.standard_normal(len(values)).astype(np.float32)
    bag = np.repeat(np.arange(B), L)
    dI, dd, dv, dc, dw = dev(I), dev(delta), dev(values), dev(cp), dev(w)
    before = [fp.snapshot(t) for t in (dI, dd, dv, dc, dw)]
    lt = et.Static(dim)
    fused = dim * 4 <= 512  # tables.fused_update_path of a Static table
    tab = Guarded(base)

    def fresh():
        tab.restore()
        A = et.SimpleEmbedding(tab.view, lt)
        assert A.ld == tab.ld > dim and et.tables.fused_update_path(A) == fused
        return A

    for exact in (True, False):
        A = fresh()
        et.update_(et.Descent(ETA), A, et.SparseEmbeddingUpdate(lt, dd, dI), exact=exact)
        tab.check(f"Descent exact={exact} dim {dim}")
        check_sgd_table(tab.host(), base, delta, I, exact, f"Descent exact={exact}")
    Rg = et.RaggedIndices(dv, dc)
    A = fresh()
    et.update_(et.Descent(ETA), A, et.SparseEmbeddingUpdate(lt, dd, Rg))
    tab.check(f"ragged dim {dim}")
    ref = base.copy()
    orc().sgd(ref, delta[bag], values, ETA, fused=fused)
    assert same(tab.host(), ref)
    A = fresh()
    et.update_(et.Descent(ETA), A, et.SparseEmbeddingUpdate(lt, dd, Rg, dw))
    tab.check(f"weighted dim {dim}")
    E, cov = wr.expanded_gradient(delta, w, cp, len(values))
    ref = base.copy()
    orc().sgd(ref, E[cov], values[cov], ETA, fused=fused)
    assert same(tab.host(), ref) and not same(ref, base)
    kind = KINDS["f32"]
    state0 = rng.random((R, dim)).astype(np.float32)
    st = Guarded(state0)
    A = fresh()
    opt = et.AdaGrad(ETA, 1e-8)
    opt.set_state(A, st.view)
    et.update_(opt, A, et.SparseEmbeddingUpdate(lt, dd, dI))
    tab.check(f"AdaGrad table dim {dim}")
    st.check(f"AdaGrad state dim {dim}")
    t2, s2 = base.copy(), state0.copy()
    ref_step(kind, t2, s2, delta, lists_fixed(I, R), ETA, 1e-8)
    assert same(tab.host(), t2) and same(st.host(), s2)
    row0 = rng.random(R).astype(np.float32)
    g = GuardedVec(R, torch.float32)
    g.raw.copy_(dev(row0).view(torch.uint8))
    A = fresh()
    opt = et.AdaGrad(ETA, 1e-8, rowwise=True)
    opt.set_state(A, g.raw.view(torch.float32))
    et.update_(opt, A, et.SparseEmbeddingUpdate(lt, dd, dI))
    tab.check(f"row-wise AdaGrad table dim {dim}")
    g.check(f"row-wise AdaGrad state dim {dim}")
    rs, rw = rowwise_bounds(kind, base, row0, delta, lists_fixed(I, R), tab.host(), g.host(), ETA,
                            1e-8)
    assert rs <= 1.0 and rw <= 1.0, (rs, rw)
    for t, s in zip((dI, dd, dv, dc, dw), before):
        assert fp.unchanged(t, s), "an update changed its gradient, indices, colptr or weights"
    assert et.check_errors() == 0
