"""Weighted sparse AdaGrad at the edges: special values in the weights and their products
(compared with the numpy reference through tests/special_values.py: NaN by position,
everything else by bits), and the memory footprint of et_weighted_adagrad, following
tests/test_gpu_footprint.py (an exact-size workspace between guard bytes, canaries around
every operand, the weights included, and read-only inputs unchanged)."""
import ctypes

import numpy as np
import pytest
import torch

import embtab as et
import footprint as fp
import special_values as sv
import weighted_adagrad_ref as war
import weighted_ref as wr
from embtab import _lib
from test_gpu_adagrad import CHUNK, EPS, ETA, KINDS, R, ragged_case
from test_gpu_footprint import Case, Guarded, GuardedVec, run
from test_gpu_ragged import dev, host, same

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COLS = [1, 2, 4, 6, 7, 8]  # 1-based columns the ordinary indices never hold


# --- special values ---------------------------------------------------------------------------------

def special_case(name, dim, garbage):
    """ragged_case with six short bags rewritten to one dedicated column each:
      1  every weight +0 on finite gradients: g = +0, the column and its state (-0) are written
      2  every weight -0
      4  weight 0 on a gradient with Inf at the planted features: NaN there only
      6  an Inf weight on a finite gradient with a zero at the planted features
      7  w = 2^-20 on delta = 2^-120: subnormal products 2^-140, kept (table 0, state 0)
      8  ordinary weights (what the others must not disturb)
    `garbage` is what the weights of entries no bag covers hold."""
    kind = KINDS[name]
    tk = "bf16" if name == "bf16" else name
    pal = sv.palette(tk)["values"]
    rng = np.random.default_rng([31, dim])
    L, values, colptr = ragged_case(rng)
    table = kind.fromf(rng.standard_normal((R, dim)))
    state = rng.random((R, dim)).astype(np.float32)
    delta = kind.fromf(rng.standard_normal((len(L), dim)))
    w = war.case_weights(rng, values, colptr, np.float32)
    first = np.nonzero(L > 0)[0][0]
    pick = [j for j in np.nonzero((L >= 2) & (L <= 12))[0] if j != first][:len(COLS)]
    b = dict(zip(COLS, pick))
    span = {c: slice(int(colptr[j]) - 1, int(colptr[j + 1]) - 1) for c, j in b.items()}
    for c in COLS:
        values[span[c]] = c
    feats = sv.feats_for(dim)
    w[span[1]], w[span[2]] = 0.0, -0.0
    state[0], state[1] = -0.0, -0.0
    w[span[4]] = 0.0
    delta[b[4], feats] = pal["inf"]
    w[span[6]] = np.inf
    delta[b[6], feats] = pal["zero"]
    w[span[7]] = 2.0 ** -20
    delta[b[7]] = kind.fromf(np.full(dim, 2.0 ** -120))
    table[6] = kind.fromf(np.zeros(dim))
    state[6] = 0.0
    w[np.isnan(w)] = garbage
    return {"kind": kind, "tk": tk, "table": table, "state": state, "delta": delta,
            "values": values, "colptr": colptr, "weights": w, "feats": feats}


@pytest.mark.parametrize("name,dim", [("f32", 128), ("bf16", 7)])
def test_special_values(name, dim):
    got = {}
    for garbage in (np.nan, np.inf, 3.0e38):
        c = special_case(name, dim, garbage)
        kind = c["kind"]
        A = et.SimpleEmbedding(kind.dev(c["table"]))
        opt = et.AdaGrad(ETA, EPS, weighted=True)
        opt.state(A).copy_(dev(c["state"]))
        Rg = et.RaggedIndices(dev(c["values"]), dev(c["colptr"]))
        et.update_(opt, A, et.SparseEmbeddingUpdate(A.lookup_type, kind.dev(c["delta"]), Rg,
                                                    dev(c["weights"])))
        got[garbage] = (host(A.data), host(opt.state(A)))
        assert et.check_errors() == 0
    c = special_case(name, dim, np.nan)
    kind, tk, feats = c["kind"], c["tk"], c["feats"]
    table, state = c["table"].copy(), c["state"].copy()
    lists, g_of = war.ref_step(kind, table, state, c["delta"], c["values"], c["colptr"],
                               c["weights"])
    # what the reference holds, so the comparison below pins what it claims to pin
    rest = np.setdiff1d(np.arange(dim), feats)
    assert same(g_of[0], np.zeros(dim, np.float32)) and sv.bits_of(state[:2], "f32").max() == 0
    assert np.isnan(g_of[3][feats]).all() and not np.isnan(g_of[3][rest]).any()
    assert np.isinf(g_of[5][rest]).all() and np.isnan(g_of[5][feats]).all()
    assert (g_of[6] != 0).all() and (np.abs(g_of[6]) < 2.0 ** -126).all()  # subnormal, kept
    assert sv.census(table[6], tk)["-0"] == 0 and (kind.toC(table[6]) < 0).all()
    assert not np.isnan(kind.toC(table[7])).any()
    t_nan, s_nan = got[np.nan]
    assert sv.same_special(t_nan, table, tk) and sv.same_special(s_nan, state, "f32")
    # the weights of entries no bag covers change nothing, whatever they hold
    for garbage in (np.inf, 3.0e38):
        assert sv.same_special(got[garbage][0], t_nan, tk, copy=True)
        assert sv.same_special(got[garbage][1], s_nan, "f32", copy=True)


# --- footprint --------------------------------------------------------------------------------------

class WeightedAdaCase(Case):
    """et_weighted_adagrad over one weighted ragged Float32 table (ragged_case: a list longer
    than a chunk, so partial rows are written); table and state in guarded matrices, the
    gradient in one too, values, colptr and a weights buffer of exactly nnz elements between
    canaries."""
    exact = True

    def __init__(self, dim, layout, seed=51):
        rng = np.random.default_rng(seed)
        self.kind = KINDS["f32"]
        L, values, colptr = ragged_case(rng)
        self.values, self.colptr = values, colptr
        assert (values == 14).sum() > CHUNK
        self.base = rng.standard_normal((R, dim)).astype(np.float32)
        self.state0 = rng.random((R, dim)).astype(np.float32)
        self.delta = rng.standard_normal((len(L), dim)).astype(np.float32)
        self.weights = war.case_weights(rng, values, colptr, np.float32)
        self.tab, self.st = Guarded(self.base, layout=layout), Guarded(self.state0, layout=layout)
        self.guarded = [self.tab, self.st]
        self.gdelta = Guarded(self.delta, layout=layout)
        self.gvals = GuardedVec(len(values), torch.int64)
        self.gcp = GuardedVec(len(colptr), torch.int64)
        self.gw = GuardedVec(len(values), torch.float32)
        for g, a in ((self.gvals, values), (self.gcp, colptr), (self.gw, self.weights)):
            g.raw.copy_(dev(a).view(torch.uint8))
        self.inputs = [self.gdelta, self.gvals, self.gcp, self.gw]
        self.readonly = [self.gdelta.view, self.gvals.raw, self.gcp.raw, self.gw.raw]
        A = _lib.WeightedAdaGradDesc
        self.descs = (A * 1)(A(self.tab.ptr, self.tab.ld, R, dim, 1, self.gdelta.ptr,
                               self.gdelta.ld, self.gvals.ptr, 1, len(L), 0, self.gcp.ptr,
                               len(values), self.st.ptr, self.st.ld, self.gw.ptr))

    def size_fn(self):
        return _lib.load().et_weighted_adagrad_workspace_size

    def status(self, ptr, nbytes):
        return _lib.load().et_weighted_adagrad(_lib.ET_F32, ctypes.addressof(self.descs), 1, ETA,
                                               EPS, _lib.ET_FLAG_NONTEMPORAL, ptr, nbytes,
                                               _lib.stream_handle())

    def call(self, ptr, nbytes):
        _lib.check(self.status(ptr, nbytes))

    def check_guards(self, what):
        super().check_guards(what)
        for i, g in enumerate(self.inputs):
            g.check(f"{what}: guarded input {i}")

    def check(self, what):
        t, s = self.base.copy(), self.state0.copy()
        war.ref_step(self.kind, t, s, self.delta, self.values, self.colptr, self.weights)
        assert same(self.tab.host(), t) and same(self.st.host(), s), what
        assert not same(t, self.base) and not same(s, self.state0), what


@pytest.mark.parametrize("dim,layout", [(128, "vec"), (20, "vec"), (7, "pad7")])
def test_footprint(dim, layout):
    c = WeightedAdaCase(dim, layout)
    what = f"weighted adagrad dim {dim} {layout}"
    ones = run(c, 0, "ones", what)
    c.check(what)
    zero = run(c, 0, "zero", what)
    c.check(what)
    assert ones == zero, f"{what}: the result depends on stale workspace bytes"
    shifted = run(c, 100, "ones", what)
    assert shifted == zero
    # one byte short: ET_ERR_WORKSPACE and nothing written, anywhere.  The size told carries
    # 256 bytes of slack for the layout's alignment (as et_adagrad_workspace_size's): a
    # workspace `pad` bytes before a 256-byte boundary needs bytes - 256 + pad of them, so
    # bytes - 1 itself is one short for the worst alignment only (pad 255, one byte past a
    # boundary); both alignments are tried.
    nb = c.size()
    for shift in (0, 1):
        need = nb - 256 + (256 - shift) % 256
        buf, whole = fp.guarded_bytes(nb, shift, DEV)
        whole.fill_(0xFF)
        c.restore()
        assert c.status(whole.data_ptr(), need - 1) == -3, shift
        torch.cuda.synchronize()
        assert b"%d bytes" % need in _lib.load().et_last_error()
        fp.assert_guards(buf, whole, what)
        assert bool((whole == 0xFF).all())
        assert same(c.tab.host(), c.base) and same(c.st.host(), c.state0)
        c.check_guards(what)
    assert et.check_errors() == 0
