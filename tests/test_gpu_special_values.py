"""Inf, NaN, subnormals, signed zeros and values at the edge of overflow through every kernel
family, against the same references as the ordinary-value tests.  The cases come from
tests/special_values.py; tests/test_special_values_host.py shows on the CPU that each of them
can fail (census, NaN cap, clean share, rejected mutations).

Comparisons are ``same_special``: equal NaN positions and byte equality everywhere else (the
sign of Inf and of zero, every subnormal bit); pure copies (the gather, one-entry bags of a
type that is its own accumulator) are compared byte for byte, NaN payload included.  Every
index is in range or a counted out-of-range index; every test ends with the error counter at
the planted count."""
import numpy as np
import pytest
import torch

import embtab as et
import special_values as sv
import weighted_ref as wr
from embtab.tables import Dynamic, Static, fused_update_path

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev(x, kind="f32"):
    x = np.ascontiguousarray(x)
    if kind == "bf16":
        return torch.from_numpy(x.view(np.int16)).to(DEV).view(torch.bfloat16)
    return torch.from_numpy(x).to(DEV)


def host(x):
    if x.dtype == torch.bfloat16:
        return x.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return x.cpu().numpy()


def ragged(values, colptr):
    return et.RaggedIndices(dev(values), dev(colptr))


# --- forward: fixed pool, gather, integers ------------------------------------------------------

@pytest.mark.parametrize("kind,dim", sv.FIXED_CASES)
def test_fixed_pool_lookup(oracle, kind, dim):
    tk = sv.table_kind(kind)
    et.check_errors()
    for P in sv.POOLS:
        case = sv.fixed_case(kind, dim, P)
        A = et.SimpleEmbedding(dev(case["table"], tk))
        I = dev(case["values"].reshape(sv.FWD_B, P))
        if kind == "f16acc":
            dst = torch.empty((sv.FWD_B, dim), dtype=torch.float16, device=DEV)
            et.maplookup_(et.PreallocationStrategy(0), dst, [A], [I], f16_fp32_acc=True)
        else:
            dst = et.lookup(A, I)
        want = sv.forward_ref(oracle, case["table"], case["values"], case["colptr"], kind)
        # a bag of one entry is a copy where the type is its own accumulator
        copy = P == 1 and kind in ("f32", "f64", "f16")
        assert sv.same_special(host(dst), want, tk, copy=copy), (kind, dim, P)
        assert et.check_errors() == case["events"]


@pytest.mark.parametrize("kind,dim", [("f32", 128), ("f32", 20), ("f32", 7), ("f64", 16),
                                      ("f16", 256), ("bf16", 128)])
def test_vector_index_gather_is_a_copy(oracle, kind, dim):
    table, rows = sv.forward_table(kind, dim, 40 + dim)
    n = table.shape[0]
    v = np.concatenate([np.arange(1, n + 1), np.random.default_rng(4).integers(1, n + 1, 301 - n)])
    got = host(et.lookup(et.SimpleEmbedding(dev(table, kind)), dev(v.astype(np.int64))))
    assert sv.same_special(got, oracle.gather(table, v, bf16=kind == "bf16"), kind, copy=True)
    assert got.tobytes() == table[v - 1].tobytes()
    assert et.check_errors() == 0


@pytest.mark.parametrize("kind", ["i32", "i64"])
def test_integer_sums_wrap(kind):
    table, I, want = sv.int_wrap_case(kind)
    got = host(et.lookup(et.SimpleEmbedding(dev(table)), dev(I)))
    assert got.tobytes() == want.tobytes()
    assert et.check_errors() == 0


# --- forward: ragged, weighted, mean ----------------------------------------------------------------

@pytest.mark.parametrize("dim", sv.RAGGED_DIMS)
def test_ragged_weighted_and_mean_lookup(oracle, dim):
    case = sv.ragged_case(dim)
    table, cp = case["table"], case["colptr"]
    A = et.SimpleEmbedding(dev(table))
    et.check_errors()
    got = host(et.lookup(A, ragged(case["values"], cp)))
    want = sv.forward_ref(oracle, table, case["values"], cp, "f32")
    assert sv.same_special(got, want, "f32")
    one = np.nonzero(np.diff(cp) == 1)[0]
    assert len(one) >= 10 and sv.same_special(got[one], want[one], "f32", copy=True)
    assert et.check_errors() == case["events"]
    # weights from the palette on in-range entries (0 * Inf is NaN: include/embtab.h)
    w, values, _ = sv.forward_weights(case, np.float32, 7)
    got = host(et.lookup(A, et.WeightedIndices(ragged(values, cp), dev(w))))
    assert sv.same_special(got, wr.forward(table, values, cp, w)[0], "f32")
    assert et.check_errors() == case["events"]
    # mean mode: bags of 3 on subnormal rows
    values, _ = sv.mean_values(case)
    got = host(et.lookup(A, et.WeightedIndices(ragged(values, cp), mode="mean")))
    assert sv.same_special(got, wr.forward(table, values, cp, mode="mean")[0], "f32")
    assert et.check_errors() == case["events"]


# --- sparse SGD, exact mode: chunk pass, early, regular and streamed chains ---------------------------

@pytest.mark.parametrize("static", [True, False])
def test_exact_sgd_chains(oracle, static):
    """The streamed-loop shape of test_gpu_paged_chains.py with special values in the gradient
    of 8 bags and in the tables (special_values.sgd_case): every table whole, against
    oracle.sgd.  The +Inf bag meets chains of S > 1 in a partial entry (r < S), where a
    masked fma slot would turn the Inf sum into NaN."""
    from test_gpu_paged_chains import EC_MAX_ROWS, ColumnPointerTable, _chain_shape, _dense

    case = sv.sgd_case()
    D = sv.SGD_D
    gen = torch.Generator(device=DEV)
    gen.manual_seed(607)
    tabs = []
    for (R, cpp), x in zip(sv.SGD_SPEC, case["tables"]):
        t = dev(x)
        tabs.append(et.SimpleEmbedding(t, Static(D) if static else Dynamic) if cpp == 0 else
                    et.SplitEmbedding(t, cpp) if cpp > 1 else ColumnPointerTable(t, D + 4, gen))
    dd = dev(case["delta"])
    idx = [dev(I) for I in case["idx"]]
    grads = [et.SparseEmbeddingUpdate(A.lookup_type, dd[:, k * D:(k + 1) * D], i)
             for k, (A, i) in enumerate(zip(tabs, idx))]
    et.check_errors()
    et.update_(et.Descent(sv.SGD_ETA), tabs, grads)  # default (exact) mode
    torch.cuda.synchronize()
    streamed = early = partial = 0
    for k, ((R, _), A, I) in enumerate(zip(sv.SGD_SPEC, tabs, idx)):
        ref = case["tables"][k].copy()
        oracle.sgd(ref, np.ascontiguousarray(case["delta"][:, k * D:(k + 1) * D]),
                   case["idx"][k], sv.SGD_ETA, fused=fused_update_path(A))
        got = host(A.data if isinstance(A, et.SimpleEmbedding) else _dense(A))
        assert sv.same_special(got, ref, "f32"), (k, R, np.argwhere(
            got.view(np.uint32) != ref.view(np.uint32))[:8].tolist())
        counts = torch.bincount(I.view(-1), minlength=R + 1)[1:]
        for c in torch.nonzero(counts > sv.CHUNK).view(-1).tolist():
            S = _chain_shape(I, c + 1)[0]
            early += R <= EC_MAX_ROWS
            streamed += R > EC_MAX_ROWS and S >= 8
            runs = (case["idx"][k][case["bags"]] == c + 1).sum(1)
            partial += bool(S > 1 and (runs % S != 0).any() and runs.all())
    assert streamed >= 3 and early >= 3 and partial >= 4, (streamed, early, partial)
    assert et.check_errors() == 0


# --- queued multi-table launch ------------------------------------------------------------------------

def test_queued_multi_table_launch(oracle):
    """et_maplookup_prealloc_q over two fabric-class and two cache-class tables; the
    destination starts from a finite sentinel, so a NaN in it was computed."""
    import ctypes

    from embtab import _lib
    from test_gpu_lookup_order import Launch, _block, _block_is_zero

    cases = sv.queued_cases()
    B, P, D = sv.QUEUED_B, sv.QUEUED_P, 128
    tabs = [dev(c["table"]) for c in cases]
    la = Launch(tabs, [c["values"].reshape(B, P) for c in cases])
    q = _block()
    dst = torch.full((B, D * la.n), -3.0, device=DEV)
    et.check_errors()
    _lib.check(_lib.load().et_maplookup_prealloc_q(
        la.code, ctypes.addressof(la.descs), la.n, B, dst.data_ptr(), D * la.n, 0, q.data_ptr(),
        _lib.stream_handle()))
    torch.cuda.synchronize()
    assert _block_is_zero(q)
    ext = [sv.zero_row_inputs(c, P) for c in cases]
    want = oracle.maplookup_prealloc([t for t, _ in ext], [i for _, i in ext])
    assert sv.same_special(host(dst), want, "f32")
    assert et.check_errors() == sum(c["events"] for c in cases)


# --- sparse SGD on ragged bags: wide chains of every type, split mode, weights ------------------------

@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("static", [True, False])
@pytest.mark.parametrize("kind,dim", [("f32", 128), ("f64", 64), ("f16", 64), ("bf16", 64)])
def test_ragged_and_weighted_sgd(oracle, kind, dim, static, weighted):
    """The hot_case shape (a 3,000-entry chain of S = 16 entries whose last run is 12) in
    every element type, ragged and weighted; in Float32 also with exact=False, which a
    ragged update accepts and runs exactly."""
    case = sv.hot_sgd_case(kind, dim, weighted)
    lt = Static(dim) if static else Dynamic
    R = ragged(case["values"], case["colptr"])
    w = None if not weighted else dev(case["weights"])
    et.check_errors()
    for exact in ((None, False) if kind == "f32" and not weighted else (None,)):
        A = et.SimpleEmbedding(dev(case["table"], kind), lt)
        g = et.SparseEmbeddingUpdate(lt, dev(case["delta"], kind), R, w)
        kw = {} if exact is None else {"exact": exact}
        et.update_(et.Descent(0.1), A, g, **kw)
        ref = sv.hot_sgd_ref(oracle, case, fused_update_path(A))
        got = host(A.data)
        assert sv.same_special(got, ref, kind), (exact, np.argwhere(
            sv.bits_of(got, kind) != sv.bits_of(ref, kind))[:8].tolist())
    assert et.check_errors() == 0


def test_split_mode_sgd_fixed_pool(oracle):
    """exact=False on a fixed-pool index: columns of at most ET_SGD_CHUNK occurrences are
    pinned like the exact mode; the longer ones are ordered partial sums, so there the
    non-finite class of every element is pinned and the finite elements lie within the a
    priori bound of a Float32 sum of n terms in any order, then one fma: gamma(n + 2) *
    (|w| + eta * sum |delta|) around the Float64 update, n the column's occurrences.  (The
    1e-6 of tests/test_gpu_update.py does not carry over to this shape: the reference's own
    serial sum of the hottest column, 40,000 terms, lies at 3.5e-6 here.)"""
    case = sv.sgd_case()
    D, eta = sv.SGD_D, sv.SGD_ETA
    x, I = case["tables"][0], case["idx"][0]
    delta = np.ascontiguousarray(case["delta"][:, :D])
    A = et.SimpleEmbedding(dev(x), Static(D))
    et.check_errors()
    et.update_(et.Descent(eta), A, et.SparseEmbeddingUpdate(A.lookup_type, dev(delta), dev(I)),
               exact=False)
    got = host(A.data)
    ref = x.copy()
    oracle.sgd(ref, delta, I, eta, fused=True)
    counts = np.bincount(I.ravel(), minlength=x.shape[0] + 1)[1:]
    hot = counts > sv.CHUNK
    assert hot.sum() >= 10 and sv.same_special(got[~hot], ref[~hot], "f32")
    fin = np.isfinite(ref[hot])
    assert np.array_equal(np.isnan(got[hot]), np.isnan(ref[hot]))
    inf = np.isinf(ref[hot])
    assert np.array_equal(got[hot][inf], ref[hot][inf])
    with np.errstate(all="ignore"):
        acc = np.zeros(x.shape, np.float64)
        np.add.at(acc, I.ravel() - 1, np.repeat(delta.astype(np.float64), sv.SGD_P, axis=0))
        mag = np.zeros(x.shape, np.float64)
        np.add.at(mag, I.ravel() - 1, np.repeat(np.abs(delta).astype(np.float64), sv.SGD_P, axis=0))
        err = np.abs(got.astype(np.float64) - (x.astype(np.float64) - eta * acc))[hot][fin]
        scale = (np.abs(x.astype(np.float64)) + eta * mag)[hot][fin]
        bound = (wr.gamma(counts + 2.0, 2.0 ** -24)[:, None] * np.ones(D))[hot][fin]
    assert (err <= bound * scale).all()
    assert et.check_errors() == 0


# --- AdaGrad ---------------------------------------------------------------------------------------------

def _ada_update(case, rowwise):
    import test_gpu_adagrad as ta

    kind = ta.KINDS[case["name"]]
    A = et.SimpleEmbedding(kind.dev(case["table"]))
    opt = et.AdaGrad(ta.ETA, ta.EPS, rowwise=rowwise)
    opt.state(A).copy_(dev(case["state"]))
    idx = (dev(case["index"][0]) if len(case["index"]) == 1 else
           et.RaggedIndices(dev(case["index"][0]), dev(case["index"][1])))
    et.update_(opt, A, et.SparseEmbeddingUpdate(A.lookup_type, kind.dev(case["delta"]), idx))
    return host(A.data), host(opt.state(A))


@pytest.mark.parametrize("ragged_idx", [False, True])
@pytest.mark.parametrize("name,dim", [("f32", 128), ("f32", 7), ("bf16", 128), ("bf16", 7)])
def test_adagrad_elementwise(name, dim, ragged_idx):
    import test_gpu_adagrad as ta

    case = sv.adagrad_case(name, dim, ragged_idx)
    et.check_errors()
    got_t, got_s = _ada_update(case, False)
    table, state = case["table"].copy(), case["state"].copy()
    with np.errstate(all="ignore"):
        ta.ref_step(ta.KINDS[name], table, state, case["delta"], case["lists"])
    assert sv.same_special(got_t, table, name)
    assert sv.same_special(got_s, state, "f32")
    assert et.check_errors() == 0


@pytest.mark.parametrize("ragged_idx", [False, True])
@pytest.mark.parametrize("name,dim", [("f32", 128), ("f32", 7), ("bf16", 128), ("bf16", 7)])
def test_adagrad_rowwise(name, dim, ragged_idx):
    """Columns that are finite in the reference keep the derived bounds of
    tests/test_gpu_adagrad.py; in the others every element has the reference's class (NaN,
    +Inf, -Inf or finite; a finite element there is an unchanged one, compared bit for bit).
    The clean columns are bit-identical to a run whose planted columns and bags hold
    ordinary values: nothing leaks from a planted column."""
    import test_gpu_adagrad as ta

    kind = ta.KINDS[name]
    case = sv.adagrad_case(name, dim, ragged_idx, rowwise=True)
    et.check_errors()
    got_t, got_s = _ada_update(case, True)
    with np.errstate(all="ignore"):
        ref_t, ref_s = ta.rowwise_in_C(kind, case["table"], case["state"], case["delta"],
                                       case["lists"], "sequential")
    bad = ~(np.isfinite(ref_s) & np.isfinite(kind.toC(ref_t)).all(1))
    bad[[0, 1, 14]] = True  # zero and subnormal gradients: the bounds are relative to s > 0
    assert 3 < bad.sum() <= 8 and set(np.nonzero(bad)[0]) <= set(case["planted"])
    fin = {c: b for c, b in case["lists"].items() if not bad[c]}
    t0, s0 = case["table"].copy(), case["state"].copy()
    gt, gs = got_t.copy(), got_s.copy()
    for c in np.nonzero(bad)[0]:  # judged below, not by the bounds
        gt[c], gs[c] = t0[c], s0[c]
    rs, rw = ta.rowwise_bounds(kind, t0, s0, case["delta"], fin, gt, gs)
    print(f"rowwise special ratio {name} dim {dim}: state {rs:.3f} table {rw:.3f}")
    assert rs <= 1.0 and rw <= 1.0, (rs, rw)
    for c in np.nonzero(bad)[0]:
        g, r = kind.toC(got_t[c]), kind.toC(ref_t[c])
        assert np.array_equal(np.isnan(g), np.isnan(r)), c
        assert np.array_equal(np.isinf(g), np.isinf(r)) and np.array_equal(
            np.signbit(g)[np.isinf(r)], np.signbit(r)[np.isinf(r)]), c
        assert np.isnan(got_s[c]) == np.isnan(ref_s[c]) and np.isinf(got_s[c]) == np.isinf(ref_s[c])
    for c in (0, 3, 14):  # steps of 0 / eps, g / Inf and 0: the row keeps every bit
        assert got_t[c].tobytes() == case["table"][c].tobytes(), c
    # isolation: the same call with ordinary values in the planted columns and bags
    plain = sv.adagrad_case(name, dim, ragged_idx, rowwise=True, plain=True)
    changed = (sv.bits_of(case["delta"], name) != sv.bits_of(plain["delta"], name)).any(1)
    assert 0 < changed.sum() <= 8
    pt, ps = _ada_update(plain, True)
    clean = np.setdiff1d(np.arange(ta.R), case["planted"])
    assert got_t[clean].tobytes() == pt[clean].tobytes()
    assert got_s[clean].tobytes() == ps[clean].tobytes()
    assert et.check_errors() == 0


# --- weight gradient ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,kind", [(16, "f32"), (128, "f32"), (7, "f32"), (16, "f16"),
                                      (128, "bf16"), (128, "f64")])
def test_weight_gradient(dim, kind):
    """An entry whose bag gradient and table row are finite keeps the gamma(D + 1) bound; an
    entry that meets a NaN is NaN.  Inf is left out: a Float32 dot product can overflow where
    the Float64 reference does not, so an entry that meets Inf has no single right answer."""
    from embtab.weighted import weight_grad

    table, delta, values, colptr, bf16, meets = sv.wgrad_case(dim, kind)
    A = et.SimpleEmbedding(dev(table, kind))
    et.check_errors()
    dw = host(weight_grad(A, dev(delta, kind), ragged(values, colptr)))
    ref, mag = wr.weight_grad_f64(table, delta, values, colptr, bf16)
    assert np.isnan(dw[meets]).all() and np.isfinite(dw[~meets]).all()
    u = 2.0 ** -53 if kind == "f64" else 2.0 ** -24
    err = np.abs(dw[~meets].astype(ref.dtype) - ref[~meets])
    assert (err <= wr.gamma(dim + 1, u) * mag[~meets]).all()
    assert et.check_errors() == 0


# --- quantised lookup -------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,dim,split", sv.QUANT_CASES)
def test_quantised_lookup(bits, dim, split):
    """Packed tables built directly (not by the quantiser) with palette header halves: INT8
    x 128 fused, INT4 x 32 with a split header, INT8 x 20 generic, into f32, f16 and bf16.
    Row 1 has a NaN header, so an out-of-range index must still add +0; 65504-scale rows
    overflow only at the final rounding to f16."""
    et.check_errors()
    for P in (1, 8):
        case = sv.quant_case(bits, dim, P)
        ld = et.quant.default_ld_bytes(dim, bits, split)
        packed, hdr = sv.quant_pack(case, ld, split)
        Q = et.QuantizedEmbedding(dev(packed), dim, bits, dev(hdr) if split else None)
        I = dev(case["values"].reshape(sv.FWD_B, P))
        for out, dt in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
            got = et.lookup_(torch.empty((sv.FWD_B, dim), dtype=dt, device=DEV), Q, I)
            want, ev = sv.quant_ref(case, out)
            assert sv.same_special(host(got), want, out), (P, out)
            assert et.check_errors() == ev == case["events"]
