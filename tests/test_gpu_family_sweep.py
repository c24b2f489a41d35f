"""Seeded random sweeps of the five newer kernel families (ragged bags, weighted and
mean-pooled bags, sparse AdaGrad, weighted AdaGrad, quantised tables), modelled on
tests/test_gpu_update_sweep.py: tests/sweep_cases.py draws every case from
``np.random.default_rng(seed)`` (family or optimiser, element type, storage, rows, dim, batch,
length law, capacity tail, Zipf or uniform indices), every seed is an independent case, and
the assertion messages carry the drawn parameters.  tests/test_family_sweep_host.py asserts
without a GPU that the seeds reach every family, element type, storage kind, batch and law.

Expected values are the ones each family's own file uses: ``expect_lookup`` over the C oracle
(ragged), ``weighted_ref.forward`` / ``weight_grad_f64`` (weighted, mean), ``quant_ref.pooled``
(quantised, up to B = 1,027; beyond it the C oracle's pooled sum of the dequantised table,
an equality tests/test_gpu_quant.py pins), the C oracle's ``sgd`` on the expanded gradient
and ``weighted_ref.sgd`` (Descent), tests/test_gpu_adagrad.py's ``ref_step`` and
``weighted_adagrad_ref`` (AdaGrad).  Comparisons are byte equality, except where the
family's file has a derived bound: the row-wise AdaGrad and the weight gradient.

A case holds at most 60,000 entries, so the per-entry Python references stay cheap.
Out-of-range indices stay with the targeted files: every case ends with no error counted."""
import numpy as np
import pytest
import torch

import embtab as et
import quant_ref as qr
import sweep_cases as sc
import test_gpu_adagrad as ta
import weighted_adagrad_ref as war
import weighted_ref as wr
from embtab.tables import Dynamic, Static, fused_update_path
from embtab.weighted import weight_grad
from test_gpu_ragged import dev, expect_lookup, host, ranges_of, same
from test_gpu_update_sweep import _ColPtr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ETA, EPS = ta.ETA, ta.EPS
OUT_TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def make_table(kind, arr, storage, page, static, seed):
    t = kind.dev(arr)
    if storage == "simple":
        return et.SimpleEmbedding(t, Static(arr.shape[1]) if static else Dynamic)
    if storage == "paged":
        return et.SplitEmbedding(t, page)
    return _ColPtr(t, np.random.default_rng(seed))


def dense(A):
    if isinstance(A, _ColPtr):
        return host(A.dense())
    return host(A.to_dense() if isinstance(A, et.SplitEmbedding) else A.data)


def destination(B, D, tdtype, strided):
    """(dst, wide): a plain (B, D) tensor, or columns 4..4+D of a wider one filled with 0xA5."""
    if not strided:
        return torch.empty((B, D), dtype=tdtype, device=DEV), None
    wide = torch.empty((B, D + 8), dtype=tdtype, device=DEV)
    wide.view(torch.uint8).fill_(0xA5)
    return wide[:, 4:4 + D], wide


def indices_of(c):
    return et.RaggedIndices(dev(c["values"]), dev(c["colptr"]))


# --- forward --------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", sc.FORWARD_SEEDS)
def test_random_forward(oracle, seed):
    c = sc.forward_case(seed)
    msg = c["params"]
    family, kname, B, D = c["family"], c["kind"], c["B"], c["D"]
    values, colptr, table = c["values"], c["colptr"], c["table"]
    nnz = len(values)
    I = indices_of(c)
    if family in ("int8", "int4"):
        A = et.QuantizedEmbedding(dev(c["rows"]), D, c["bits"],
                                  dev(c["hdr"]) if c["split"] else None)
        assert A.ld_bytes == c["ld_bytes"]
        dst, wide = destination(B, D, OUT_TORCH[kname], c["strided"])
        et.lookup_(dst, A, I)
        if B <= sc.QUANT_REF_MAX_B:
            rg = ranges_of(colptr, nnz)
            want, oob = qr.pooled(table, [values[lo:hi] for lo, hi in rg], kname)
            assert oob == 0
        else:
            want = qr.store(expect_lookup(oracle, table, values, ranges_of(colptr, nnz)), kname)
    else:
        kind = sc.kind_of(kname)
        bf16 = kname == "bf16"
        A = make_table(kind, table, c["storage"], c["page"], False, seed)
        dst, wide = destination(B, D, kind.torch, c["strided"])
        if family == "ragged":
            kw = {"bf16": True} if bf16 else {"f16_fp32_acc": True} if kname == "f16acc" else {}
            if kname == "f16acc":
                et.maplookup_(et.PreallocationStrategy(0), dst, [A], [I], f16_fp32_acc=True)
            else:
                et.lookup_(dst, A, I)
            want = expect_lookup(oracle, table, values, ranges_of(colptr, nnz), **kw)
        else:
            w = c.get("weights")
            W = et.WeightedIndices(I, None if w is None else dev(w),
                                   mode="mean" if family == "wmean" else "sum")
            et.lookup_(dst, A, W)
            want, events = wr.forward(table, values, colptr, w,
                                      mode="mean" if family == "wmean" else "sum", bf16=bf16)
            assert events == 0
            if c.get("weight_grad"):
                dw = host(weight_grad(A, kind.dev(c["delta"]), I))
                ref, mag = wr.weight_grad_f64(table, c["delta"], values, colptr, bf16)
                u = 2.0 ** -53 if kname == "f64" else 2.0 ** -24
                err = np.abs(dw.astype(ref.dtype) - ref)
                assert (err <= wr.gamma(D + 1, u) * mag).all(), msg
                assert same(dw[c["used"]:], np.zeros(c["tail"], dw.dtype)), msg
    assert same(host(dst), want), msg
    if wide is not None:
        assert ta.padding_intact(wide, D), msg
    assert et.check_errors() == 0, msg


# --- update ---------------------------------------------------------------------------------------

def fixed_colptr(B, P):
    return 1 + P * np.arange(B + 1, dtype=np.int64)


def sgd_reference(oracle, kname, table, delta, c, fused):
    """The Descent reference of one table, in place on `table`: the C oracle on the expanded
    gradient (``delta[bag]``; ``w_k * delta[bag(k)]`` for Float32 / Float64 weighted
    gradients), ``weighted_ref.sgd`` for 16-bit weighted gradients."""
    bf16 = kname == "bf16"
    used, values = c["used"], c["values"]
    if used == 0:
        return
    if "weights" not in c:
        oracle.sgd(table, delta[c["bag"]], values[:used], 0.1, fused=fused, bf16=bf16)
    elif kname in ("f32", "f64"):
        E, cov = wr.expanded_gradient(delta, c["weights"], c["colptr"], len(values))
        assert cov.sum() == used
        oracle.sgd(table, E[cov], values[cov], 0.1, fused=fused)
    else:
        wr.sgd(table, delta, values, c["colptr"], c["weights"], 0.1, fused=fused, bf16=bf16)


def adagrad_reference(kind, c, delta):
    """(lists, g_of) for ta.ref_step / the row-wise bounds of one table's gradient."""
    R = c["table"].shape[0]
    fixed = c.get("fixed") or c.get("form") == "fixed"
    if "weights" in c:
        colptr = fixed_colptr(len(c["L"]), int(c["L"][0])) if fixed else c["colptr"]
        return war.reference_inputs(kind, delta, c["values"], colptr, c["weights"], nrows=R)
    if fixed:
        return ta.lists_fixed(c["values"].reshape(len(c["L"]), -1), nrows=R), None
    return ta.lists_ragged(c["values"], c["colptr"], nrows=R), None


def gradient(kind, A, c, ddev):
    """The SparseEmbeddingUpdate of one table's case over the device gradient `ddev`."""
    fixed = c.get("fixed") or c.get("form") == "fixed"
    I = dev(c["values"].reshape(len(c["L"]), -1)) if fixed else indices_of(c)
    w = dev(c["weights"]) if "weights" in c else None
    return et.SparseEmbeddingUpdate(A.lookup_type, ddev, I, w)


@pytest.mark.parametrize("seed", sc.UPDATE_SEEDS)
def test_random_update(oracle, seed):
    c = sc.update_case(seed)
    msg = c["params"]
    kname = c["kind"]
    kind = sc.kind_of(kname)
    A = make_table(kind, c["table"], c["storage"], c["page"], c["static"], seed)
    table = c["table"].copy()
    if not c["adagrad"]:
        delta = c["deltas"][0]
        et.update_(et.Descent(0.1), A, gradient(kind, A, c, kind.dev(delta)))
        sgd_reference(oracle, kname, table, delta, c, fused_update_path(A))
        assert same(dense(A), table), msg
        assert et.check_errors() == 0, msg
        return
    opt = et.AdaGrad(ETA, EPS, rowwise=c["rowwise"], weighted=c["weighted"])
    S = opt.state(A)
    S.copy_(dev(c["state"]))
    state = c["state"].copy()
    for step, delta in enumerate(c["deltas"]):  # fresh gradients; the state is carried
        et.update_(opt, A, gradient(kind, A, c, kind.dev(delta)), nontemporal=step == 0)
        lists, g_of = adagrad_reference(kind, c, delta)
        got_t, got_s = dense(A), host(S)
        if c["rowwise"]:
            if g_of is None:
                rs, rw = ta.rowwise_bounds(kind, table, state, delta, lists, got_t, got_s)
            else:
                rs, rw = war.rowwise_bounds(kind, table, state, g_of, got_t, got_s)
            assert rs <= 1.0 and rw <= 1.0, (step, rs, rw, msg)
            table, state = got_t, got_s  # each step is judged alone, from what the GPU wrote
        else:
            with np.errstate(all="ignore"):
                ta.ref_step(kind, table, state, delta, lists, g_of=g_of)
            assert same(got_t, table) and same(got_s, state), (step, msg)
    assert et.check_errors() == 0, msg


# --- multi-table ----------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", sc.MULTI_SEEDS)
def test_random_multi_table_update(oracle, seed):
    """Two to five tables in one ``update_`` call, their gradients column blocks of one
    Preallocation-strided gradient with k prepended columns: Descent, then
    AdaGrad(weighted=True) on fresh copies, every table bit-identical to its own single-table
    reference.  16-bit tables under a weighted gradient are Static: the fused path is the one
    ``weighted_ref.sgd`` is pinned for."""
    c = sc.multi_case(seed)
    msg = c["params"]
    kname = c["kind"]
    kind = sc.kind_of(kname)
    bf16 = kname == "bf16"
    ddev = kind.dev(c["delta"])
    offs = c["offs"]
    blocks = [np.ascontiguousarray(c["delta"][:, offs[t]:offs[t + 1]])
              for t in range(c["n"])]

    def build():
        As = []
        for t, tab in enumerate(c["tables"]):
            pinned = "weights" in tab and kname in ("f16", "bf16")
            static = tab["static"] or pinned
            As.append(et.SimpleEmbedding(kind.dev(tab["table"]),
                                         Static(tab["D"]) if static else Dynamic))
            assert not pinned or fused_update_path(As[-1])
        grads = [gradient(kind, A, tab, ddev[:, offs[t]:offs[t + 1]])
                 for t, (A, tab) in enumerate(zip(As, c["tables"]))]
        assert grads[0].delta.stride(0) == c["delta"].shape[1]
        return As, grads

    # Descent: the oracle's multi-table model over the expanded gradients
    As, grads = build()
    et.update_(et.Descent(0.1), As, grads)
    refs = [tab["table"].copy() for tab in c["tables"]]
    ts, exp_d, exp_i = [], [], []
    for t, tab in enumerate(c["tables"]):
        used, values = tab["used"], tab["values"]
        if "weights" in tab and kname in ("f16", "bf16"):
            wr.sgd(refs[t], blocks[t], values, tab["colptr"], tab["weights"], 0.1, fused=True,
                   bf16=bf16)
            continue
        if "weights" in tab:
            E, cov = wr.expanded_gradient(blocks[t], tab["weights"], tab["colptr"], len(values))
            d, i = E[cov], values[cov]
        elif tab["form"] == "fixed":
            d, i = blocks[t], values.reshape(c["B"], -1)
        else:
            d, i = blocks[t][tab["bag"]], values[:used]
        ts.append(t)
        exp_d.append(d)
        exp_i.append(i)
    if ts:
        oracle.sgd_multi([refs[t] for t in ts], exp_d, exp_i, 0.1,
                         [fused_update_path(As[t]) for t in ts], bf16=bf16)
    for t, A in enumerate(As):
        assert same(host(A.data), refs[t]), ("Descent", t, msg)

    # AdaGrad(weighted=True), element-wise, on fresh copies
    As, grads = build()
    opt = et.AdaGrad(ETA, EPS, initial_accumulator_value=0.1, weighted=True)
    et.update_(opt, As, grads)
    for t, (A, tab) in enumerate(zip(As, c["tables"])):
        table = tab["table"].copy()
        state = np.full(table.shape, 0.1, kind.C)
        lists, g_of = adagrad_reference(kind, tab, blocks[t])
        with np.errstate(all="ignore"):
            ta.ref_step(kind, table, state, blocks[t], lists, g_of=g_of)
        assert same(host(A.data), table), ("AdaGrad table", t, msg)
        assert same(host(opt.state(A)), state), ("AdaGrad state", t, msg)
    assert et.check_errors() == 0, msg
