"""Weighted and mean-pooled bags, the parts that need no GPU: symbols and struct layouts
against the header, every argument error of the et_weighted_* entry points (status codes
before any device work, dummy pointers never dereferenced), the workspace size, the
validation of WeightedIndices on CPU tensors, and the numpy reference itself
(tests/weighted_ref.py) against the existing oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import weighted_ref as wr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --- ABI ------------------------------------------------------------------------------------

def test_symbols_and_constants():
    from embtab import _lib

    L = _lib.load()
    for name in ("et_weighted_maplookup_prealloc", "et_weighted_weight_grad",
                 "et_weighted_sgd_workspace_size", "et_weighted_sgd"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    hdr = open(os.path.join(REPO, "include", "embtab.h")).read()
    assert "#define ET_POOL_SUM 0" in hdr and "#define ET_POOL_MEAN 1" in hdr
    assert (_lib.ET_POOL_SUM, _lib.ET_POOL_MEAN) == (0, 1)
    assert "#define ET_ABI_VERSION 9" in hdr and L.et_abi_version() == 9


def test_weighted_struct_layouts_match_header(tmp_path):
    from embtab import _lib

    structs = (("et_weighted_desc", _lib.WeightedDesc),
               ("et_weighted_update_desc", _lib.WeightedUpdateDesc))
    lines = []
    for cname, S in structs:
        fields = [f[0] for f in S._fields_]
        fmt = " ".join(["%zu"] * (len(fields) + 1))
        args = ", ".join([f"sizeof({cname})"] + [f"offsetof({cname}, {f})" for f in fields])
        lines.append(f'  printf("{fmt}\\n", {args});')
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "embtab.h"\n'
                    "int main(void) {\n" + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    for (cname, S), line in zip(structs, out.strip().split("\n")):
        want = [ctypes.sizeof(S)] + [getattr(S, f[0]).offset for f in S._fields_]
        assert list(map(int, line.split())) == want, cname
    # the new structs are the ragged ones with the stated changes
    rf = [f[0] for f in _lib.RaggedDesc._fields_]
    wf = [f[0] for f in _lib.WeightedDesc._fields_]
    assert wf == [("mode" if f == "reserved" else f) for f in rf] + ["weights"]
    assert [f[0] for f in _lib.WeightedUpdateDesc._fields_] == \
        [f[0] for f in _lib.RaggedUpdateDesc._fields_] + ["weights", "dweights"]


def _desc(L, **kw):
    d = dict(table=1 << 20, ld_table=16, nrows=100, dim=16, mode=0, idx=1 << 21, nnz=64,
             colptr=1 << 22, dst_row_off=0, cols_per_page=0, weights=1 << 25)
    d.update(kw)
    arr = (L.WeightedDesc * 1)()
    arr[0] = L.WeightedDesc(*[d[f[0]] for f in L.WeightedDesc._fields_])
    return arr


def _udesc(L, **kw):
    d = dict(table=1 << 20, ld_table=16, nrows=100, dim=16, reserved=0, delta=1 << 23,
             ld_delta=16, idx=1 << 21, nnz=64, colptr=1 << 22, batch=8, cols_per_page=0,
             weights=1 << 25, dweights=1 << 26)
    d.update(kw)
    arr = (L.WeightedUpdateDesc * 1)()
    arr[0] = L.WeightedUpdateDesc(*[d[f[0]] for f in L.WeightedUpdateDesc._fields_])
    return arr


def test_lookup_argument_errors_need_no_gpu():
    from embtab import _lib

    L = _lib.load()
    f = L.et_weighted_maplookup_prealloc
    dst = 1 << 24  # never dereferenced: every call below stops at the host checks
    a = ctypes.addressof
    assert f(_lib.ET_F32, a(_desc(_lib, dst_row_off=4)), 1, 8, dst, 16, 0, None) == -1
    assert b"ld_dst" in L.et_last_error()
    # unknown, integer dtypes
    for dt in (99, _lib.ET_I32, _lib.ET_I64):
        assert f(dt, a(_desc(_lib)), 1, 8, dst, 16, 0, None) == -4
    # weights with mean mode; a mode that is neither
    assert f(_lib.ET_F32, a(_desc(_lib, mode=1)), 1, 8, dst, 16, 0, None) == -4
    assert b"mean" in L.et_last_error()
    assert f(_lib.ET_F32, a(_desc(_lib, mode=2, weights=0)), 1, 8, dst, 16, 0, None) == -1
    # flags: ET_FLAG_NONTEMPORAL only
    assert f(_lib.ET_F16, a(_desc(_lib)), 1, 8, dst, 16, _lib.ET_FLAG_F16_FP32_ACC, None) == -4
    # negative sizes, leading dimension below dim
    assert f(_lib.ET_F32, a(_desc(_lib)), 1, -1, dst, 16, 0, None) == -1
    assert f(_lib.ET_F32, a(_desc(_lib)), -1, 8, dst, 16, 0, None) == -1
    assert f(_lib.ET_F32, a(_desc(_lib, nnz=-1)), 1, 8, dst, 16, 0, None) == -1
    assert f(_lib.ET_F32, a(_desc(_lib, dim=-2)), 1, 8, dst, 16, 0, None) == -1
    assert f(_lib.ET_F32, a(_desc(_lib, ld_table=8)), 1, 8, dst, 16, 0, None) == -1
    # NULL with non-empty work
    assert f(_lib.ET_F32, None, 1, 8, dst, 16, 0, None) == -1
    assert f(_lib.ET_F32, a(_desc(_lib)), 1, 8, None, 16, 0, None) == -1
    assert f(_lib.ET_F32, a(_desc(_lib, idx=0)), 1, 8, dst, 16, 0, None) == -1
    assert f(_lib.ET_F32, a(_desc(_lib, colptr=0)), 1, 8, dst, 16, 0, None) == -1
    assert f(_lib.ET_F32, a(_desc(_lib, table=0)), 1, 8, dst, 16, 0, None) == -1
    # misaligned weights
    assert f(_lib.ET_F64, a(_desc(_lib, weights=(1 << 25) + 4)), 1, 8, dst, 16, 0, None) == -1
    big = (_lib.WeightedDesc * 33)()
    assert f(_lib.ET_F32, a(big), 33, 8, dst, 16, 0, None) == -1
    # batch == 0 (and no table) is a no-op success
    assert f(_lib.ET_F32, a(_desc(_lib)), 1, 0, None, 16, 0, None) == 0
    assert f(_lib.ET_F32, None, 0, 8, None, 16, 0, None) == 0


def test_weight_grad_argument_errors_need_no_gpu():
    from embtab import _lib

    L = _lib.load()
    f = L.et_weighted_weight_grad
    a = ctypes.addressof
    for dt in (99, _lib.ET_I32, _lib.ET_I64):
        assert f(dt, a(_udesc(_lib)), 1, None) == -4
    assert f(_lib.ET_F32, None, 1, None) == -1
    assert f(_lib.ET_F32, a(_udesc(_lib)), -1, None) == -1
    for bad in (dict(nnz=-1), dict(batch=-1), dict(dim=-1), dict(ld_delta=8), dict(ld_table=8),
                dict(dweights=0), dict(delta=0), dict(colptr=0), dict(idx=0), dict(table=0)):
        assert f(_lib.ET_F32, a(_udesc(_lib, **bad)), 1, None) == -1, bad
    big = (_lib.WeightedUpdateDesc * 33)()
    assert f(_lib.ET_F32, a(big), 33, None) == -1
    # nothing to write: no entries, no tables; weights are ignored (NULL is fine: checked
    # by the call above reaching the dweights check with weights set, and here without)
    assert f(_lib.ET_F32, a(_udesc(_lib, nnz=0, weights=0)), 1, None) == 0
    assert f(_lib.ET_F32, None, 0, None) == 0


def test_sgd_argument_errors_need_no_gpu():
    from embtab import _lib

    L = _lib.load()
    f = L.et_weighted_sgd
    a = ctypes.addressof
    assert f(_lib.ET_I32, a(_udesc(_lib)), 1, 0.1, 0, None, 0, None) == -4
    assert f(99, a(_udesc(_lib)), 1, 0.1, 0, None, 0, None) == -4
    for flag in (_lib.ET_FLAG_SGD_INDEX_ONLY, _lib.ET_FLAG_SGD_APPLY_ONLY,
                 _lib.ET_FLAG_SGD_HOT_PASS):
        assert f(_lib.ET_F32, a(_udesc(_lib)), 1, 0.1, flag, None, 0, None) == -4
    for bad in (dict(nnz=-1), dict(batch=-1), dict(ld_delta=8), dict(ld_table=8), dict(delta=0),
                dict(colptr=0), dict(weights=0)):
        assert f(_lib.ET_F32, a(_udesc(_lib, **bad)), 1, 0.1, 0, None, 0, None) == -1, bad
    assert f(_lib.ET_F32, None, 1, 0.1, 0, None, 0, None) == -1
    big = (_lib.WeightedUpdateDesc * 33)()
    assert f(_lib.ET_F32, a(big), 33, 0.1, 0, None, 0, None) == -1
    # valid descriptors stop at the missing workspace, before any device work; the exact
    # flags and the implied Float16 accumulation flag are accepted
    for fl in (0, _lib.ET_FLAG_EXACT_UPDATE, _lib.ET_FLAG_EXACT_IF_FAST,
               _lib.ET_FLAG_F16_FP32_ACC, _lib.ET_FLAG_SGD_UNFUSED):
        assert f(_lib.ET_F16, a(_udesc(_lib)), 1, 0.1, fl, None, 0, None) == -3
    # nothing to do: dweights is ignored
    assert f(_lib.ET_F32, a(_udesc(_lib, batch=0)), 1, 0.1, 0, None, 0, None) == 0
    assert f(_lib.ET_F32, a(_udesc(_lib, nnz=0, dweights=0)), 1, 0.1, 0, None, 0, None) == 0
    assert f(_lib.ET_F32, None, 0, 0.1, 0, None, 0, None) == 0


def test_workspace_size_equals_the_ragged_one():
    from embtab import _lib

    L = _lib.load()
    for nnz, batch, dim in ((0, 8, 16), (1000, 8, 16), (100000, 4096, 128), (10000000, 1, 7)):
        w = _udesc(_lib, nnz=nnz, batch=batch, dim=dim, ld_table=dim, ld_delta=dim)
        r = (_lib.RaggedUpdateDesc * 1)()
        r[0] = _lib.RaggedUpdateDesc(*[getattr(w[0], f[0])
                                       for f in _lib.RaggedUpdateDesc._fields_])
        a, b = ctypes.c_int64(-1), ctypes.c_int64(-2)
        assert L.et_weighted_sgd_workspace_size(ctypes.addressof(w), 1, ctypes.byref(a)) == 0
        assert L.et_ragged_sgd_workspace_size(ctypes.addressof(r), 1, ctypes.byref(b)) == 0
        assert a.value == b.value > 0
    nb = ctypes.c_int64(0)
    big = (_lib.WeightedUpdateDesc * 33)()
    assert L.et_weighted_sgd_workspace_size(ctypes.addressof(big), 33, ctypes.byref(nb)) == -1
    assert L.et_weighted_sgd_workspace_size(ctypes.addressof(_udesc(_lib)), 1, None) == -1
    assert L.et_weighted_sgd_workspace_size(ctypes.addressof(_udesc(_lib, nnz=1 << 31)), 1,
                                            ctypes.byref(nb)) == -1


# --- WeightedIndices --------------------------------------------------------------------------

def test_weighted_indices_validation():
    import embtab as et

    I = torch.arange(1, 13, dtype=torch.int64).reshape(3, 4)
    w = torch.ones(3, 4)
    W = et.WeightedIndices(I, w)
    assert W.batch == 3 and W.nnz == 12 and W.mode == "sum" and not W.weight_grad
    assert W.ragged.colptr.tolist() == [1, 5, 9, 13] and W.ragged.values.data_ptr() == I.data_ptr()
    assert et.WeightedIndices(I, w.reshape(-1), weight_grad=True).weight_grad
    assert et.WeightedIndices(I, mode="mean").weights is None
    assert et.WeightedIndices(I).mode == "sum"
    R = et.RaggedIndices.from_lengths(torch.arange(1, 8, dtype=torch.int64), [3, 0, 2])
    assert et.WeightedIndices(R, torch.ones(7, dtype=torch.float64)).ragged is R
    for bad in (lambda: et.WeightedIndices(I, w, mode="mean"),        # mean takes no weights
                lambda: et.WeightedIndices(I, w, mode="max"),
                lambda: et.WeightedIndices(I, weight_grad=True),      # nothing to differentiate
                lambda: et.WeightedIndices(I, torch.ones(3, 5)),      # shape
                lambda: et.WeightedIndices(R, torch.ones(5)),         # the capacity, not the use
                lambda: et.WeightedIndices(R, torch.ones(1, 7)),
                lambda: et.WeightedIndices(I, torch.ones(3, 8)[:, ::2]),  # strided
                lambda: et.WeightedIndices(I, w.to(torch.float16)),
                lambda: et.WeightedIndices(I, w.to("meta")),          # device mix
                lambda: et.WeightedIndices(I[:, ::2], torch.ones(3, 2)),  # strided indices
                lambda: et.WeightedIndices(I.reshape(-1), torch.ones(12))):  # a vector index
        with pytest.raises(et.ArgumentError):
            bad()
    with pytest.raises(TypeError):
        et.WeightedIndices(I.to(torch.int32), w)
    with pytest.raises(TypeError):
        et.WeightedIndices(I, w.tolist())
    # the weights' type is checked against the table at the call
    A32 = et.SimpleEmbedding(torch.zeros(20, 16))
    A64 = et.SimpleEmbedding(torch.zeros(20, 16, dtype=torch.float64))
    Aint = et.SimpleEmbedding(torch.zeros(20, 16, dtype=torch.int32))
    W.check_for(A32)
    et.WeightedIndices(I, w.double()).check_for(A64)
    for A, X in ((A64, W), (A32, et.WeightedIndices(I, w.double())), (Aint, W),
                 (Aint, et.WeightedIndices(I, mode="mean"))):
        with pytest.raises(et.ArgumentError):
            X.check_for(A)
    # lookups refuse host indices, as for plain tensors
    from embtab.lookup import _check_idx

    with pytest.raises(et.ArgumentError):
        _check_idx(W)
    # a gradient that carries weights is refused where weights would be ignored
    g = et.SparseEmbeddingUpdate(A32.lookup_type, torch.zeros(3, 16), I, torch.ones(12))
    assert g.weights is not None and g.ragged().batch == 3
    assert et.SparseEmbeddingUpdate(A32.lookup_type, torch.zeros(3, 16), I).weights is None
    with pytest.raises(et.ArgumentError):
        et.update_(et.AdaGrad(0.1), A32, g)
    with pytest.raises(et.ArgumentError):
        et.PhasedUpdate([A32], [g])
    with pytest.raises(et.ArgumentError):
        et.update_(et.Descent(0.1), A32, g, exact=False)
    with pytest.raises(et.ArgumentError):
        et.update_(et.Descent(0.1), [A32], [g], exact=False)


# --- the reference itself ------------------------------------------------------------------------

LENMIX = [0, 1, 2, 3, 4, 5, 7, 8, 9, 33]


def _case(seed, B=40, rows=50, dim=24):
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 6, B)
    L[1:1 + len(LENMIX)] = LENMIX
    L[0] = L[-1] = 0
    colptr = np.concatenate([[1], 1 + np.cumsum(L)]).astype(np.int64)
    values = rng.integers(1, rows + 1, int(L.sum())).astype(np.int64)
    return rng, L, colptr, values


@pytest.mark.parametrize("kind", ["f32", "f64", "f16", "bf16"])
def test_reference_with_unit_weights_is_the_pooled_sum(oracle, kind):
    from oracle import f32_to_bf16

    rng, L, colptr, values = _case(1)
    x = rng.standard_normal((50, 24))
    bf16 = kind == "bf16"
    table = f32_to_bf16(x.astype(np.float32)) if bf16 else x.astype(
        {"f32": np.float32, "f64": np.float64, "f16": np.float16}[kind])
    C = wr.acc_type(table, bf16)
    kw = {"bf16": True} if bf16 else ({"f16_fp32_acc": True} if kind == "f16" else {})
    want = np.zeros((len(L), 24), table.dtype)
    for n in np.unique(L):
        if n:
            sel = np.nonzero(L == n)[0]
            I = np.stack([values[colptr[j] - 1:colptr[j + 1] - 1] for j in sel])
            want[sel] = oracle.pooled_sum(table, I, **kw)
    for w in (None, np.ones(len(values), C)):
        got, ev = wr.forward(table, values, colptr, w, bf16=bf16)
        assert ev == 0 and got.tobytes() == want.tobytes()
    # mean: the sum divided once; length 3 is not exact
    got, _ = wr.forward(table, values, colptr, mode="mean", bf16=bf16)
    j = int(np.nonzero(L == 3)[0][0])
    s = wr.to_c(want[j], bf16) if kind in ("f32", "f64") else None
    if s is not None:
        assert got[j].tobytes() == (s / C(3)).astype(table.dtype).tobytes()
    assert not got[0].any() and not np.signbit(wr.to_c(got[0], bf16)).any()


def test_reference_signed_zeros_and_out_of_range():
    table = np.full((4, 3), -0.0, np.float32)
    table[1] = [1.0, -2.0, 0.5]
    values = np.array([1, 9, 2, 1, 0], np.int64)       # 9 and 0 are out of range
    colptr = np.array([1, 2, 4, 4, 5, 6], np.int64)
    w = np.array([1.0, -1.0, 2.0, -3.0, -1.0], np.float32)
    got, ev = wr.forward(table, values, colptr, w)
    assert ev == 2
    assert np.signbit(got[0]).all() and (got[0] == 0).all()      # 1.0 * -0.0 = -0.0
    assert got[1].tolist() == [2.0, -4.0, 1.0]                    # -1 * +0 = -0, then + 2x
    assert not np.signbit(got[2]).any()                           # empty: +0
    assert not np.signbit(got[3]).any() and (got[3] == 0).all()   # -3 * -0 = +0
    assert np.signbit(got[4]).all()                               # -1 * +0 = -0 (out of range)
    # colptr beyond the capacity is clamped and counted
    _, ev = wr.forward(table, values, np.array([0, 3, 9], np.int64), w)
    assert ev == 2 + 2  # two bounds moved, indices 9 and 0 seen


@pytest.mark.parametrize("fused", [True, False])
def test_reference_sgd_is_the_oracle_on_the_expanded_gradient(oracle, fused):
    rng, L, colptr, values = _case(2, rows=12)  # 12 rows: every column has several entries
    nnz = len(values) + 6                       # a capacity tail no bag covers
    values = np.concatenate([values, rng.integers(1, 13, 6)]).astype(np.int64)
    table = rng.standard_normal((12, 24)).astype(np.float32)
    delta = rng.standard_normal((len(L), 24)).astype(np.float32)
    w = rng.standard_normal(nnz).astype(np.float32)
    E, covered = wr.expanded_gradient(delta, w, colptr, nnz)
    assert covered.sum() == L.sum() and not covered[-6:].any()
    want = table.copy()
    oracle.sgd(want, E[covered], values[covered], 0.1, fused=fused)
    got = wr.sgd(table.copy(), delta, values, colptr, w, 0.1, fused=fused)
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() != table.tobytes()


def test_fma32_emulation_matches_exact_arithmetic():
    from fractions import Fraction

    rng = np.random.default_rng(3)
    a = rng.standard_normal(2000).astype(np.float32)
    b = rng.standard_normal(2000).astype(np.float32)
    c = (rng.standard_normal(2000) * 10.0 ** rng.integers(-8, 3, 2000)).astype(np.float32)
    # ties on purpose: c = -(a*b rounded) + half an ulp patterns come from cancelling sums
    c[:500] = -(a[:500] * b[:500])
    got = wr._fma32(a, b, c)
    for i in range(2000):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        # float(Fraction) rounds once to float64; a float32 from the exact value needs care:
        # compare through the two neighbouring float32 candidates instead
        lo = np.float32(float(exact))
        cands = {lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))}
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact),
                                         int(np.float32(v).view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i])


# --- the weight-gradient bound holds for any order of summation ------------------------------------

@pytest.mark.parametrize("dim,kind", [(16, "f32"), (128, "f32"), (1504, "f32"), (7, "f32"),
                                      (16, "f16"), (7, "f16"), (128, "bf16"), (7, "bf16")])
def test_weight_grad_bound_holds_for_cpu_summation_orders(dim, kind):
    """|dw - ref| <= gamma_{D+1} * sum_f |delta_f * x_f| (D products, D - 1 additions: any
    order of summation stays inside it; Higham, Accuracy and Stability, §3.1) — checked for
    sequential, reversed and pairwise Float32 sums of the inputs the GPU test uses."""
    table, delta, values, colptr, bf16 = wr.wgrad_case(dim, kind)
    ref, mag = wr.weight_grad_f64(table, delta, values, colptr, bf16)
    bound = wr.gamma(dim + 1, 2.0 ** -24) * mag
    t, d = wr.to_c(table, bf16), wr.to_c(delta, bf16)
    bag = np.repeat(np.arange(len(colptr) - 1), np.diff(colptr))
    P = d[bag] * t[values - 1]  # (entries, D) products, one Float32 rounding each
    assert P.dtype == np.float32 and (mag > 0).all()
    worst = 0.0
    for order in ("seq", "rev", "pair"):
        if order == "pair":
            Q = P
            while Q.shape[1] > 1:
                if Q.shape[1] % 2:
                    Q = np.concatenate([Q, np.zeros((len(Q), 1), np.float32)], axis=1)
                Q = Q[:, 0::2] + Q[:, 1::2]
            dw = Q[:, 0]
        else:
            dw = np.zeros(len(P), np.float32)
            for f in (range(dim) if order == "seq" else range(dim - 1, -1, -1)):
                dw = dw + P[:, f]
        assert dw.dtype == np.float32
        err = np.abs(dw.astype(np.float64) - ref)
        assert (err <= bound).all(), order
        worst = max(worst, float((err / bound).max()))
    print(f"dim {dim} {kind}: largest observed / bound over the CPU orders = {worst:.4f}")
    assert 0 < worst <= 1
