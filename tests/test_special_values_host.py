"""The cases of tests/test_gpu_special_values.py, vetted on the CPU: the same builders, the
reference alone.  Each case must be able to fail: its reference holds every class of special
value the family can produce, few enough NaNs that positions still matter, enough clean bags
or rows that isolation is observable, and ``same_special`` rejects every mutation a wrong
kernel would produce.  The references are also checked against each other on these inputs."""
import numpy as np
import pytest

import special_values as sv
import weighted_ref as wr

ALL = ("nan", "+inf", "-inf", "subnormal", "-0")


def vet(ref, kind, clean, need=ALL):
    """`clean`: mask of the reference's clean rows (bags of a lookup, touched rows of an
    update, among `of` rows)."""
    c = sv.census(ref, kind)
    for k in need:
        assert c[k] > 0, (k, c)
    assert 8 * c["nan"] <= ref.size, c
    assert 2 * clean.sum() >= len(clean), (int(clean.sum()), len(clean))
    clean_row = int(np.nonzero(clean)[0][len(np.nonzero(clean)[0]) // 2])
    assert not sv.nan_mask(ref[clean_row], kind).any()
    muts = sv.mutations(ref, kind, clean_row)
    want = {"flush subnormals", "inf to nan", "nan a clean row", "swap one inf's sign"}
    if "-0" in need:
        want.add("-0 to +0")
    assert want <= set(muts), set(muts)
    assert sv.same_special(ref, ref.copy(), kind)
    for name, m in muts.items():
        assert not sv.same_special(m, ref, kind), name
    return c


def test_palette_pairs_sum_as_named():
    for kind in ("f32", "f64", "f16", "bf16"):
        pal = sv.palette(kind)
        v = pal["values"]
        c = sv.census(np.array([v[n] for n in v]).reshape(1, -1), kind)
        assert c["nan"] == 1 and c["+inf"] == 1 and c["-inf"] == 1 and c["-0"] == 1
        assert c["subnormal"] == 4
        if kind == "bf16":
            continue  # no numpy arithmetic on bit patterns: the forward cases sum them
        with np.errstate(all="ignore"):
            for a, b, s in pal["pairs"]:
                got = np.array([v[a] + v[b]])
                assert sv.same_special(got, np.array([v[s]]), kind), (kind, a, b)
    f = sv.palette("f16")["values"]
    with np.errstate(all="ignore"):
        assert np.isinf(f["big"] + f["big"] + f["-big"])
        assert np.float16(np.float32(f["big"]) * 2 - np.float32(f["big"])) == f["big"]


def test_same_special_and_census():
    a = np.array([[0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, 1.0]], np.float32)
    assert sv.census(a, "f32") == {"nan": 1, "+inf": 1, "-inf": 1, "subnormal": 1, "-0": 1}
    b = a.copy()
    b.view(np.uint32)[0, 4] = 0xffc00123  # another NaN: sign and payload are not compared
    assert sv.same_special(b, a, "f32") and not sv.same_special(b, a, "f32", copy=True)
    assert not sv.same_special(a[:, :6], a, "f32")
    assert not sv.same_special(a.astype(np.float64), a, "f32")


@pytest.mark.parametrize("kind,dim", sv.FIXED_CASES)
def test_fixed_pool_cases(oracle, kind, dim):
    tk = sv.table_kind(kind)
    for P in sv.POOLS:
        case = sv.fixed_case(kind, dim, P)
        assert sv.is_clean(case) and case["events"] == (1 if P == 1 else 2)
        ref = sv.forward_ref(oracle, case["table"], case["values"], case["colptr"], kind)
        vet(ref, tk, ~case["planted"])
        rows = case["rows"]
        assert case["table"].shape[0] == rows["inf"] and rows["nan"] == 1
        assert sv.nan_mask(case["table"][0, :1], tk).all()
    if kind == "f16acc":
        # [big, big, -big]: Inf in Julia's Float16 adds, 40000 with one final rounding
        case = sv.fixed_case(kind, dim, 8)
        v, cp, r = case["values"], case["colptr"], case["rows"]
        j = [j for j in range(sv.FWD_B)
             if v[cp[j] - 1:cp[j] + 2].tolist() == [r["big"], r["big"], r["-big"]]]
        assert len(j) == 1
        acc = sv.forward_ref(oracle, case["table"], v, cp, "f16acc")[j[0], 0]
        jul = sv.forward_ref(oracle, case["table"], v, cp, "f16")[j[0], 0]
        assert np.isfinite(acc) and np.isinf(jul)


@pytest.mark.parametrize("kind", ["i32", "i64"])
def test_integer_sums_wrap_in_the_oracle(oracle, kind):
    table, I, want = sv.int_wrap_case(kind)
    info = np.iinfo(table.dtype)
    exact = table.astype(object)[I - 1].sum(1)
    assert ((exact > info.max) | (exact < info.min)).sum() > 16  # sums that wrapped
    assert oracle.pooled_sum(table, I).tobytes() == want.tobytes()


@pytest.mark.parametrize("dim", sv.RAGGED_DIMS)
def test_ragged_and_weighted_cases(oracle, dim):
    case = sv.ragged_case(dim)
    table, cp = case["table"], case["colptr"]
    assert sv.is_clean(case) and case["events"] == 3
    ref = sv.forward_ref(oracle, table, case["values"], cp, "f32")
    vet(ref, "f32", ~case["planted"])
    # the two references agree: unit weights, and no weights, are the ragged lookup
    for w in (None, np.ones(len(case["values"]), np.float32)):
        got, ev = wr.forward(table, case["values"], cp, w)
        assert ev == 3 and sv.same_special(got, ref, "f32")
    w, values, planted = sv.forward_weights(case, np.float32, 7)
    assert sv.is_clean(case, values, planted)
    assert sv.census(w.reshape(1, -1), "f32")["nan"] == 1   # the NaN weight and nothing else
    ref, ev = wr.forward(table, values, cp, w)
    assert ev == 3
    vet(ref, "f32", ~planted)
    j = int(np.nonzero(w.view(np.uint32) == 0)[0][0])       # 0 * Inf is NaN
    assert values[j] == case["rows"]["inf"]
    assert np.isnan(ref[np.searchsorted(cp, j + 1, side="right") - 1, 0])
    values, planted = sv.mean_values(case)
    assert sv.is_clean(case, values, planted)
    ref, _ = wr.forward(table, values, cp, mode="mean")
    vet(ref, "f32", ~planted)


@pytest.mark.parametrize("fused", [True, False])
def test_sgd_case(oracle, fused):
    """-0 is a class the update can produce only from a -0 element under a zero sum (the sum
    starts at +0): the case plants one."""
    case = sv.sgd_case()
    refs = sv.sgd_ref(oracle, case, fused)
    partial = 0
    for t, ((R, _), x, I, ref) in enumerate(zip(sv.SGD_SPEC, case["tables"], case["idx"], refs)):
        touched = np.unique(I) - 1
        planted = np.array(sv.sgd_planted_rows(case, t)) - 1
        clean = ~np.isin(touched, planted)
        # no planted bag holds another column, and the reserved ones occur nowhere else
        assert set(np.unique(I[case["bags"]]).tolist()) == set((planted + 1).tolist())
        c = case["cols"][t]
        other = np.delete(I, case["bags"], axis=0)
        assert not np.isin(other, [c["cA"], c["cB"]]).any()
        vet(ref[touched], "f32", clean)
        untouched = np.setdiff1d(np.arange(R), touched)
        assert ref[untouched].tobytes() == x[untouched].tobytes()
        # what the planted values must become (the reference, read feature by feature)
        h1, cA, cB = c["hot"][0] - 1, c["cA"] - 1, c["cB"] - 1
        assert ref[h1, sv.F_INF] == -np.inf and ref[cA, sv.F_INF] == -np.inf
        assert np.isnan(ref[h1, sv.F_INF_NINF]) and np.isnan(ref[h1, sv.F_NAN])
        assert ref[h1, sv.F_MAXMAX] == -np.inf
        assert ref[cA, sv.F_OVF] == -np.inf and np.isfinite(ref[h1, sv.F_OVF])
        assert ref[h1, sv.F_WINF] == np.inf and ref[c["hot"][1] - 1, sv.F_WINF] == -np.inf
        tiny = np.finfo(np.float32).tiny
        assert 0 < abs(ref[cB, sv.F_SUB]) < tiny <= abs(ref[cA, sv.F_SUB])
        assert np.signbit(ref[cA, sv.F_ZERO]) and ref[cA, sv.F_ZERO] == 0
        assert ref[cB, sv.F_ZERO] == x[cB, sv.F_ZERO]
        # chain shapes: the reserved column and the hot ones are chains of entries of
        # several adds, and a planted bag's run leaves a partial entry (r < S)
        counts = np.bincount(I.ravel(), minlength=R + 1)[1:]
        assert counts[cA] == 296 > sv.CHUNK >= counts[cB] == 24
        for col in (c["cA"], c["hot"][0]):
            S, _, _ = sv.chain_shape(I, col)
            runs = (I[case["bags"]] == col).sum(1)
            assert S > 1 and ((runs % S) != 0).any(), (t, col, S)
            partial += int((runs[0] % S) != 0)   # the +Inf bag itself
    assert partial >= len(sv.SGD_SPEC)


def test_queued_cases(oracle):
    for case, R in zip(sv.queued_cases(), sv.QUEUED_ROWS):
        assert case["table"].shape == (R, 128) and sv.is_clean(case) and case["events"] == 2
        ext, I = sv.zero_row_inputs(case, sv.QUEUED_P)
        ref = oracle.pooled_sum(ext, I)
        assert sv.same_special(ref, sv.forward_ref(oracle, case["table"], case["values"],
                                                   case["colptr"], "f32"), "f32")
        vet(ref, "f32", ~case["planted"])


HOT_CASES = [("f32", 128), ("f64", 64), ("f16", 64), ("bf16", 64)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("kind,dim", HOT_CASES)
def test_hot_sgd_cases(oracle, kind, dim, fused, weighted):
    case = sv.hot_sgd_case(kind, dim, weighted)
    ref = sv.hot_sgd_ref(oracle, case, fused)
    values, L = case["values"], case["L"]
    touched = np.unique(values) - 1
    clean = ~np.isin(touched + 1, case["planted_rows"])
    bag = np.repeat(np.arange(sv.HOT_B), L)
    assert set(np.unique(values[np.isin(bag, case["bags"])]).tolist()) == set(case["planted_rows"])
    counts = np.bincount(values, minlength=sv.HOT_ROWS + 1)
    assert counts.max() >= 3000 and len(touched) == 40
    vet(ref[touched], kind, clean)
    untouched = np.setdiff1d(np.arange(sv.HOT_ROWS), touched)
    assert ref[untouched].tobytes() == case["table"][untouched].tobytes()
    if weighted:
        c = sv.census(case["weights"].reshape(1, -1), "f64" if kind == "f64" else "f32")
        assert c["nan"] == 1 and c["+inf"] == 1 and c["-inf"] == 1 and c["subnormal"] == 3


ADA_CASES = [(n, d, rg) for n in ("f32", "bf16") for d in (128, 7) for rg in (False, True)]


@pytest.mark.parametrize("name,dim,ragged", ADA_CASES)
def test_adagrad_elementwise_cases(name, dim, ragged):
    """State elements are sums of squares: never -Inf and never -0."""
    import test_gpu_adagrad as ta

    kind = ta.KINDS[name]
    case = sv.adagrad_case(name, dim, ragged)
    table, state = case["table"].copy(), case["state"].copy()
    with np.errstate(all="ignore"):
        ta.ref_step(kind, table, state, case["delta"], case["lists"])
    touched = np.array(sorted(c for c, b in case["lists"].items() if any(b)))
    assert set(case["planted"]) <= set(touched.tolist())
    clean = ~np.isin(touched, case["planted"])
    vet(table[touched], name, clean)
    vet(state[touched], "f32", clean, need=("nan", "+inf", "subnormal"))
    # column 4 (state = max finite): the state overflows and the row keeps every bit
    assert np.isinf(state[3]).all() and table[3].tobytes() == case["table"][3].tobytes()
    assert state[0].tobytes() == bytes(4 * dim) and table[0].tobytes() == case["table"][0].tobytes()
    # the same definition in longdouble, rounded once: the same classes, close values
    LD = np.longdouble
    dC, tC = kind.toC(case["delta"]), kind.toC(case["table"])
    with np.errstate(all="ignore"):
        for col in case["planted"]:
            g = ta.ref_g(dC, case["lists"][col]).astype(LD)
            # (the state is a stored value: it is rounded to C before the step reads it)
            s1 = (case["state"][col].astype(LD) + g * g).astype(np.float32)
            w2 = tC[col].astype(LD) - LD(np.float32(ta.ETA)) * g / (np.sqrt(s1.astype(LD)) + LD(np.float32(ta.EPS)))
            w1 = kind.toC(kind.toT(w2.astype(np.float32)))
            got_w = kind.toC(table[col])
            assert np.array_equal(np.isnan(s1), np.isnan(state[col])), col
            assert np.array_equal(np.isnan(w1), np.isnan(got_w)), col
            fin = ~np.isnan(w1)
            assert np.allclose(w1[fin], got_w[fin], rtol=2.0 ** -6 if name == "bf16" else 1e-5,
                               atol=1e-30), col
            fin = ~np.isnan(s1)
            assert np.allclose(s1[fin], state[col][fin], rtol=1e-5, atol=1e-44), col


@pytest.mark.parametrize("name,dim,ragged", ADA_CASES)
def test_adagrad_rowwise_cases(name, dim, ragged):
    """Row-wise: one state per column; the reference in C with sequential squares gives the
    classes (any order of a sum that holds Inf or NaN, or overflows from max, agrees)."""
    import test_gpu_adagrad as ta

    kind = ta.KINDS[name]
    case = sv.adagrad_case(name, dim, ragged, rowwise=True)
    with np.errstate(all="ignore"):
        refs = [ta.rowwise_in_C(kind, case["table"], case["state"], case["delta"], case["lists"], o)
                for o in ("sequential", "reversed", "pairwise")]
    t, s = refs[0]
    for t2, s2 in refs[1:]:
        assert np.array_equal(sv.nan_mask(t, name), sv.nan_mask(t2, name))
        assert np.array_equal(np.isnan(s), np.isnan(s2)) and np.array_equal(np.isinf(s), np.isinf(s2))
    touched = np.array(sorted(c for c, b in case["lists"].items() if any(b)))
    clean = ~np.isin(touched, case["planted"])
    c = sv.census(t[touched], name)
    assert c["nan"] > 0 and c["subnormal"] > 0 and c["-0"] > 0 and 8 * c["nan"] <= t[touched].size
    assert 2 * clean.sum() >= len(clean)
    assert np.isnan(s[[5, 6, 7]]).sum() == 1 and np.isinf(s[[3, 5, 7]]).all()
    assert np.isfinite(s[touched[clean]]).all() and np.isfinite(kind.toC(t[touched[clean]])).all()


@pytest.mark.parametrize("dim,kind", [(16, "f32"), (128, "f32"), (7, "f32"), (16, "f16"),
                                      (128, "bf16"), (128, "f64")])
def test_weight_gradient_cases(dim, kind):
    table, delta, values, colptr, bf16, meets = sv.wgrad_case(dim, kind)
    ref, mag = wr.weight_grad_f64(table, delta, values, colptr, bf16)
    assert 0 < meets.sum() <= len(values) // 8
    assert np.isnan(ref[meets]).all() and np.isfinite(ref[~meets]).all()
    assert np.isfinite(mag[~meets]).all()


def test_adagrad_plain_twin_differs_in_the_planted_columns_only():
    case = sv.adagrad_case("f32", 7, True, rowwise=True)
    plain = sv.adagrad_case("f32", 7, True, rowwise=True, plain=True)
    assert case["lists"] == plain["lists"]
    rows = np.nonzero((case["table"] != plain["table"]).any(1))[0]
    assert set(rows) <= set(case["planted"]) and set(np.nonzero(
        case["state"].view(np.uint32) != plain["state"].view(np.uint32))[0]) <= set(case["planted"])


@pytest.mark.parametrize("bits,dim,split", sv.QUANT_CASES)
def test_quantised_cases(bits, dim, split):
    import quant_ref as qr

    for P in (1, 8):
        case = sv.quant_case(bits, dim, P)
        assert sv.is_clean(case)
        # quant_ref's dequantisation is q * scale + bias in Float64, rounded once
        with np.errstate(all="ignore"):
            T = qr.dequantize(case["q"], case["scale"], case["bias"])
            lit = (case["q"].astype(np.float64) * case["scale"].astype(np.float64)[:, None]
                   + case["bias"].astype(np.float64)[:, None]).astype(np.float32)
        assert sv.same_special(T, lit, "f32")
        assert np.isnan(T[0]).all() and np.isfinite(T[case["rows"]["max"] - 1]).all()
        # the packed rows decode to the levels and headers they were built from
        ld = (qr.payload_bytes(dim, bits) + (0 if split else 4) + 3) // 4 * 4
        packed, hdr = sv.quant_pack(case, ld, split)
        q2, s2, b2 = qr.split_rows(packed, dim, bits, hdr)
        assert (q2 == case["q"]).all() and s2.tobytes() == case["scale"].tobytes()
        assert b2.tobytes() == case["bias"].tobytes()
        for out in sv.QUANT_OUTS:
            ref, ev = sv.quant_ref(case, out)
            assert ev == case["events"]
            # subnormals appear in the f16 output only (the Float32 sums are normal)
            need = ALL if out == "f16" else ("nan", "+inf", "-inf", "-0")
            c = sv.census(ref, out)
            for k in need:
                assert c[k] > 0, (out, k, c)
            assert 8 * c["nan"] <= ref.size and 2 * (~case["planted"]).sum() >= sv.FWD_B
            clean_row = int(np.nonzero(~case["planted"])[0][7])
            muts = sv.mutations(ref, out, clean_row)
            assert {"inf to nan", "-0 to +0", "nan a clean row", "swap one inf's sign"} <= set(muts)
            assert (out != "f16") or "flush subnormals" in muts
            for name, m in muts.items():
                assert not sv.same_special(m, ref, out), (out, name)
        # overflow only at the final rounding: the max + max bag is finite in f32 and bf16
        f32, f16 = sv.quant_ref(case, "f32")[0], sv.quant_ref(case, "f16")[0]
        assert (np.isinf(f16) & np.isfinite(f32)).sum() > 0
