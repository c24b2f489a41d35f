"""Sparse AdaGrad on the GPU (et_sparse_adagrad through ``et.AdaGrad`` / ``update_``).

The expected values come from the reference below, a numpy restatement of the definition in
include/embtab.h: the gradient sum ``g`` of a column is formed chunk by chunk (ET_SGD_CHUNK
list positions each, one vector add per occurrence, the partial sums added in chunk order)
and the update is evaluated with numpy operations in the accumulator type ``C`` (Float32, or
Float64 for Float64 tables), one correctly rounded operation at a time.  The element-wise
form is compared with ``tobytes()`` equality; the row-wise form, whose sum of squares has no
fixed order, against an extended-precision evaluation with a priori bounds (see
``rowwise_bounds``).

Indices: a table of 300 columns with pool 4 x batch 1024, one column each forced to 1, 255,
256, 257, 513 and 2307 occurrences (below, at and above one chunk; two chunks and a rest;
ten chunks), the others uniform over a sub-range, so some columns are never touched."""
import numpy as np
import pytest
import torch

import embtab as et
from embtab.tables import Static
from test_gpu_ragged import LENMIX, ScatteredColumns, colptr_of, dev, host, mix_lengths, same

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHUNK = et._lib.ET_SGD_CHUNK
R, B, P = 300, 1024, 4
FORCED = {3: 1, 10: 255, 11: 256, 12: 257, 13: 513, 14: 2307}  # 1-based column: occurrences
ETA, EPS = 0.1, 1e-8
LD = np.longdouble


# --- element kinds -----------------------------------------------------------------------------

class Kind:
    def __init__(self, name, store, C, tdtype, uT):
        self.name, self.store, self.C, self.torch, self.uT = name, store, C, tdtype, uT
        self.u = 2.0 ** -53 if C is np.float64 else 2.0 ** -24

    def fromf(self, x):
        """Float64 values -> the table's storage (bfloat16 as its uint16 bit patterns)."""
        if self.name == "bf16":
            from oracle import f32_to_bf16

            return f32_to_bf16(x.astype(np.float32))
        return x.astype(self.store)

    def toC(self, a):
        if self.name == "bf16":
            from oracle import bf16_to_f32

            return bf16_to_f32(a)
        return a.astype(self.C)

    def toT(self, c):
        """One round-to-nearest-even conversion from C to the table type."""
        if self.name == "bf16":
            from oracle import f32_to_bf16

            return f32_to_bf16(c)
        return c.astype(self.store)

    def dev(self, a):
        if self.name == "bf16":
            return dev(a.view(np.int16)).view(torch.bfloat16)
        return dev(a)


KINDS = {k.name: k for k in (Kind("f32", np.float32, np.float32, torch.float32, 0.0),
                             Kind("f64", np.float64, np.float64, torch.float64, 0.0),
                             Kind("f16", np.float16, np.float32, torch.float16, 2.0 ** -11),
                             Kind("bf16", np.uint16, np.float32, torch.bfloat16, 2.0 ** -8))}


# --- inputs ------------------------------------------------------------------------------------

def make_indices(rng):
    forced = np.concatenate([np.full(c, r) for r, c in FORCED.items()])
    others = np.arange(20, 261)  # 1-based; columns 1, 2, 4..9, 15..19 and 261..300 stay untouched
    rest = rng.choice(others, B * P - len(forced))
    I = rng.permutation(np.concatenate([forced, rest])).reshape(B, P).astype(np.int64)
    cnt = np.bincount(I.reshape(-1), minlength=R + 1)
    assert all(cnt[r] == c for r, c in FORCED.items())
    return I


def lists_fixed(I, nrows=R):
    """Column (0-based) -> the 1-based gradient columns of its occurrences, in occurrence
    order (bag-major, the entry fastest); out-of-range indices belong to no column."""
    I2 = I.reshape(I.shape[0], -1)
    flat = I2.reshape(-1)
    out = {}
    for o in np.argsort(flat, kind="stable"):
        c = int(flat[o])
        if 1 <= c <= nrows:
            out.setdefault(c - 1, []).append(o // I2.shape[1] + 1)
    return out


def lists_ragged(values, colptr, nrows=R):
    """The same for ragged indices: every entry k of the capacity holding the column, in
    increasing k, with bag 0 for an entry no bag covers (it keeps its list position)."""
    bag = np.zeros(len(values), np.int64)
    for j in range(len(colptr) - 1):
        bag[colptr[j] - 1:colptr[j + 1] - 1] = j + 1
    out = {}
    for k in np.argsort(values, kind="stable"):
        c = int(values[k])
        if 1 <= c <= nrows:
            out.setdefault(c - 1, []).append(int(bag[k]))
    return out


# --- the reference -----------------------------------------------------------------------------

def ref_g(deltaC, bags):
    parts = []
    for c0 in range(0, len(bags), CHUNK):
        p = np.zeros(deltaC.shape[1], deltaC.dtype)  # +0
        for b in bags[c0:c0 + CHUNK]:
            if b:
                p = p + deltaC[b - 1]
        parts.append(p)
    g = parts[0]
    for p in parts[1:]:
        g = g + p
    return g


def ref_step(kind, table, state, delta, lists, eta=ETA, eps=EPS, g_of=None):
    """The element-wise update, in place on `table` (storage type) and `state` (C)."""
    C = kind.C
    deltaC = kind.toC(delta)
    eta_c, eps_c = C(eta), C(eps)
    for col, bags in lists.items():
        if not any(bags):
            continue  # no participating entry: neither the column nor its state is written
        g = ref_g(deltaC, bags) if g_of is None else g_of[col]
        assert g.dtype == C
        s2 = state[col] + g * g
        d = np.sqrt(s2) + eps_c
        w2 = kind.toC(table[col]) - (eta_c * g) / d
        assert s2.dtype == C and w2.dtype == C
        state[col] = s2
        table[col] = kind.toT(w2)


def wide_pair(kind, a, off=4, pad=8):
    """`a` as columns off..off+D of a wider device tensor prefilled with a byte pattern."""
    wide = torch.empty((a.shape[0], a.shape[1] + pad), dtype=kind.torch, device=DEV)
    wide.view(torch.uint8).fill_(0xA5)
    view = wide[:, off:off + a.shape[1]]
    view.copy_(kind.dev(a))
    return wide, view


def padding_intact(wide, D, off=4):
    h = host(wide)
    rest = np.ascontiguousarray(np.delete(h, np.s_[off:off + D], axis=1))
    return rest.tobytes() == b"\xa5" * rest.nbytes


def fixed_grad(kind, A, delta, I):
    return et.SparseEmbeddingUpdate(A.lookup_type, kind.dev(delta), dev(I))


# --- 1. geometry ---------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("dim", [128, 16, 20, 1504, 7])
def test_geometry(dim):
    kind = KINDS["f32"]
    rng = np.random.default_rng(100 + dim)
    table = rng.standard_normal((R, dim)).astype(np.float32)
    state = rng.random((R, dim)).astype(np.float32)
    table0, state0 = table.copy(), state.copy()
    tw, tv = wide_pair(kind, table)
    sw, sv = wide_pair(kind, state)
    A = et.SimpleEmbedding(tv)
    assert A.ld == dim + 8
    opt = et.AdaGrad(ETA, EPS)
    opt.set_state(A, sv)
    touched = set()
    for step in range(2):  # fresh indices and gradients; the state is carried
        I = make_indices(rng)
        delta = rng.standard_normal((B, dim)).astype(np.float32)
        et.update_(opt, A, fixed_grad(kind, A, delta, I), nontemporal=step == 0)
        ref_step(kind, table, state, delta, lists_fixed(I))
        touched |= set((I.reshape(-1) - 1).tolist())
        assert same(host(tv), table), step
        assert same(host(sv), state), step
        assert padding_intact(tw, dim) and padding_intact(sw, dim)
    untouched = np.setdiff1d(np.arange(R), sorted(touched))
    assert len(untouched) >= 50
    assert same(host(tv)[untouched], table0[untouched])
    assert same(host(sv)[untouched], state0[untouched])
    assert not same(state, state0)
    assert et.check_errors() == 0


# --- 2. the gradient sum is the existing oracle's ------------------------------------------------

@gpu
def test_gradient_sum_links_to_the_sgd_oracle(oracle):
    kind = KINDS["f32"]
    rng = np.random.default_rng(2)
    dim = 128
    I = rng.integers(1, R + 1, (B, P)).astype(np.int64)
    assert np.bincount(I.reshape(-1)).max() <= CHUNK  # every column is one chunk
    delta = rng.standard_normal((B, dim)).astype(np.float32)
    G = np.zeros((R, dim), np.float32)
    oracle.sgd(G, delta, I, -1.0, fused=True)  # fma(1, acc, 0): the serial sum itself
    lists = lists_fixed(I)
    for col, bags in lists.items():
        assert same(ref_g(delta, bags), G[col]), col
    table = rng.standard_normal((R, dim)).astype(np.float32)
    state = rng.random((R, dim)).astype(np.float32)
    A = et.SimpleEmbedding(dev(table))
    opt = et.AdaGrad(ETA, EPS)
    opt.state(A).copy_(dev(state))
    et.update_(opt, A, fixed_grad(kind, A, delta, I))
    ref_step(kind, table, state, delta, lists, g_of=G)
    assert same(host(A.data), table) and same(host(opt.state(A)), state)
    assert et.check_errors() == 0


# --- 3. element types ------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("dim", [128, 20])
@pytest.mark.parametrize("name", ["f64", "f16", "bf16"])
def test_element_types(name, dim):
    kind = KINDS[name]
    rng = np.random.default_rng(300 + dim)
    table = kind.fromf(rng.standard_normal((R, dim)))
    state = rng.random((R, dim)).astype(kind.C)
    A = et.SimpleEmbedding(kind.dev(table))
    opt = et.AdaGrad(ETA, EPS)
    S = opt.state(A)
    assert S.dtype == (torch.float64 if name == "f64" else torch.float32) and S.shape == (R, dim)
    S.copy_(dev(state))
    for step in range(2):
        I = make_indices(rng)
        delta = kind.fromf(rng.standard_normal((B, dim)))
        et.update_(opt, A, fixed_grad(kind, A, delta, I), nontemporal=step == 1)
        ref_step(kind, table, state, delta, lists_fixed(I))
        assert same(host(A.data), table), step
        assert same(host(S), state), step
    assert et.check_errors() == 0


# --- 4. storage ------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("store", ["split64", "colptr_vec", "colptr_generic"])
def test_storage(store):
    kind = KINDS["f32"]
    rng = np.random.default_rng(4)
    dim = 10 if store == "colptr_generic" else 128
    table = rng.standard_normal((R, dim)).astype(np.float32)
    state = rng.random((R, dim)).astype(np.float32)
    if store == "split64":
        A = et.SplitEmbedding(dev(table), 64)
        dense = lambda: host(A.to_dense())
    else:
        A = ScatteredColumns(table, dim + (4 if store == "colptr_vec" else 3), rng)
        dense = A.dense
    opt = et.AdaGrad(ETA, EPS)
    S = opt.state(A)  # one contiguous (R, D) allocation whatever the table's storage
    assert S.is_contiguous() and S.shape == (R, dim)
    S.copy_(dev(state))
    for step in range(2):
        I = make_indices(rng)
        delta = rng.standard_normal((B, dim)).astype(np.float32)
        et.update_(opt, A, fixed_grad(kind, A, delta, I))
        ref_step(kind, table, state, delta, lists_fixed(I))
        assert same(dense(), table) and same(host(S), state), step
    assert et.check_errors() == 0


# --- 5. ragged ---------------------------------------------------------------------------------------

def ragged_case(rng, nb=301, head=40, tail=600):
    """Lengths from LENMIX; the bag of 300 entries and the 40 entries in front of the first
    bag all hold column 14, so its list is longer than a chunk and its chunk boundaries
    depend on entries no bag covers; a capacity tail of valid indices, column 14 among them."""
    L = mix_lengths(nb, rng)
    used = int(L.sum())
    values = rng.integers(20, 261, head + used + tail).astype(np.int64)
    colptr = colptr_of(L) + head
    j = int(np.nonzero(L == 300)[0][0])
    values[colptr[j] - 1:colptr[j + 1] - 1] = 14
    values[:head] = 14
    values[head + used::7] = 14
    values[-3:] = 5  # a column that only the tail holds: no participating entry
    return L, values, colptr


@gpu
@pytest.mark.parametrize("name,dim", [("f32", 128), ("f32", 20), ("f32", 7), ("bf16", 128)])
def test_ragged(name, dim):
    kind = KINDS[name]
    rng = np.random.default_rng(500 + dim)
    nb = 301
    L, values, colptr = ragged_case(rng)
    lists = lists_ragged(values, colptr)
    assert len(lists[13]) > CHUNK + 40 and lists[13][0] == 0 and lists[13][-1] == 0
    assert any(not any(b) for b in lists.values())  # a column present in the tail only
    table = kind.fromf(rng.standard_normal((R, dim)))
    state = rng.random((R, dim)).astype(kind.C)
    delta = kind.fromf(rng.standard_normal((nb, dim)))
    A = et.SimpleEmbedding(kind.dev(table))
    opt = et.AdaGrad(ETA, EPS)
    opt.state(A).copy_(dev(state))
    Rg = et.RaggedIndices(dev(values), dev(colptr))
    et.update_(opt, A, et.SparseEmbeddingUpdate(A.lookup_type, kind.dev(delta), Rg))
    ref_step(kind, table, state, delta, lists)
    assert same(host(A.data), table) and same(host(opt.state(A)), state)
    assert et.check_errors() == 0
    assert set(LENMIX) <= set(L.tolist())


@gpu
@pytest.mark.parametrize("dim", [128, 7])
def test_ragged_bags_of_four_equal_the_fixed_pool(dim):
    kind = KINDS["f32"]
    rng = np.random.default_rng(55)
    I = make_indices(rng)
    table = rng.standard_normal((R, dim)).astype(np.float32)
    delta = rng.standard_normal((B, dim)).astype(np.float32)
    tail = rng.integers(1, R + 1, 500).astype(np.int64)
    Rg = et.RaggedIndices(dev(np.concatenate([I.reshape(-1), tail])),
                          dev(colptr_of(np.full(B, P))))
    got = []
    for indices in (dev(I), Rg):
        A = et.SimpleEmbedding(dev(table))
        opt = et.AdaGrad(ETA, EPS, initial_accumulator_value=0.5)
        et.update_(opt, A, et.SparseEmbeddingUpdate(A.lookup_type, dev(delta), indices))
        got.append((host(A.data), host(opt.state(A))))
    assert same(got[0][0], got[1][0]) and same(got[0][1], got[1][1])
    state = np.full((R, dim), 0.5, np.float32)
    ref_step(kind, table, state, delta, lists_fixed(I))
    assert same(got[0][0], table) and same(got[0][1], state)
    assert et.check_errors() == 0


# --- 6. multi-table ------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("k", [3, 4])  # prependrows: element-aligned, then 16-byte aligned
def test_multi_table_equals_single_calls(k):
    rng = np.random.default_rng(6)
    dims = [128, 64, 20, 128, 128]
    hs = [rng.standard_normal((R, d)).astype(np.float32) for d in dims]
    L = mix_lengths(B, rng)
    values = rng.integers(1, R + 1, int(L.sum()) + 100).astype(np.int64)
    Is = [dev(make_indices(rng)) for _ in range(4)]
    Is.append(et.RaggedIndices(dev(values), dev(colptr_of(L))))
    delta = dev(rng.standard_normal((B, k + sum(dims))).astype(np.float32))

    def build():
        As = [et.SimpleEmbedding(dev(hs[0])), et.SimpleEmbedding(dev(hs[1]), Static(64)),
              et.SimpleEmbedding(dev(hs[2])), et.SplitEmbedding(dev(hs[3]), 64),
              et.SimpleEmbedding(dev(hs[4]))]
        offs = np.cumsum([k] + dims)
        grads = [et.SparseEmbeddingUpdate(A.lookup_type, delta[:, offs[t]:offs[t + 1]], Is[t])
                 for t, A in enumerate(As)]
        assert grads[1].delta.stride(0) == k + sum(dims)
        return As, grads, et.AdaGrad(ETA, EPS, initial_accumulator_value=0.1)

    As, grads, opt = build()
    Bs, grads1, opt1 = build()
    for step in range(2):
        et.update_(opt, As, grads)
        for A, g in zip(Bs, grads1):
            et.update_(opt1, A, g)
    dense = lambda A: host(A.to_dense() if isinstance(A, et.SplitEmbedding) else A.data)
    for t, (A, A1) in enumerate(zip(As, Bs)):
        assert same(dense(A), dense(A1)), t
        assert same(host(opt.state(A)), host(opt1.state(A1))), t
        assert not same(dense(A), hs[t])
    # an empty gradient in the list is skipped
    empty = et.SparseEmbeddingUpdate(As[0].lookup_type, delta[:0, k:k + 128],
                                     torch.empty((0, P), dtype=torch.int64, device=DEV))
    before = dense(As[1])
    et.update_(opt, [As[0], As[1]], [empty, grads[1]])
    assert same(dense(As[0]), dense(Bs[0])) and not same(dense(As[1]), before)
    assert et.check_errors() == 0


# --- 7. row-wise ------------------------------------------------------------------------------------------

ROW_CASES = [(n, d) for n in ("f32", "f64", "f16", "bf16") for d in (128, 20, 7)]


def rowwise_inputs(name, dim, step):
    """Tables and gradients N(0, 1) (nothing subnormal), the test's own inputs for step 0 / 1."""
    kind = KINDS[name]
    rng = np.random.default_rng([7, dim, step, sorted(KINDS).index(name)])
    return (kind.fromf(rng.standard_normal((R, dim))), rng.random(R).astype(kind.C),
            make_indices(rng), kind.fromf(rng.standard_normal((B, dim))))


def rowwise_bounds(kind, table, state, delta, lists, got_table, got_state, eta=ETA, eps=EPS):
    """Largest observed-to-bound ratio of (got_table, got_state) against the definition
    evaluated in extended precision (np.longdouble: unit roundoff 2^-64, negligible beside
    u = 2^-24 and 2^-53) from the bit-exact g, per touched column:
        |s - s_ref| <= (dim + 4) u s_ref
        |w - w_ref| <= (dim / 2 + 8) u |step_ref| + (u + uT) |w_ref|
    Any order of summing dim non-negative terms g_f^2 (each rounded once) has relative error
    <= (dim - 1 + 1) u; the division by dim and the add to s are two more roundings, plus
    second-order slack: dim + 4.  sqrt halves that, then sqrt, + eps, eta * g and / round once
    each: dim / 2 + 6, with slack dim / 2 + 8 on the step; the subtraction and the rounding
    to T are relative to w'.  Untouched columns must be unchanged.  Returns the two ratios."""
    assert np.finfo(LD).eps <= 2.0 ** -60
    C, dim, u, uT = kind.C, table.shape[1], kind.u, kind.uT
    deltaC, tC, gC = kind.toC(delta), kind.toC(table), kind.toC(got_table)
    eta_c, eps_c = LD(C(eta)), LD(C(eps))
    rs = rw = 0.0
    for col in range(table.shape[0]):
        bags = lists.get(col, [])
        if not any(bags):
            assert same(got_table[col], table[col]) and got_state[col] == state[col], col
            continue
        g = ref_g(deltaC, bags).astype(LD)
        s_ref = LD(state[col]) + (g * g).sum() / LD(dim)
        step = eta_c * g / (np.sqrt(s_ref) + eps_c)
        w_ref = tC[col].astype(LD) - step
        rs = max(rs, float(abs(LD(got_state[col]) - s_ref) / ((dim + 4) * u * s_ref)))
        bound = (dim / 2 + 8) * u * np.abs(step) + (u + uT) * np.abs(w_ref)
        rw = max(rw, float((np.abs(gC[col].astype(LD) - w_ref) / bound).max()))
    return rs, rw


def rowwise_in_C(kind, table, state, delta, lists, order, eta=ETA, eps=EPS):
    """The row-wise definition evaluated in C with one summation order of the squares."""
    C = kind.C
    deltaC = kind.toC(delta)
    eta_c, eps_c = C(eta), C(eps)
    table, state = table.copy(), state.copy()

    def total(x):
        if order == "pairwise":
            while len(x) > 1:
                if len(x) % 2:
                    x = np.concatenate([x, np.zeros(1, C)])
                x = x[0::2] + x[1::2]
            return x[0]
        acc = C(0)
        for v in (x if order == "sequential" else x[::-1]):
            acc = acc + v
        return acc

    for col, bags in lists.items():
        if not any(bags):
            continue
        g = ref_g(deltaC, bags)
        s2 = state[col] + total(g * g) / C(g.shape[0])
        w2 = kind.toC(table[col]) - (eta_c * g) / (np.sqrt(s2) + eps_c)
        assert s2.dtype == C and w2.dtype == C
        state[col], table[col] = s2, kind.toT(w2)
    return table, state


@pytest.mark.parametrize("name,dim", ROW_CASES)
def test_rowwise_bounds_hold_for_cpu_summation_orders(name, dim):
    """No GPU: the bounds' derivation checked on the GPU test's own inputs with three
    summation orders evaluated in C.  A ratio of 1 or more would mean the derivation is wrong."""
    kind = KINDS[name]
    table, state, I, delta = rowwise_inputs(name, dim, 0)
    lists = lists_fixed(I)
    worst = 0.0
    for order in ("sequential", "reversed", "pairwise"):
        t2, s2 = rowwise_in_C(kind, table, state, delta, lists, order)
        rs, rw = rowwise_bounds(kind, table, state, delta, lists, t2, s2)
        print(f"rowwise bound ratio {name} dim {dim} {order}: state {rs:.3f} table {rw:.3f}")
        worst = max(worst, rs, rw)
    assert worst < 1.0


@gpu
@pytest.mark.parametrize("name,dim", ROW_CASES)
def test_rowwise(name, dim):
    kind = KINDS[name]
    table, state, _, _ = rowwise_inputs(name, dim, 0)
    A = et.SimpleEmbedding(kind.dev(table))
    opt = et.AdaGrad(ETA, EPS, rowwise=True)
    S = opt.state(A)
    assert S.shape == (R,) and S.dtype == (torch.float64 if name == "f64" else torch.float32)
    S.copy_(dev(state))
    for step in range(2):
        _, _, I, delta = rowwise_inputs(name, dim, step)
        et.update_(opt, A, fixed_grad(kind, A, delta, I), nontemporal=step == 0)
        got_t, got_s = host(A.data), host(S)
        rs, rw = rowwise_bounds(kind, table, state, delta, lists_fixed(I), got_t, got_s)
        print(f"rowwise GPU ratio {name} dim {dim} step {step}: state {rs:.3f} table {rw:.3f}")
        assert rs <= 1.0 and rw <= 1.0, (step, rs, rw)
        table, state = got_t, got_s  # each step is judged alone, from what the GPU wrote
    assert et.check_errors() == 0


# --- 8. out-of-range indices ----------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("dim", [128, 7])
def test_out_of_range_indices_are_counted_and_skipped(dim):
    kind = KINDS["f32"]
    rng = np.random.default_rng(8)
    I = make_indices(rng)
    flat = I.reshape(-1)
    bad = rng.choice(np.nonzero(flat >= 20)[0], 6, replace=False)
    flat[bad[:3]], flat[bad[3:]] = 0, R + 1
    table = rng.standard_normal((R, dim)).astype(np.float32)
    state = rng.random((R, dim)).astype(np.float32)
    delta = rng.standard_normal((B, dim)).astype(np.float32)
    for rowwise in (False, True):
        A = et.SimpleEmbedding(dev(table))
        opt = et.AdaGrad(ETA, EPS, rowwise=rowwise)
        if not rowwise:
            opt.state(A).copy_(dev(state))
        et.check_errors()
        et.update_(opt, A, fixed_grad(kind, A, delta, I))
        assert et.check_errors() == 6
        if rowwise:  # within the row-wise bounds of the lists without the bad occurrences
            rs, rw = rowwise_bounds(kind, table, np.zeros(R, np.float32), delta, lists_fixed(I),
                                    host(A.data), host(opt.state(A)))
            assert rs <= 1.0 and rw <= 1.0, (rs, rw)
            continue
        t2, s2 = table.copy(), state.copy()
        ref_step(kind, t2, s2, delta, lists_fixed(I))
        assert same(host(A.data), t2) and same(host(opt.state(A)), s2)


# --- 9. graph capture --------------------------------------------------------------------------------------

@gpu
def test_graph_capture_refill():
    kind = KINDS["f32"]
    rng = np.random.default_rng(9)
    dim = 128
    table = rng.standard_normal((R, dim)).astype(np.float32)
    Idev = torch.ones((B, P), dtype=torch.int64, device=DEV)
    ddev = torch.zeros((B, dim), device=DEV)

    def fill():
        I = make_indices(rng)
        delta = rng.standard_normal((B, dim)).astype(np.float32)
        Idev.copy_(dev(I))
        ddev.copy_(dev(delta))
        return I, delta

    def step(T, o, out):
        et.lookup_(out, T, Idev)
        et.update_(o, T, et.SparseEmbeddingUpdate(T.lookup_type, ddev, Idev))

    fill()
    A = et.SimpleEmbedding(dev(table), Static(dim))
    opt = et.AdaGrad(ETA, EPS)
    opt.state(A)  # allocated before the capture
    dst = torch.empty((B, dim), device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # one eager step first (workspaces), on a scratch table
        step(et.SimpleEmbedding(dev(table), Static(dim)), et.AdaGrad(ETA, EPS),
             torch.empty_like(dst))
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(A, opt, dst)
    I2, delta2 = fill()  # refill the indices and the gradient in place, then replay
    g.replay()
    torch.cuda.synchronize()
    A2 = et.SimpleEmbedding(dev(table), Static(dim))
    opt2 = et.AdaGrad(ETA, EPS)
    dst2 = torch.empty_like(dst)
    step(A2, opt2, dst2)
    assert same(host(dst), host(dst2))
    assert same(host(A.data), host(A2.data)) and same(host(opt.state(A)), host(opt2.state(A2)))
    state = np.zeros((R, dim), np.float32)
    ref_step(kind, table, state, delta2, lists_fixed(I2))
    assert same(host(A.data), table) and same(host(opt.state(A)), state)
    assert et.check_errors() == 0
