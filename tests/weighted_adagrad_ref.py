"""Weighted sparse AdaGrad: the numpy restatement of the gradient sum in include/embtab.h
("Sparse AdaGrad over weighted gradients") and the inputs shared by
tests/test_weighted_adagrad_host.py and tests/test_gpu_weighted_adagrad*.py.  The update
itself is tests/test_gpu_adagrad.py's ``ref_step`` fed with ``g_of`` from here; the row-wise
bounds are that file's ``rowwise_bounds`` with the bit-exact weighted ``g`` passed in."""
import numpy as np

import test_gpu_adagrad as ta
import weighted_ref as wr

CHUNK = ta.CHUNK
LD = np.longdouble
ROW_CASES = ta.ROW_CASES


def entry_lists(values, colptr, nrows=ta.R, nnz=None):
    """Column (0-based) -> [(bag, k)] over every entry k of the capacity that holds the column,
    in increasing k; bag is 1-based, 0 for an entry no bag covers (it keeps its position).
    Bags follow the kernels' clamping rule; out-of-range indices belong to no column."""
    nnz = len(values) if nnz is None else nnz
    bag = np.zeros(nnz, np.int64)
    for j, (lo, hi) in enumerate(wr.ranges(colptr, nnz)[0]):
        bag[lo:hi] = j + 1
    out = {}
    for k in np.argsort(values[:nnz], kind="stable"):
        c = int(values[k])
        if 1 <= c <= nrows:
            out.setdefault(c - 1, []).append((int(bag[k]), int(k)))
    return out


def weighted_g(deltaC, entries, weights):
    """The weighted chunk rule: per chunk p = +0, then t = w_k * delta[bag(k)], p = p + t for
    the covered entries in order (two roundings); the partial sums added in chunk order."""
    assert weights.dtype == deltaC.dtype
    parts = []
    with np.errstate(all="ignore"):
        for c0 in range(0, len(entries), CHUNK):
            p = np.zeros(deltaC.shape[1], deltaC.dtype)  # +0
            for b, k in entries[c0:c0 + CHUNK]:
                if b:
                    t = weights[k] * deltaC[b - 1]
                    p = p + t
            parts.append(p)
        g = parts[0]
        for p in parts[1:]:
            g = g + p
    return g


def reference_inputs(kind, delta, values, colptr, weights, nrows=ta.R, nnz=None):
    """(lists, g_of) for ta.ref_step: the bag lists that say which columns participate, and
    the weighted gradient sum of each of those."""
    ent = entry_lists(values, colptr, nrows, nnz)
    deltaC = kind.toC(delta)
    lists = {c: [b for b, _ in e] for c, e in ent.items()}
    g_of = {c: weighted_g(deltaC, e, weights) for c, e in ent.items() if any(b for b, _ in e)}
    return lists, g_of


def ref_step(kind, table, state, delta, values, colptr, weights, nrows=ta.R, nnz=None):
    """The element-wise weighted update, in place on `table` and `state`."""
    lists, g_of = reference_inputs(kind, delta, values, colptr, weights, nrows, nnz)
    with np.errstate(all="ignore"):
        ta.ref_step(kind, table, state, delta, lists, g_of=g_of)
    return lists, g_of


def case_weights(rng, values, colptr, C, lo=0.25, hi=2.0):
    """Weights uniform on [lo, hi) for covered entries, NaN at every entry no bag covers."""
    w = (lo + (hi - lo) * rng.random(len(values))).astype(C)
    covered = np.zeros(len(values), bool)
    for a, b in wr.ranges(colptr, len(values))[0]:
        covered[a:b] = True
    w[~covered] = np.nan
    return w


# --- row-wise -----------------------------------------------------------------------------------

def rowwise_case(name, dim, step):
    """The row-wise tests' inputs for step 0 / 1: N(0, 1) tables and gradients, the ragged case
    of tests/test_gpu_adagrad.py, weights uniform on [0.25, 2)."""
    kind = ta.KINDS[name]
    rng = np.random.default_rng([17, dim, step, sorted(ta.KINDS).index(name)])
    table = kind.fromf(rng.standard_normal((ta.R, dim)))
    state = rng.random(ta.R).astype(kind.C)
    L, values, colptr = ta.ragged_case(rng)
    delta = kind.fromf(rng.standard_normal((len(L), dim)))
    weights = case_weights(rng, values, colptr, kind.C)
    lists, g_of = reference_inputs(kind, delta, values, colptr, weights)
    return {"table": table, "state": state, "values": values, "colptr": colptr, "delta": delta,
            "weights": weights, "lists": lists, "g_of": g_of}


def rowwise_bounds(kind, table, state, g_of, got_table, got_state, eta=ta.ETA, eps=ta.EPS):
    """tests/test_gpu_adagrad.py's rowwise_bounds with the bit-exact gradient sums passed in
    (`g_of`: column -> g in C, the participating columns only).  The derivation does not
    depend on how g was formed, only on g being the exact input of the row-wise step:
        |s - s_ref| <= (dim + 4) u s_ref
        |w - w_ref| <= (dim / 2 + 8) u |step_ref| + (u + uT) |w_ref|
    Columns without a participating entry must be unchanged.  Returns the two ratios."""
    assert np.finfo(LD).eps <= 2.0 ** -60
    C, dim, u, uT = kind.C, table.shape[1], kind.u, kind.uT
    tC, gC = kind.toC(table), kind.toC(got_table)
    eta_c, eps_c = LD(C(eta)), LD(C(eps))
    rs = rw = 0.0
    for col in range(table.shape[0]):
        if col not in g_of:
            assert ta.same(got_table[col], table[col]) and got_state[col] == state[col], col
            continue
        assert g_of[col].dtype == C
        g = g_of[col].astype(LD)
        s_ref = LD(state[col]) + (g * g).sum() / LD(dim)
        step = eta_c * g / (np.sqrt(s_ref) + eps_c)
        w_ref = tC[col].astype(LD) - step
        rs = max(rs, float(abs(LD(got_state[col]) - s_ref) / ((dim + 4) * u * s_ref)))
        bound = (dim / 2 + 8) * u * np.abs(step) + (u + uT) * np.abs(w_ref)
        rw = max(rw, float((np.abs(gC[col].astype(LD) - w_ref) / bound).max()))
    return rs, rw


def rowwise_in_C(kind, table, state, g_of, order, eta=ta.ETA, eps=ta.EPS):
    """The row-wise step evaluated in C with one summation order of the squares."""
    C = kind.C
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

    for col, g in g_of.items():
        s2 = state[col] + total(g * g) / C(g.shape[0])
        w2 = kind.toC(table[col]) - (eta_c * g) / (np.sqrt(s2) + eps_c)
        assert s2.dtype == C and w2.dtype == C
        state[col], table[col] = s2, kind.toT(w2)
    return table, state
