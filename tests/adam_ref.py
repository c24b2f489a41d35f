"""A plain numpy model of et_sparse_adam (include/embtab.h states the arithmetic): every
float32 / float64 numpy operation is one correctly rounded IEEE operation, so the model does
the definition operation by operation in the accumulator type C and the kernels must match it
bit for bit.  Rounding to Float16 / BFloat16 goes through torch on the CPU (one RNE)."""
import numpy as np
import torch

CHUNK = 256  # ET_SGD_CHUNK


def lists_fixed(I, nrows):
    """Column (0-based) -> the 1-based gradient columns of its occurrences, in occurrence
    order (bag-major); out-of-range indices belong to no column."""
    I2 = I.reshape(I.shape[0], -1)
    flat = I2.reshape(-1)
    out = {}
    for o in np.argsort(flat, kind="stable"):
        if 1 <= flat[o] <= nrows:
            out.setdefault(int(flat[o]) - 1, []).append(int(o) // I2.shape[1] + 1)
    return out


def lists_ragged(values, colptr, nrows):
    """The same for ragged indices: every entry of the capacity in increasing position, with
    bag 0 for an entry no bag covers (it keeps its list position)."""
    bag = np.zeros(len(values), np.int64)
    for j in range(len(colptr) - 1):
        bag[colptr[j] - 1:colptr[j + 1] - 1] = j + 1
    out = {}
    for k in np.argsort(values, kind="stable"):
        if 1 <= values[k] <= nrows:
            out.setdefault(int(values[k]) - 1, []).append(int(bag[k]))
    return out


def grad_sum(deltaC, bags):
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


class AdamModel:
    """Table (a CPU torch tensor of the table type), moments and step (numpy, type C) of one
    table; ``update`` is one call with work."""

    def __init__(self, table, eta, beta, eps, rowwise=False):
        self.table = table.clone()
        self.C = np.float64 if table.dtype == torch.float64 else np.float32
        C, (R, D) = self.C, table.shape
        self.m = np.zeros((R, D), C)
        self.v = np.zeros(R if rowwise else (R, D), C)
        self.step = np.ones(2, C)
        self.rowwise = rowwise
        self.h = (C(eta), C(eps), C(beta[0]), C(beta[1]), C(1.0 - beta[0]), C(1.0 - beta[1]))

    def toC(self, t):
        return t.to(torch.float64 if self.C is np.float64 else torch.float32).numpy()

    def update(self, delta, lists, feature_order=None):
        C = self.C
        eta, eps, b1, b2, omb1, omb2 = self.h
        self.step = self.step * np.array([b1, b2], C)
        c1, c2 = C(1) - self.step[0], C(1) - self.step[1]
        deltaC, tC = self.toC(delta), self.toC(self.table)
        for col, bags in lists.items():
            if not any(bags):
                continue  # no participating entry: nothing of the column is written
            g = grad_sum(deltaC, bags)
            m2 = (b1 * self.m[col]) + (omb1 * g)
            if self.rowwise:
                ss = C(0)
                for f in (range(len(g)) if feature_order is None else feature_order):
                    ss = ss + g[f] * g[f]
                q = ss / C(len(g))
            else:
                q = g * g
            v2 = (b2 * self.v[col]) + (omb2 * q)
            w2 = tC[col] - (eta * (m2 / c1)) / (np.sqrt(v2 / c2) + eps)
            assert m2.dtype == C and np.asarray(v2).dtype == C and w2.dtype == C
            self.m[col], self.v[col] = m2, v2
            self.table[col] = torch.from_numpy(w2).to(self.table.dtype)
