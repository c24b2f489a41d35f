"""Weighted sparse Adam: no arithmetic of its own.  Consequence (b) of include/embtab.h
("Sparse Adam over weighted gradients") says the weighted update is et_sparse_adam of the
expanded gradient with every covered entry its own bag, so the expected values are
tests/adam_ref.py's AdamModel fed with that gradient: one numpy multiply per element in C."""
import numpy as np
import torch

from adam_ref import AdamModel  # noqa: F401  (the tests take the model from here)


def expanded(delta, values, colptr, weights, nrows):
    """(E, lists) for ``AdamModel.update``: ``E[k] = fl_C(w_k * C(delta[bag(k)]))`` for every
    entry a bag covers (a zero row elsewhere: the weight there is never read), as a CPU tensor
    of type C, and column (0-based) -> its entries in increasing k, ``k + 1`` for a covered one
    and 0 for one no bag covers (it keeps its list position)."""
    C = weights.dtype.type
    bag = np.zeros(len(values), np.int64)
    for j in range(len(colptr) - 1):
        bag[colptr[j] - 1:colptr[j + 1] - 1] = j + 1
    covered = bag > 0
    dC = delta.to(torch.float64 if C is np.float64 else torch.float32).numpy()
    E = np.zeros((len(values), dC.shape[1]), C)
    E[covered] = weights[covered][:, None] * dC[bag[covered] - 1]
    assert E.dtype == C
    lists = {}
    for k in np.argsort(values, kind="stable"):
        if 1 <= values[k] <= nrows:
            lists.setdefault(int(values[k]) - 1, []).append(int(k) + 1 if covered[k] else 0)
    return torch.from_numpy(E), lists
