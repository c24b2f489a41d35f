"""Sparse Adam, the parts that need no GPU: the exported symbols, the ctypes mirror of
et_adam_desc, every argument and flag error of et_sparse_adam (status codes before any device
work), and what ``et.Adam`` / ``update_`` refuse."""
import ctypes
import os
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20  # dummy device addresses: every call below stops at the host checks
COL = 100 * 16 * 4  # bytes of a 100 x 16 Float32 block


def _desc(L, **kw):
    d = dict(table=P, ld_table=16, nrows=100, dim=16, pool=4, delta=2 * P, ld_delta=16,
             idx=3 * P, ld_idx=4, batch=8, cols_per_page=0, colptr=0, nnz=0, m=5 * P, ld_m=16,
             v=6 * P, ld_v=16, step=7 * P)
    d.update(kw)
    return L.AdamDesc(*[d[f[0]] for f in L.AdamDesc._fields_])


def test_symbols_and_struct_layout(tmp_path):
    from embtab import _lib

    L = _lib.load()
    assert hasattr(L, "et_sparse_adam") and hasattr(L, "et_adam_workspace_size")
    assert L.et_abi_version() == 9
    S = _lib.AdamDesc
    fields = [f[0] for f in S._fields_]
    args = ", ".join(["sizeof(et_adam_desc)"] + [f"offsetof(et_adam_desc, {f})" for f in fields])
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "embtab.h"\n'
                    f'int main(void) {{\n  size_t x[] = {{{args}}};\n'
                    '  for (unsigned i = 0; i < sizeof x / sizeof *x; ++i) printf("%zu ", x[i]);\n'
                    '  printf("%u %d\\n", ET_FLAG_ADAM_ROWWISE, ET_ADAM_VEC_MAX_DIM);\n'
                    '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)],
                   check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                       check=True).stdout.split()))
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields] + [
        _lib.ET_FLAG_ADAM_ROWWISE, _lib.ET_ADAM_VEC_MAX_DIM]
    assert _lib.ET_FLAG_ADAM_ROWWISE == _lib.ET_FLAG_ADAGRAD_ROWWISE
    # the same sizes cost what AdaGrad's workspace costs
    a = (S * 1)(_desc(_lib, batch=1000))
    g = (_lib.AdaGradDesc * 1)(_lib.AdaGradDesc(P, 16, 100, 16, 4, 2 * P, 16, 3 * P, 4, 1000, 0,
                                                0, 0, 5 * P, 16))
    na, ng = ctypes.c_int64(0), ctypes.c_int64(0)
    assert L.et_adam_workspace_size(ctypes.addressof(a), 1, ctypes.byref(na)) == 0
    assert L.et_adagrad_workspace_size(ctypes.addressof(g), 1, ctypes.byref(ng)) == 0
    assert na.value == ng.value > 0
    assert L.et_adam_workspace_size(ctypes.addressof(a), 1, None) == -1


def test_julia_shim_binds_adam():
    from test_julia_abi import JL_FIELD, header_structs, shim_ccalls, shim_structs

    jf = [(n, JL_FIELD[t]) for n, t in shim_structs()["AdamDesc"]]
    assert jf == header_structs()["et_adam_desc"]
    assert {"et_adam_workspace_size", "et_sparse_adam"} <= {c[0] for c in shim_ccalls()}


ROW = 512
ARG_ERRORS = [  # (descriptor fields, flags, betas, expected status)
    ({}, 0, (0.9, 0.999), -3),                       # valid: stops at the missing workspace
    ({}, ROW | 1, (0.0, 0.0), -3),
    ({"m": 0}, 0, (0.9, 0.999), -1), ({"v": 0}, 0, (0.9, 0.999), -1),
    ({"step": 0}, ROW, (0.9, 0.999), -1),
    ({"ld_m": 15}, ROW, (0.9, 0.999), -1), ({"ld_v": 15}, 0, (0.9, 0.999), -1),
    ({"ld_v": 0}, ROW, (0.9, 0.999), -3),            # ignored by the row-wise form
    ({"m": P + COL - 4}, 0, (0.9, 0.999), -1),       # m overlaps the table's last element
    ({"m": P + COL}, 0, (0.9, 0.999), -3),           # right behind it
    ({"v": P - COL + 4}, 0, (0.9, 0.999), -1),       # v overlaps the table's first element
    ({"v": P - 400}, ROW, (0.9, 0.999), -3), ({"v": P - 396}, ROW, (0.9, 0.999), -1),
    ({"v": 5 * P + COL - 4}, 0, (0.9, 0.999), -1),   # the moments overlap each other
    ({"v": 5 * P + COL}, 0, (0.9, 0.999), -3),       # two blocks of one allocation
    ({"step": 5 * P + 8}, 0, (0.9, 0.999), -1), ({"step": P + COL - 4}, 0, (0.9, 0.999), -1),
    ({"step": 6 * P + COL}, 0, (0.9, 0.999), -3),
    ({}, 0, (1.0, 0.999), -1), ({}, 0, (0.9, -0.1), -1), ({}, 0, (float("nan"), 0.5), -1),
    ({"dim": -1}, 0, (0.9, 0.999), -1), ({"nnz": -1}, 0, (0.9, 0.999), -1),
    ({"table": 0}, 0, (0.9, 0.999), -1), ({"ld_delta": 8}, 0, (0.9, 0.999), -1),
    ({"batch": 0, "m": 0, "v": 0, "step": 0}, 0, (0.9, 0.999), 0),  # no work: nothing is read
    ({}, 4, (0.9, 0.999), -4), ({}, 256 | ROW, (0.9, 0.999), -4), ({}, 8, (0.9, 0.999), -4),
    ({}, 32, (0.9, 0.999), -4), ({}, 128, (0.9, 0.999), -4), ({}, 2, (0.9, 0.999), -4),
    ({}, 1024, (0.9, 0.999), -1),
]


@pytest.mark.parametrize("kw,flags,beta,rc", ARG_ERRORS)
def test_argument_errors_need_no_gpu(kw, flags, beta, rc):
    from embtab import _lib

    L = _lib.load()
    arr = (_lib.AdamDesc * 1)(_desc(_lib, **kw))
    for ragged in (False, True):
        if ragged:
            arr[0].pool, arr[0].ld_idx, arr[0].colptr, arr[0].nnz = 0, 0, 4 * P, max(kw.get("nnz", 64), -1)
        got = L.et_sparse_adam(_lib.ET_F32, ctypes.addressof(arr), 1, 1e-3, beta[0], beta[1], 1e-8,
                               flags, None, 0, None)
        assert got == rc, (ragged, L.et_last_error())


def test_call_level_errors():
    from embtab import _lib

    L = _lib.load()

    def call(arr, n, dtype=_lib.ET_F32):
        return L.et_sparse_adam(dtype, ctypes.addressof(arr) if arr is not None else None, n,
                                1e-3, 0.9, 0.999, 1e-8, 0, None, 0, None)

    one = (_lib.AdamDesc * 1)(_desc(_lib))
    for dtype in (_lib.ET_I32, _lib.ET_I64, 99):
        assert call(one, 1, dtype) == -4
    for dtype in (_lib.ET_F64, _lib.ET_F16, _lib.ET_BF16):
        assert call(one, 1, dtype) == -3
    assert call(None, 0) == 0 and call(None, 1) == -1 and call(one, -1) == -1
    assert call((_lib.AdamDesc * 33)(), 33) == -1 and b"32" in L.et_last_error()
    # two tables: the same step, then one table's moment inside the other's table
    two = (_lib.AdamDesc * 2)(_desc(_lib), _desc(_lib, table=8 * P, m=9 * P, v=10 * P))
    assert call(two, 2) == -1 and b"same step" in L.et_last_error()
    two[1].step = 11 * P
    assert call(two, 2) == -3
    two[1].v = P + 64
    assert call(two, 2) == -1 and b"overlaps" in L.et_last_error()
    two[1].v, two[1].batch = 10 * P, 0  # a table without work is not looked at
    two[1].step = two[0].step
    assert call(two, 2) == -3


def test_optimiser_object_and_refusals():
    import embtab as et

    A = et.SimpleEmbedding(torch.zeros((10, 16)))
    g = et.SparseEmbeddingUpdate(A.lookup_type, torch.zeros((4, 16)),
                                 torch.ones((4, 2), dtype=torch.int64))
    opt = et.Adam()
    assert (opt.eta, opt.beta, opt.eps, opt.rowwise) == (1e-3, (0.9, 0.999), 1e-8, False)
    m, v = opt.state(A)
    assert m.shape == v.shape == (10, 16) and m.dtype == torch.float32 and not m.any()
    assert opt.state(A)[0] is m and opt.step(A) is opt.step(A)
    assert opt.step(A).tolist() == [1.0, 1.0]
    row = et.Adam(rowwise=True)
    H = et.SimpleEmbedding(torch.zeros((10, 16), dtype=torch.float64))
    assert row.state(H)[1].shape == (10,) and row.step(H).dtype == torch.float64
    wide = torch.zeros((10, 40))
    assert opt.set_state(A, wide[:, :16], wide[:, 20:36])[1] is opt.state(A)[1]
    for bad in (torch.zeros((10, 15)), torch.zeros((10, 16), dtype=torch.float64),
                torch.zeros((10, 32))[:, ::2]):
        with pytest.raises(et.ArgumentError):
            opt.set_state(A, m, bad)
    with pytest.raises(et.ArgumentError):
        et.Adam(beta=(0.9, 1.0))
    for kw in ({"exact": True}, {"exact": False}, {"split": True}, {"hot_pass": True},
               {"indexers": [None]}):
        with pytest.raises(et.ArgumentError, match=next(iter(kw))):
            et.update_(opt, [A], [g], **kw)
    weighted = et.SparseEmbeddingUpdate(A.lookup_type, g.delta, g.indices, torch.ones(8))
    with pytest.raises(et.ArgumentError, match="weighted"):
        et.update_(opt, A, weighted)
    with pytest.raises(et.ArgumentError, match="SGD-only"):
        et.PhasedUpdate([], []).update_(opt)
