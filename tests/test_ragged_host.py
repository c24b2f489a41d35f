"""Variable-length bags, the parts that need no GPU: RaggedIndices on CPU tensors, the
argument errors of the et_ragged_* entry points (status codes before any device work), the
workspace size, and the ctypes mirrors of the two new descriptor structs."""
import ctypes
import os
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_from_lengths_on_cpu_tensors():
    import embtab as et

    v = torch.arange(1, 8, dtype=torch.int64)
    R = et.RaggedIndices.from_lengths(v, [0, 3, 0, 2, 1, 0])
    assert R.colptr.tolist() == [1, 1, 4, 4, 6, 7, 7]
    assert R.colptr.dtype == torch.int64
    assert R.batch == 6 and R.nnz == 7  # nnz is the capacity, not colptr[B] - 1
    assert R.values is v
    assert R.lengths().tolist() == [0, 3, 0, 2, 1, 0]
    # lengths as a tensor; every bag empty; no bag at all
    R = et.RaggedIndices.from_lengths(v, torch.tensor([2, 5]))
    assert R.colptr.tolist() == [1, 3, 8] and R.batch == 2
    R = et.RaggedIndices.from_lengths(v[:0], [0, 0, 0])
    assert R.colptr.tolist() == [1, 1, 1, 1] and R.batch == 3 and R.nnz == 0
    R = et.RaggedIndices.from_lengths(v[:0], [])
    assert R.colptr.tolist() == [1] and R.batch == 0
    assert et.RaggedIndices.from_lengths(v, [3, 4], check=True).batch == 2


def test_constructor_rejections():
    import embtab as et

    v = torch.arange(1, 5, dtype=torch.int64)
    c = torch.tensor([1, 3, 5], dtype=torch.int64)
    assert et.RaggedIndices(v, c).batch == 2
    with pytest.raises(TypeError):
        et.RaggedIndices(v.to(torch.int32), c)
    with pytest.raises(TypeError):
        et.RaggedIndices(v, c.to(torch.int32))
    with pytest.raises(TypeError):
        et.RaggedIndices(v.tolist(), c)
    with pytest.raises(et.ArgumentError):
        et.RaggedIndices(v.reshape(2, 2), c)
    with pytest.raises(et.ArgumentError):
        et.RaggedIndices(v, c.reshape(1, 3))
    with pytest.raises(et.ArgumentError):
        et.RaggedIndices(torch.arange(1, 9, dtype=torch.int64)[::2], c)  # strided values
    with pytest.raises(et.ArgumentError):
        et.RaggedIndices(v, c[:0])  # colptr needs B + 1 >= 1 entries
    with pytest.raises(et.ArgumentError):
        et.RaggedIndices(v, c.to("meta"))  # device mix
    # check=True: monotonicity, range of colptr, range of the values
    for bad in ([1, 4, 3], [0, 2, 5], [1, 3, 6]):
        with pytest.raises(et.ArgumentError):
            et.RaggedIndices(v, torch.tensor(bad, dtype=torch.int64), check=True)
    with pytest.raises(et.ArgumentError):
        et.RaggedIndices(v, c, check=True, maxindex=3)
    assert et.RaggedIndices(v, c, check=True, maxindex=4).nnz == 4
    # lookups refuse host indices, as for plain tensors
    from embtab.lookup import _check_idx

    with pytest.raises(et.ArgumentError):
        _check_idx(et.RaggedIndices(v, c))


def _desc(L, **kw):
    d = dict(table=1 << 20, ld_table=16, nrows=100, dim=16, reserved=0, idx=1 << 21, nnz=64,
             colptr=1 << 22, dst_row_off=0, cols_per_page=0)
    d.update(kw)
    arr = (L.RaggedDesc * 1)()
    arr[0] = L.RaggedDesc(*[d[f[0]] for f in L.RaggedDesc._fields_])
    return arr


def _udesc(L, **kw):
    d = dict(table=1 << 20, ld_table=16, nrows=100, dim=16, reserved=0, delta=1 << 23,
             ld_delta=16, idx=1 << 21, nnz=64, colptr=1 << 22, batch=8, cols_per_page=0)
    d.update(kw)
    arr = (L.RaggedUpdateDesc * 1)()
    arr[0] = L.RaggedUpdateDesc(*[d[f[0]] for f in L.RaggedUpdateDesc._fields_])
    return arr


def test_lookup_argument_errors_need_no_gpu():
    from embtab import _lib

    L = _lib.load()
    f = L.et_ragged_maplookup_prealloc
    dst = 1 << 24  # never dereferenced: every call below stops at the host checks
    a = ctypes.addressof
    # ld_dst < dst_row_off + dim
    assert f(_lib.ET_F32, a(_desc(_lib, dst_row_off=4)), 1, 8, dst, 16, 0, None) == -1
    assert b"ld_dst" in L.et_last_error()
    # unknown dtype
    assert f(99, a(_desc(_lib)), 1, 8, dst, 16, 0, None) == -4
    # negative sizes
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
    # too many tables for one launch
    big = (_lib.RaggedDesc * 33)()
    assert f(_lib.ET_F32, a(big), 33, 8, dst, 16, 0, None) == -1
    # batch == 0 (and no table) is a no-op success
    assert f(_lib.ET_F32, a(_desc(_lib)), 1, 0, None, 16, 0, None) == 0
    assert f(_lib.ET_F32, None, 0, 8, None, 16, 0, None) == 0


def test_bag_ids_argument_errors_need_no_gpu():
    from embtab import _lib

    L = _lib.load()
    assert L.et_ragged_bag_ids(1 << 20, -1, 8, 1 << 21, None) == -1
    assert L.et_ragged_bag_ids(1 << 20, 4, -8, 1 << 21, None) == -1
    assert L.et_ragged_bag_ids(1 << 20, 4, 8, None, None) == -1
    assert L.et_ragged_bag_ids(None, 4, 8, 1 << 21, None) == -1
    assert L.et_ragged_bag_ids(None, 0, 0, None, None) == 0  # nothing to write


def test_update_argument_errors_need_no_gpu():
    from embtab import _lib

    L = _lib.load()
    f = L.et_ragged_sgd
    a = ctypes.addressof
    assert f(_lib.ET_I32, a(_udesc(_lib)), 1, 0.1, 0, None, 0, None) == -4
    assert f(99, a(_udesc(_lib)), 1, 0.1, 0, None, 0, None) == -4
    for flag in (_lib.ET_FLAG_SGD_INDEX_ONLY, _lib.ET_FLAG_SGD_APPLY_ONLY,
                 _lib.ET_FLAG_SGD_HOT_PASS):
        assert f(_lib.ET_F32, a(_udesc(_lib)), 1, 0.1, flag, None, 0, None) == -4
    assert f(_lib.ET_F32, a(_udesc(_lib, nnz=-1)), 1, 0.1, 0, None, 0, None) == -1
    assert f(_lib.ET_F32, a(_udesc(_lib, batch=-1)), 1, 0.1, 0, None, 0, None) == -1
    assert f(_lib.ET_F32, a(_udesc(_lib, ld_delta=8)), 1, 0.1, 0, None, 0, None) == -1
    assert f(_lib.ET_F32, a(_udesc(_lib, delta=0)), 1, 0.1, 0, None, 0, None) == -1
    assert f(_lib.ET_F32, a(_udesc(_lib, colptr=0)), 1, 0.1, 0, None, 0, None) == -1
    assert f(_lib.ET_F32, None, 1, 0.1, 0, None, 0, None) == -1
    big = (_lib.RaggedUpdateDesc * 33)()
    assert f(_lib.ET_F32, a(big), 33, 0.1, 0, None, 0, None) == -1
    # valid descriptors stop at the missing workspace, before any device work
    for exact in (0, _lib.ET_FLAG_EXACT_UPDATE, _lib.ET_FLAG_EXACT_IF_FAST):
        assert f(_lib.ET_F32, a(_udesc(_lib)), 1, 0.1, exact, None, 0, None) == -3
    # nothing to do: no bags, no entries, no tables
    assert f(_lib.ET_F32, a(_udesc(_lib, batch=0)), 1, 0.1, 0, None, 0, None) == 0
    assert f(_lib.ET_F32, a(_udesc(_lib, nnz=0)), 1, 0.1, 0, None, 0, None) == 0
    assert f(_lib.ET_F32, None, 0, 0.1, 0, None, 0, None) == 0


def test_workspace_size_grows_with_nnz():
    from embtab import _lib

    L = _lib.load()
    sizes = []
    for nnz in (0, 1000, 100000, 10000000):
        nb = ctypes.c_int64(-1)
        assert L.et_ragged_sgd_workspace_size(ctypes.addressof(_udesc(_lib, nnz=nnz)), 1,
                                              ctypes.byref(nb)) == 0
        sizes.append(nb.value)
    assert sizes[0] > 0 and sizes == sorted(set(sizes))
    # at least the sort's key / value pairs and the bag ids: 5 words per entry
    assert sizes[3] - sizes[0] >= 10000000 * 20
    nb = ctypes.c_int64(0)
    big = (_lib.RaggedUpdateDesc * 33)()
    assert L.et_ragged_sgd_workspace_size(ctypes.addressof(big), 33, ctypes.byref(nb)) == -1
    assert L.et_ragged_sgd_workspace_size(ctypes.addressof(_udesc(_lib)), 1, None) == -1
    assert L.et_ragged_sgd_workspace_size(ctypes.addressof(_udesc(_lib, nnz=1 << 31)), 1,
                                          ctypes.byref(nb)) == -1


def test_ragged_struct_layouts_match_header(tmp_path):
    from embtab import _lib

    structs = (("et_ragged_desc", _lib.RaggedDesc), ("et_ragged_update_desc",
                                                     _lib.RaggedUpdateDesc))
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
