"""et.interact / its pullback against the same computation in Float64 on the CPU: the batched
``Xv @ Xv.T``, the triangle gather, ``cat``, and torch autograd for the backward."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
U = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
DIMS = {torch.float32: (4, 8, 36, 128), torch.float16: (8, 24, 40, 128),
        torch.bfloat16: (8, 24, 40, 128)}


def reference(X64, dim, copy, itself, dY64=None):
    """(Y, dX) in Float64 on the CPU; dX is None without dY64."""
    X64 = X64.clone().requires_grad_(dY64 is not None)
    B, F = X64.shape[0], X64.shape[1] // dim
    Xv = X64.view(B, F, dim)
    Z = Xv @ Xv.transpose(1, 2)
    li, lj = torch.tril_indices(F, F, 0 if itself else -1)
    Y = torch.cat([X64[:, :copy], Z[:, li, lj]], 1)
    if dY64 is None:
        return Y, None
    Y.backward(dY64)
    return Y.detach(), X64.grad


def eighths(shape, gen):
    return torch.randint(-4, 5, shape, generator=gen).double() / 8


def same(got, ref64, dtype):
    """Float32 / Float16: the Float64 value itself; BFloat16: its one RNE rounding."""
    got = got.cpu()
    return torch.equal(got, ref64.to(dtype)) and (dtype == torch.bfloat16 or
                                                  torch.equal(got.double(), ref64))


def run_exact(et, dtype, B, F, dim, copy, itself, seed):
    gen = torch.Generator().manual_seed(seed)
    NP = F * (F + 1) // 2 if itself else F * (F - 1) // 2
    X64, dY64 = eighths((B, F * dim), gen), eighths((B, copy + NP), gen)
    Yr, dXr = reference(X64, dim, copy, itself, dY64)
    Y, back = et.rrule(et.interact, X64.to(dtype).cuda(), dim, copy, itself)
    tang = back(dY64.to(dtype).cuda())
    assert same(Y, Yr, dtype), (dtype, B, F, dim, copy, itself)
    assert same(tang[1], dXr, dtype), (dtype, B, F, dim, copy, itself)
    assert len(tang) == 5 and all(isinstance(t, et.NoTangent) for t in tang[:1] + tang[2:])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F", [1, 2, 3, 27, 32])
@pytest.mark.parametrize("di", range(4))
def test_exact_every_shape(dtype, F, di):
    import embtab as et

    run_exact(et, dtype, 7, F, DIMS[dtype][di], DIMS[dtype][di], False, 100 * F + di)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("itself", [False, True])
@pytest.mark.parametrize("copy_of", [lambda F, D: 0, lambda F, D: D, lambda F, D: F * D])
@pytest.mark.parametrize("B", [1, 7])
def test_exact_every_mode(dtype, itself, copy_of, B):
    import embtab as et

    for F, dim in ((2, DIMS[dtype][2]), (27, DIMS[dtype][3]), (32, DIMS[dtype][1])):
        run_exact(et, dtype, B, F, dim, copy_of(F, dim), itself, 7 * F + B)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("itself", [False, True])
def test_views_inside_nan_buffers(dtype, itself):
    """X, Y, dY and dX are views (ld > width) inside NaN-filled buffers: the results are exact
    and no cell outside the views changes, so no tile row or K tail comes from behind a row."""
    import embtab as et
    from embtab import _lib

    B, F, dim = 5, 27, DIMS[dtype][2]
    copy, NP, W = dim, F * (F + 1) // 2 if itself else F * (F - 1) // 2, F * dim
    gen = torch.Generator().manual_seed(5)
    X64, dY64 = eighths((B, W), gen), eighths((B, copy + NP), gen)
    Yr, dXr = reference(X64, dim, copy, itself, dY64)
    a = 16 // X64.to(dtype).element_size()  # elements in 16 bytes: the alignment X and dX need
    bufs, views = [], []
    for width, off, pad in ((W, a, 2 * a), (copy + NP, 3, 5), (copy + NP, 1, 2), (W, 2 * a, a)):
        buf = torch.full((B + 2, off + width + pad), float("nan"), dtype=dtype, device="cuda")
        bufs.append(buf)
        views.append(buf[1:B + 1, off:off + width])
    Xd, Yd, dYd, dXd = views
    Xd.copy_(X64.to(dtype))
    dYd.copy_(dY64.to(dtype))
    assert et.interact_(Yd, Xd, dim, copy, itself) is Yd
    flags = _lib.ET_FLAG_INTERACT_ITSELF if itself else 0
    _lib.check(_lib.load().et_interact_backward(
        _lib.et_dtype(Xd), Xd.data_ptr(), Xd.stride(0), dYd.data_ptr(), dYd.stride(0), B, F, dim,
        copy, dXd.data_ptr(), dXd.stride(0), flags, _lib.stream_handle(Xd.device)))
    assert same(Yd, Yr, dtype) and same(dXd, dXr, dtype)
    assert same(Xd, X64, dtype) and same(dYd, dY64, dtype)
    for buf, view in zip(bufs, views):
        view.fill_(float("nan"))
        assert bool(torch.isnan(buf).all())


def normal_case(dtype, B, F, dim, itself, seed):
    gen = torch.Generator().manual_seed(seed)
    NP = F * (F + 1) // 2 if itself else F * (F - 1) // 2
    return (torch.randn((B, F * dim), generator=gen).to(dtype),
            torch.randn((B, dim + NP), generator=gen).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_invariance(dtype):
    """A sample's bits do not depend on the batch it sits in, nor on the grid sweep."""
    import embtab as et
    from embtab import _lib

    X, dY = (t.cuda() for t in normal_case(dtype, 7, 27, 128, False, 11))
    Y, back = et.rrule(et.interact, X, 128)
    dX = back(dY)[1]
    for b in range(7):
        y1, back1 = et.rrule(et.interact, X[b:b + 1], 128)
        assert torch.equal(y1.view(torch.int16), Y[b:b + 1].view(torch.int16))
        assert torch.equal(back1(dY[b:b + 1])[1].view(torch.int16), dX[b:b + 1].view(torch.int16))
    cap = _lib.ET_INTERACT_GRID_CAP * _lib.ET_INTERACT_WAVES  # samples in one grid sweep
    Xs, dYs = (t.cuda() for t in normal_case(dtype, cap, 3, 8, True, 12))
    rows = torch.arange(3 * cap + 1, device="cuda") % cap
    Y, back = et.rrule(et.interact, Xs[rows], 8, 8, True)
    dX = back(dYs[rows])[1]
    assert torch.equal(Y.view(torch.int16), Y[:cap][rows].view(torch.int16))
    assert torch.equal(dX.view(torch.int16), dX[:cap][rows].view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F,dim,itself", [(27, 128, False), (32, 40, True)])
def test_rounding_bound(dtype, F, dim, itself):
    """The any-order Float32 summation bound with truncation's unit roundoff (2^-23), plus the
    one rounding to T: |Y - ref| <= 1.01 D 2^-23 sum|x_i x_j| (1 + u) + u |ref|; the backward
    with F + 2 terms and sum_j |G[i,j] x_j[n]| + |dY| on the copied columns."""
    import embtab as et

    X, dY = normal_case(dtype, 4, F, dim, itself, 21)
    Yr, dXr = reference(X.double(), dim, dim, itself, dY.double())
    Ya, dXa = reference(X.double().abs(), dim, dim, itself, dY.double().abs())
    Y, back = et.rrule(et.interact, X.cuda(), dim, dim, itself)
    dX = back(dY.cuda())[1]
    u = U[dtype]
    Ya[:, :dim] = 0  # the copied columns are a bit copy
    for got, ref, mag, n in ((Y, Yr, Ya, dim), (dX, dXr, dXa, F + 2)):
        err = (got.cpu().double() - ref).abs()
        bound = 1.01 * n * 2.0 ** -23 * mag * (1 + u) + u * ref.abs()
        print(dtype, F, dim, "max err / bound", float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("itself", [False, True])
def test_nan_stays_in_its_pairs(dtype, itself):
    import embtab as et

    B, F, dim = 3, 5, DIMS[dtype][1]
    X64 = eighths((B, F * dim), torch.Generator().manual_seed(3))
    X64[1, 2 * dim + 3] = float("nan")  # vector 2 of sample 1
    Yr, _ = reference(X64, dim, dim, itself)
    Y = et.interact(X64.to(dtype).cuda(), dim, dim, itself).cpu()
    assert int(torch.isnan(Yr).sum()) == F - 1 + itself
    assert torch.equal(torch.isnan(Y), torch.isnan(Yr))
    assert same(torch.nan_to_num(Y, 77.0), torch.nan_to_num(Yr, 77.0), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_capture_replays(dtype):
    """Forward + backward captured on one stream; every replay after refilling X and dY in
    place equals the eager result."""
    import embtab as et

    cases = [normal_case(dtype, 9, 27, 128, False, 30 + k) for k in range(3)]
    X, dY = (t.clone().cuda() for t in cases[0])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        et.interact(X, 128)  # the library's first call outside the capture
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            Y, back = et.rrule(et.interact, X, 128)
            dX = back(dY)[1]
    for Xh, dYh in cases[::-1]:
        X.copy_(Xh)
        dY.copy_(dYh)
        graph.replay()
        torch.cuda.synchronize()
        Ye, backe = et.rrule(et.interact, Xh.cuda(), 128)
        assert torch.equal(Y.view(torch.int16), Ye.view(torch.int16))
        assert torch.equal(dX.view(torch.int16), backe(dYh.cuda())[1].view(torch.int16))
