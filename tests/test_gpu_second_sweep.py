"""Every grid-stride loop of the ragged, weighted and AdaGrad update kernels taken at least
twice: one test per launch threshold, at the smallest shape that crosses it.

The grids are capped, so a loop's second iteration runs only above a size no targeted file
reaches.  The thresholds, from the launch code (``n`` is the call's occurrences, ``GPW`` the
lane groups per wave: 64 / (D / 4) for a capacity D < 256, else 1):

=====  ==================================  ==============================  ===========================
test   kernel                              one sweep covers                source
=====  ==================================  ==============================  ===========================
1a     k_ragged_bag_ids                    16,384 x 16 = 262,144 bags      et_ragged_update.hip:33-34,
                                                                           47-48
1b     k_ragged_apply                      16,384 x 4 = 65,536 distinct    et_ragged_update.hip:66,
                                           columns                         256-257
1b     k_weighted_apply                    the same                        et_weighted_update.hip:30,
                                                                           204-205
1c     k_adagrad_chunks<D>,                sgd_grid(n) x 4 x GPW chunk     et_adagrad.hip:200-201, 657;
       k_weighted_adagrad_chunks<D>        records; sgd_grid(n) = 256 up   et_weighted_adagrad.hip:108,
                                           to n = 524,288: 16,384 at       253; et_update.hip:3135-3138
                                           capacity 16, 2,048 at 128,
                                           1,024 from 256 on
1c     k_adagrad_chunks_generic,           sgd_grid(n) x 4 = 1,024 chunk   et_adagrad.hip:390-391;
       k_weighted_adagrad_chunks_generic   records                         et_weighted_adagrad.hip:168
1d     k_adagrad_combine<D>                min(cdiv(n / 256 + 2, 4 GPW),   et_adagrad.hip:267-268,
                                           2,048) x 4 x GPW multi-chunk    666-671
                                           columns: 8,192 at capacity 256
=====  ==================================  ==============================  ===========================

tests/sweep_cases.py restates these on the host; before it launches, every test asserts with
those predicates that its inputs cross the threshold (tests/test_family_sweep_host.py asserts
the same without a GPU), so a later edit of a shape cannot hollow a test out.

References are the families' own: the C oracle's ``sgd`` on the expanded gradient,
``weighted_ref.sgd``, tests/test_gpu_adagrad.py's ``ref_step`` / ``rowwise_bounds`` and
``weighted_adagrad_ref``.  Comparisons are byte equality except the row-wise AdaGrad state,
which keeps its derived bound.  1d's 2.1 M entries are beyond the per-occurrence ``ref_step``:
its reference is ``sweep_cases.equal_count_step``, the same additions in the same order for
all columns at once, shown equal to ``ref_step`` bit for bit on the CPU.

The generic twin of 1d (16,384 columns x 257 entries at dim 7, 4.2 M entries) is left out:
its values and sort workspace alone take about 120 MB of device memory."""
import numpy as np
import pytest

import embtab as et
import sweep_cases as sc
import test_gpu_adagrad as ta
import weighted_adagrad_ref as war
import weighted_ref as wr
from embtab.tables import Dynamic, Static, fused_update_path
from test_gpu_ragged import dev, host, same

pytestmark = pytest.mark.gpu
ETA, EPS = ta.ETA, ta.EPS
F32 = ta.KINDS["f32"]


def ragged(c, key="values"):
    return et.RaggedIndices(dev(c[key]), dev(c["colptr"]))


def test_thresholds_use_the_library_chunk():
    assert sc.CHUNK == et._lib.ET_SGD_CHUNK


# --- 1a. bag ids past 262,144 bags ----------------------------------------------------------------

@pytest.fixture(scope="module")
def bags():
    return sc.bag_ids_case()


def sgd_expected(oracle, c, fused):
    ref = c["table"].copy()
    oracle.sgd(ref, c["delta"][c["bag"]], c["values"][:c["used"]], 0.1, fused=fused)
    return ref


@pytest.mark.parametrize("static", [True, False])
def test_bag_ids_ragged_sgd(oracle, bags, static):
    c = bags
    assert sc.crosses_bag_ids(c["colptr"])
    lt = Static(c["D"]) if static else Dynamic
    A = et.SimpleEmbedding(dev(c["table"]), lt)
    et.update_(et.Descent(0.1), A, et.SparseEmbeddingUpdate(lt, dev(c["delta"]), ragged(c)))
    assert fused_update_path(A) == static
    assert same(host(A.data), sgd_expected(oracle, c, static))
    assert et.check_errors() == 0


def test_bag_ids_weighted_sgd(bags):
    c = bags
    assert sc.crosses_bag_ids(c["colptr"])
    lt = Static(c["D"])
    A = et.SimpleEmbedding(dev(c["table"]), lt)
    et.update_(et.Descent(0.1), A, et.SparseEmbeddingUpdate(lt, dev(c["delta"]), ragged(c),
                                                           dev(c["weights"])))
    ref = wr.sgd(c["table"].copy(), c["delta"], c["values"], c["colptr"], c["weights"], 0.1,
                 fused=fused_update_path(A))
    assert same(host(A.data), ref) and np.isfinite(ref).all()
    assert et.check_errors() == 0


def test_bag_ids_ragged_adagrad(bags):
    c = bags
    assert sc.crosses_bag_ids(c["colptr"])
    assert sc.multi_chunk_columns(c["values"], c["R"]) == c["R"]  # every column is multi-chunk
    A = et.SimpleEmbedding(dev(c["table"]))
    opt = et.AdaGrad(ETA, EPS)
    opt.state(A).copy_(dev(c["state"]))
    et.update_(opt, A, et.SparseEmbeddingUpdate(A.lookup_type, dev(c["delta"]), ragged(c)))
    table, state = c["table"].copy(), c["state"].copy()
    ta.ref_step(F32, table, state, c["delta"], ta.lists_ragged(c["values"], c["colptr"],
                                                              nrows=c["R"]))
    assert same(host(A.data), table) and same(host(opt.state(A)), state)
    assert et.check_errors() == 0


def test_bag_ids_weighted_adagrad(bags):
    c = bags
    assert sc.crosses_bag_ids(c["colptr"])
    A = et.SimpleEmbedding(dev(c["table"]))
    opt = et.AdaGrad(ETA, EPS, weighted=True)
    opt.state(A).copy_(dev(c["state"]))
    et.update_(opt, A, et.SparseEmbeddingUpdate(A.lookup_type, dev(c["delta"]), ragged(c),
                                                dev(c["weights"])))
    table, state = c["table"].copy(), c["state"].copy()
    war.ref_step(F32, table, state, c["delta"], c["values"], c["colptr"], c["weights"],
                 nrows=c["R"])
    assert same(host(A.data), table) and same(host(opt.state(A)), state)
    assert et.check_errors() == 0


@pytest.mark.parametrize("big_first", [True, False])
def test_bag_ids_two_tables_of_different_batch(oracle, bags, big_first):
    """`max_batch` sizes the grid and each table has its own `batch` bound: the long table
    beside a 301-bag one in one call, in both orders, each against its single-table
    reference."""
    cases = [bags, sc.small_ragged_case()]
    assert sc.crosses_bag_ids(bags["colptr"]) and cases[1]["B"] == 301
    if not big_first:
        cases.reverse()
    lt = Static(16)
    As = [et.SimpleEmbedding(dev(c["table"]), lt) for c in cases]
    grads = [et.SparseEmbeddingUpdate(lt, dev(c["delta"]), ragged(c)) for c in cases]
    et.update_(et.Descent(0.1), As, grads)
    for A, c in zip(As, cases):
        assert same(host(A.data), sgd_expected(oracle, c, True)), c["B"]
    assert et.check_errors() == 0


# --- 1b. apply kernels past 65,536 distinct columns ------------------------------------------------

@pytest.fixture(scope="module")
def wide():
    return sc.apply_case()


def second_sweep_changed(c, got):
    """All R columns are touched, in increasing order: a column of the second sweep."""
    rows = np.arange(sc.APPLY_COLUMNS, c["R"])
    return not (got[rows] == c["table"][rows]).all(axis=1).any()


def test_apply_ragged_sgd(oracle, wide):
    c = wide
    assert sc.crosses_apply(c["values"], c["R"])
    lt = Static(c["D"])
    A = et.SimpleEmbedding(dev(c["table"]), lt)
    et.update_(et.Descent(0.1), A, et.SparseEmbeddingUpdate(lt, dev(c["delta"]), ragged(c)))
    got = host(A.data)
    assert same(got, sgd_expected(oracle, c, fused_update_path(A)))
    assert second_sweep_changed(c, got)
    assert et.check_errors() == 0


def test_apply_weighted_sgd(oracle, wide):
    """The reference of tests/test_gpu_weighted.py for Float32: the C oracle on the expanded
    gradient E[k] = w_k * delta[bag(k)].  ``weighted_ref.sgd``, which 1a uses, searches the
    values once per column: 70,000 searches here."""
    c = wide
    assert sc.crosses_apply(c["values"], c["R"])
    lt = Static(c["D"])
    A = et.SimpleEmbedding(dev(c["table"]), lt)
    et.update_(et.Descent(0.1), A, et.SparseEmbeddingUpdate(lt, dev(c["delta"]), ragged(c),
                                                           dev(c["weights"])))
    got = host(A.data)
    E, cov = wr.expanded_gradient(c["delta"], c["weights"], c["colptr"], len(c["values"]))
    assert cov.all()
    ref = c["table"].copy()
    oracle.sgd(ref, E, c["values"], 0.1, fused=fused_update_path(A))
    assert same(got, ref)
    assert second_sweep_changed(c, got)
    assert et.check_errors() == 0


# --- 1c. the AdaGrad chunk pass past its lane groups ----------------------------------------------

def run_adagrad(c, form, rowwise, weighted=False):
    """One AdaGrad step of chunk case `c` on the device: (table, state) as written."""
    kind = sc.kind_of(c["kind"])
    A = et.SimpleEmbedding(kind.dev(c["table"]))
    opt = et.AdaGrad(ETA, EPS, rowwise=rowwise, weighted=weighted)
    opt.state(A).copy_(dev(c["state_row"] if rowwise else c["state"]))
    if form == "fixed":
        g = et.SparseEmbeddingUpdate(A.lookup_type, kind.dev(c["delta"]), dev(c["I"]))
    else:
        g = et.SparseEmbeddingUpdate(A.lookup_type, kind.dev(c["delta_ragged"]), ragged(c),
                                     dev(c["weights"]) if weighted else None)
    et.update_(opt, A, g)
    assert et.check_errors() == 0
    return host(A.data), host(opt.state(A))


def check_adagrad(c, got, delta, lists, rowwise, g_of=None):
    kind = sc.kind_of(c["kind"])
    got_t, got_s = got
    last = c["R"] - 40 - 1  # 0-based: the last 50 touched columns moved
    assert not same(got_t[last - 50:last], c["table"][last - 50:last])
    if rowwise:
        if g_of is None:
            rs, rw = ta.rowwise_bounds(kind, c["table"], c["state_row"], delta, lists, got_t,
                                       got_s)
        else:
            rs, rw = war.rowwise_bounds(kind, c["table"], c["state_row"], g_of, got_t, got_s)
        print(f"rowwise GPU ratio {c['name']}: state {rs:.3f} table {rw:.3f}")
        assert rs <= 1.0 and rw <= 1.0, (rs, rw)
        return
    table, state = c["table"].copy(), c["state"].copy()
    ta.ref_step(kind, table, state, delta, lists, g_of=g_of)
    assert same(got_t, table) and same(got_s, state)


@pytest.mark.parametrize("rowwise", [False, True])
@pytest.mark.parametrize("name", sorted(sc.CHUNK_CASES))
def test_chunks_fixed_pool(name, rowwise):
    c = sc.chunk_case(name)
    assert sc.crosses_chunks(c["I"], c["R"], c["cap"])
    check_adagrad(c, run_adagrad(c, "fixed", rowwise), c["delta"],
                  ta.lists_fixed(c["I"], nrows=c["R"]), rowwise)


@pytest.mark.parametrize("rowwise", [False, True])
@pytest.mark.parametrize("name", sorted(sc.CHUNK_CASES))
def test_chunks_ragged(name, rowwise):
    c = sc.chunk_case(name)
    assert sc.crosses_chunks(c["values"], c["R"], c["cap"])
    check_adagrad(c, run_adagrad(c, "ragged", rowwise), c["delta_ragged"],
                  ta.lists_ragged(c["values"], c["colptr"], nrows=c["R"]), rowwise)


@pytest.mark.parametrize("rowwise", [False, True])
@pytest.mark.parametrize("name", sc.CHUNK_WEIGHTED)
def test_chunks_weighted(name, rowwise):
    c = sc.chunk_case(name)
    assert sc.crosses_chunks(c["values"], c["R"], c["cap"])
    lists, g_of = war.reference_inputs(sc.kind_of(c["kind"]), c["delta_ragged"], c["values"],
                                       c["colptr"], c["weights"], nrows=c["R"])
    check_adagrad(c, run_adagrad(c, "ragged", rowwise, weighted=True), c["delta_ragged"], lists,
                  rowwise, g_of=g_of)


# --- 1d. the AdaGrad combine pass past 8,192 multi-chunk columns ----------------------------------

def test_combine_past_one_sweep():
    c = sc.combine_case()
    assert sc.crosses_combine(c["values"], c["R"], sc.capacity(c["D"]))
    A = et.SimpleEmbedding(dev(c["table"]))
    opt = et.AdaGrad(ETA, EPS)
    opt.state(A).copy_(dev(c["state"]))
    et.update_(opt, A, et.SparseEmbeddingUpdate(A.lookup_type, dev(c["delta"]), ragged(c)))
    got_t, got_s = host(A.data), host(opt.state(A))
    table, state = c["table"].copy(), c["state"].copy()
    sc.equal_count_step(F32, table, state, c["delta"], c["values"], c["colptr"])
    assert same(got_t, table) and same(got_s, state)
    touched = np.unique(c["values"]) - 1
    assert not (got_t[touched[8192:]] == c["table"][touched[8192:]]).all(axis=1).any()
    assert et.check_errors() == 0
