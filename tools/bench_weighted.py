"""Weighted and mean-pooled bags on bench.py's tables, timed with HIP events.

One process, the launches alternated inside every repeat, on the config-3 tables (26 Criteo
tables x 128 fp32, B = 65,536) with bag lengths uniform on 0..40 (case (b) of
tools/bench_ragged.py):

  forward   the ragged unweighted launch (et_ragged_maplookup_prealloc), the weighted launch
            on the same indices, the mean launch, and the weight-gradient launch
            (et_weighted_weight_grad, all tables in one call);
  update    et_weighted_sgd against et_ragged_sgd on the same uniform indices.

Every timing is the average of `--steps` launches, repeated `--repeats` times (min / median /
max: the spread of this box).  Writes profiles/weighted/bench_weighted.json.

    python tools/bench_weighted.py [--steps 20] [--warmup 5] [--repeats 5] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "embeddingtables.jl_amd"))
import bench  # noqa: E402


def alternated(cases, steps, warmup, repeats, stream):
    """{name: spread} with the cases timed one after another inside every repeat."""
    ms = {name: [] for name in cases}
    for r in range(repeats):
        for name, fn in cases.items():
            ms[name].append(bench._timed(fn, steps, warmup if r == 0 else 1, stream))
    return {name: {"min_ms": min(v), "median_ms": statistics.median(v), "max_ms": max(v),
                   "repeats": v} for name, v in ms.items()}


def main():
    import torch

    import embtab as et
    from embtab import _lib
    from embtab.weighted import weighted_update_desc

    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--update-steps", type=int, default=3)
    p.add_argument("--batch", type=int, default=bench.BATCH)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "weighted",
                                                 "bench_weighted.json"))
    a = p.parse_args()

    dev = torch.device("cuda", 0)
    L = _lib.load()
    B, D = a.batch, bench.DIM
    tids = list(range(len(bench.CRITEO_KAGGLE_ROWS)))
    rows = [bench.CRITEO_KAGGLE_ROWS[t] for t in tids]
    tables = bench.make_tables(et, L, tids, dev)
    stream = torch.cuda.current_stream(dev)
    strat = et.PreallocationStrategy(0)
    dst = torch.empty((B, D * len(tables)), dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20)

    Rs, Ws, Ms, dws = [], [], [], []
    for t in tids:
        l = torch.randint(0, 41, (B,), generator=gen, device=dev)
        v = torch.empty(int(l.sum()), dtype=torch.int64, device=dev)
        _lib.check(L.et_fill_index_uniform(v.data_ptr(), v.numel(), rows[t],
                                           bench.INDEX_SEED + 100 + t, 0, stream.cuda_stream))
        R = et.RaggedIndices.from_lengths(v, l, check=True)
        w = torch.empty(v.numel(), dtype=torch.float32, device=dev)
        _lib.check(L.et_fill_uniform(_lib.ET_F32, w.data_ptr(), w.numel(), 7000 + t, 0, -1.0, 1.0,
                                     stream.cuda_stream))
        Rs.append(R)
        Ws.append(et.WeightedIndices(R, w))
        Ms.append(et.WeightedIndices(R, mode="mean"))
        dws.append(torch.empty_like(w))
    entries = int(sum(R.nnz for R in Rs))
    delta = torch.empty_like(dst)
    _lib.check(L.et_fill_uniform(_lib.ET_F32, delta.data_ptr(), delta.numel(), 4001, 0, -1.0, 1.0,
                                 stream.cuda_stream))
    blocks = [delta[:, k * D:(k + 1) * D] for k in range(len(tables))]

    gd = (_lib.WeightedUpdateDesc * len(tables))(*[
        weighted_update_desc(A, d, R, None, dw) for A, d, R, dw in zip(tables, blocks, Rs, dws)])

    def weight_grad_all():
        _lib.check(L.et_weighted_weight_grad(_lib.ET_F32, ctypes.addressof(gd), len(tables),
                                             stream.cuda_stream))

    out = {"workload": f"{len(tables)} Criteo tables x {D} fp32, B = {B}, lengths uniform 0..40",
           "entries": entries, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    out["forward"] = alternated({
        "ragged_unweighted": et.PreallocationPlan(strat, dst, tables, Rs),
        "weighted": et.PreallocationPlan(strat, dst, tables, Ws),
        "mean": et.PreallocationPlan(strat, dst, tables, Ms),
        "weight_grad": weight_grad_all,
    }, a.steps, a.warmup, a.repeats, stream)
    for r in out["forward"].values():
        r["ns_per_entry"] = 1e6 * r["median_ms"] / max(entries, 1)
    # by bytes: an entry moves its 512-byte row and its 8-byte index; the weight adds 4, the
    # weight gradient writes 4 more
    out["bytes_per_entry"] = {"ragged_unweighted": 520, "weighted": 524, "weight_grad": 524}
    assert et.check_errors() == 0

    opt = et.Descent(0.1)
    rgrads = [et.SparseEmbeddingUpdate(A.lookup_type, d, R) for A, d, R in zip(tables, blocks, Rs)]
    wgrads = [et.SparseEmbeddingUpdate(A.lookup_type, d, R, W.weights)
              for A, d, R, W in zip(tables, blocks, Rs, Ws)]
    out["update"] = alternated({
        "ragged_sgd": lambda: et.update_(opt, tables, rgrads),
        "weighted_sgd": lambda: et.update_(opt, tables, wgrads),
    }, a.update_steps, 1, min(a.repeats, 3), stream)
    assert et.check_errors() == 0

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: {kk: vv["median_ms"] for kk, vv in out[k].items()}
                      for k in ("forward", "update")}))


if __name__ == "__main__":
    main()
