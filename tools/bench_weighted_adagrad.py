"""Sparse AdaGrad over weighted and mean-pooled gradients on bench.py's tables, timed with HIP
events.

One process, the launches alternated inside every repeat, on the config-3 tables (26 Criteo
tables x 128 fp32, B = 65,536) with bag lengths uniform on 0..40 (the workload of
tools/bench_weighted.py), indices uniform and Zipf(1.05):

  weighted          et_weighted_adagrad, element-wise, weights uniform on [-1, 1)
  weighted_rowwise  the same, row-wise
  mean              et_weighted_adagrad with the mean-mode weights 1 / len(bag)
  unweighted        et_sparse_adagrad on the same ragged indices: the yardstick
  weighted_sgd      et_weighted_sgd on the same indices (one serial chain per column)

Every timing is the average of `--steps` launches, repeated `--repeats` times (min / median /
max: the spread of this box).  Writes profiles/weighted_adagrad/bench_weighted_adagrad.json.

    python tools/bench_weighted_adagrad.py [--steps 5] [--warmup 2] [--repeats 5] [--out PATH]
"""
import argparse
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
    from embtab.weighted import mean_weights

    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--batch", type=int, default=bench.BATCH)
    p.add_argument("--batches", default="uniform,zipf_1.05")
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "weighted_adagrad",
                                                 "bench_weighted_adagrad.json"))
    a = p.parse_args()

    dev = torch.device("cuda", 0)
    L = _lib.load()
    B, D = a.batch, bench.DIM
    tids = list(range(len(bench.CRITEO_KAGGLE_ROWS)))
    rows = [bench.CRITEO_KAGGLE_ROWS[t] for t in tids]
    tables = bench.make_tables(et, L, tids, dev)
    stream = torch.cuda.current_stream(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20)
    delta = torch.empty((B, D * len(tables)), dtype=torch.float32, device=dev)
    _lib.check(L.et_fill_uniform(_lib.ET_F32, delta.data_ptr(), delta.numel(), 4001, 0, -1.0, 1.0,
                                 stream.cuda_stream))
    blocks = [delta[:, k * D:(k + 1) * D] for k in range(len(tables))]
    ada, row = et.AdaGrad(0.1, weighted=True), et.AdaGrad(0.1, rowwise=True, weighted=True)
    sgd = et.Descent(0.1)
    for A in tables:  # the states, allocated outside the timed region
        ada.state(A), row.state(A)

    def values_of(kind, t, n):
        if kind == "uniform":
            v = torch.empty(n, dtype=torch.int64, device=dev)
            _lib.check(L.et_fill_index_uniform(v.data_ptr(), n, rows[t],
                                               bench.INDEX_SEED + 100 + t, 0, stream.cuda_stream))
            return v
        return bench.zipf_indices(rows[t], (n,), 1.05, gen, dev)

    out = {"workload": f"{len(tables)} Criteo tables x {D} fp32, B = {B}, lengths uniform 0..40",
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    S = et.SparseEmbeddingUpdate
    for name in filter(None, a.batches.split(",")):
        Rs, ws = [], []
        for t in tids:
            l = torch.randint(0, 41, (B,), generator=gen, device=dev)
            R = et.RaggedIndices.from_lengths(values_of(name, t, int(l.sum())), l, check=True)
            w = torch.empty(R.nnz, dtype=torch.float32, device=dev)
            _lib.check(L.et_fill_uniform(_lib.ET_F32, w.data_ptr(), w.numel(), 7000 + t, 0, -1.0,
                                         1.0, stream.cuda_stream))
            Rs.append(R)
            ws.append(w)
        plain = [S(A.lookup_type, d, R) for A, d, R in zip(tables, blocks, Rs)]
        wtd = [S(A.lookup_type, d, R, w) for A, d, R, w in zip(tables, blocks, Rs, ws)]
        mean = [S(A.lookup_type, d, R, mean_weights(R, torch.float32))
                for A, d, R in zip(tables, blocks, Rs)]
        res = alternated({
            "unweighted": lambda: et.update_(ada, tables, plain),
            "weighted": lambda: et.update_(ada, tables, wtd),
            "weighted_rowwise": lambda: et.update_(row, tables, wtd),
            "mean": lambda: et.update_(ada, tables, mean),
            "weighted_sgd": lambda: et.update_(sgd, tables, wtd),
        }, a.steps, a.warmup, a.repeats, stream)
        res["entries"] = int(sum(R.nnz for R in Rs))
        res["hottest_column_entries"] = max(int(torch.bincount(R.values).max()) for R in Rs)
        res["weighted_over_unweighted"] = (res["weighted"]["median_ms"] /
                                           res["unweighted"]["median_ms"])
        res["weighted_sgd_over_weighted"] = (res["weighted_sgd"]["median_ms"] /
                                             res["weighted"]["median_ms"])
        out[name] = res
    assert et.check_errors() == 0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else
                          {kk: (vv["median_ms"] if isinstance(vv, dict) else vv)
                           for kk, vv in v.items()}) for k, v in out.items()}))


if __name__ == "__main__":
    main()
