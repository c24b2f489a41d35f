"""Sparse AdaGrad on bench.py's tables, timed with HIP events beside the sparse SGD.

The config-4 tables (26 Criteo tables x 128 fp32, B = 65,536, pool 20) with the config-4
Zipf(1.05) batch and a uniform batch; for each batch, in the same run: element-wise AdaGrad,
row-wise AdaGrad, the split sparse SGD (``exact=False``, the yardstick: AdaGrad's chunks are
the split mode's) and the exact sparse SGD.  Every timing is `--steps` updates repeated
`--repeats` times (min / median / max of the per-repeat averages: the spread of this box).
Writes profiles/adagrad/bench_adagrad.json.

    python tools/bench_adagrad.py [--steps 20] [--warmup 5] [--repeats 5] [--out PATH]
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


def spread(fn, steps, warmup, repeats, stream):
    ms = [bench._timed(fn, steps, warmup if r == 0 else 1, stream) for r in range(repeats)]
    return {"min_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms),
            "repeats": ms}


def main():
    import torch

    import embtab as et
    from embtab import _lib

    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--batch", type=int, default=bench.BATCH)
    p.add_argument("--only", default="", help="comma list of: adagrad,rowwise,split,exact")
    p.add_argument("--batches", default="zipf_1.05,uniform")
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "adagrad",
                                                 "bench_adagrad.json"))
    a = p.parse_args()

    dev = torch.device("cuda", 0)
    L = _lib.load()
    B, P, D = a.batch, bench.POOL, bench.DIM
    tids = list(range(len(bench.CRITEO_KAGGLE_ROWS)))
    rows = [bench.CRITEO_KAGGLE_ROWS[t] for t in tids]
    tables = bench.make_tables(et, L, tids, dev)
    stream = torch.cuda.current_stream(dev)
    delta = torch.empty((B, D * len(tables)), dtype=torch.float32, device=dev)
    _lib.check(L.et_fill_uniform(_lib.ET_F32, delta.data_ptr(), delta.numel(), 4001, 0, -1.0, 1.0,
                                 stream.cuda_stream))
    gen = torch.Generator(device=dev)
    gen.manual_seed(4000)
    batches = {
        "zipf_1.05": lambda: [bench.zipf_indices(rows[t], (B, P), 1.05, gen, dev) for t in tids],
        "uniform": lambda: bench.make_indices(L, tids, B, dev),
    }
    ada, row, sgd = et.AdaGrad(0.1), et.AdaGrad(0.1, rowwise=True), et.Descent(0.1)
    for A in tables:  # the states, allocated outside the timed region
        ada.state(A), row.state(A)
    only = set(filter(None, a.only.split(",")))
    out = {"workload": f"{len(tables)} Criteo tables x {D} fp32, B = {B}, pool {P}",
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    for name in filter(None, a.batches.split(",")):
        idx = batches[name]()
        grads = [et.SparseEmbeddingUpdate(A.lookup_type, delta[:, k * D:(k + 1) * D], i)
                 for k, (A, i) in enumerate(zip(tables, idx))]
        runs = {
            "adagrad": lambda: et.update_(ada, tables, grads),
            "rowwise": lambda: et.update_(row, tables, grads),
            "split": lambda: et.update_(sgd, tables, grads, exact=False),
            "exact": lambda: et.update_(sgd, tables, grads, exact=True),
        }
        res = {k: spread(f, a.steps, a.warmup, a.repeats, stream) for k, f in runs.items()
               if not only or k in only}
        U = sum(int(torch.unique(i).numel()) for i in idx)
        res["distinct_columns"] = U
        res["hottest_column_occurrences"] = max(int(torch.bincount(i.view(-1)).max())
                                                for i in idx)
        res["state_rmw_bytes_elementwise"] = 2 * U * D * 4
        if "adagrad" in res and "split" in res:
            res["adagrad_over_split"] = res["adagrad"]["median_ms"] / res["split"]["median_ms"]
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
