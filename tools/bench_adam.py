"""Sparse Adam on bench.py's tables, timed with HIP events beside AdaGrad and the split SGD.

The config-4 tables (26 Criteo tables x 128 fp32, B = 65,536, pool 20) with the config-4
Zipf(1.05) batch.  Element-wise Adam, row-wise Adam, element-wise AdaGrad (the yardstick: the
same front and gradient gather, four row transfers per touched column against Adam's six) and
the split sparse SGD alternate in one process for `--rounds` rounds, so drift of the box lands
on all four alike; every timing is `--steps` updates.  Writes profiles/adam/bench_adam.json.

    python tools/bench_adam.py [--steps 20] [--warmup 5] [--rounds 5] [--out PATH]
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


def main():
    import torch

    import embtab as et
    from embtab import _lib

    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--batch", type=int, default=bench.BATCH)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "adam", "bench_adam.json"))
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
    idx = [bench.zipf_indices(rows[t], (B, P), 1.05, gen, dev) for t in tids]
    grads = [et.SparseEmbeddingUpdate(A.lookup_type, delta[:, k * D:(k + 1) * D], i)
             for k, (A, i) in enumerate(zip(tables, idx))]
    adam, adam_row = et.Adam(1e-3), et.Adam(1e-3, rowwise=True)
    ada, sgd = et.AdaGrad(0.1), et.Descent(0.1)
    for A in tables:  # the states, allocated outside the timed region
        adam.state(A), adam.step(A), adam_row.state(A), adam_row.step(A), ada.state(A)
    runs = {
        "adam": lambda: et.update_(adam, tables, grads),
        "adam_rowwise": lambda: et.update_(adam_row, tables, grads),
        "adagrad": lambda: et.update_(ada, tables, grads),
        "split_sgd": lambda: et.update_(sgd, tables, grads, exact=False),
    }
    ms = {k: [] for k in runs}
    for r in range(a.rounds):
        for k, f in runs.items():
            ms[k].append(bench._timed(f, a.steps, a.warmup if r == 0 else 1, stream))
    assert et.check_errors() == 0
    U = sum(int(torch.unique(i).numel()) for i in idx)
    out = {"workload": f"{len(tables)} Criteo tables x {D} fp32, B = {B}, pool {P}, Zipf(1.05)",
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "distinct_columns": U,
           "row_bytes_moved": {"adam": 6 * U * D * 4, "adam_rowwise": 4 * U * D * 4 + 8 * U,
                               "adagrad": 4 * U * D * 4, "split_sgd": 2 * U * D * 4},
           "gradient_gather_bytes": B * P * len(tables) * D * 4}
    for k, v in ms.items():
        out[k] = {"min_ms": min(v), "median_ms": statistics.median(v), "max_ms": max(v),
                  "rounds": v}
    for k in ("adam", "adam_rowwise"):
        out[f"{k}_over_adagrad"] = out[k]["median_ms"] / out["adagrad"]["median_ms"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v)
                      for k, v in out.items()}))


if __name__ == "__main__":
    main()
