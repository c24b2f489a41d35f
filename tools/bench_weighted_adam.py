"""Sparse Adam over weighted and mean-pooled gradients on bench.py's tables, timed with HIP
events.

The config-4 tables (26 Criteo tables x 128 fp32, B = 65,536) with the ragged Zipf(1.05) batch
of tools/bench_weighted_adagrad.py (bag lengths uniform on 0..40).  These updates alternate in
one process for `--rounds` rounds, so drift of the box lands on all alike; every timing is
`--steps` updates:

  weighted           et_weighted_adam, element-wise, weights uniform on [-1, 1)
  weighted_rowwise   the same, row-wise
  mean               et_weighted_adam with the mean-mode weights 1 / len(bag)
  unit_weights       et_weighted_adam with every weight 1.0: the pair-stream chunk kernel on
                     the batch k_adam_chunks sums below
  unweighted         et_sparse_adam on the same ragged indices: the yardstick
  weighted_adagrad   et_weighted_adagrad, element-wise, the same weights
  adagrad            et_sparse_adagrad on the same ragged indices

Writes profiles/weighted_adam/bench_weighted_adam.json.  `--only NAME --steps N --rounds 1` runs
one update alone (for a kernel trace).

    python tools/bench_weighted_adam.py [--steps 20] [--warmup 5] [--rounds 5] [--out PATH]
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
    from embtab.weighted import mean_weights

    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--batch", type=int, default=bench.BATCH)
    p.add_argument("--only", default="")
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "weighted_adam",
                                                 "bench_weighted_adam.json"))
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
    Rs, ws = [], []
    for t in tids:
        l = torch.randint(0, 41, (B,), generator=gen, device=dev)
        R = et.RaggedIndices.from_lengths(
            bench.zipf_indices(rows[t], (int(l.sum()),), 1.05, gen, dev), l, check=True)
        w = torch.empty(R.nnz, dtype=torch.float32, device=dev)
        _lib.check(L.et_fill_uniform(_lib.ET_F32, w.data_ptr(), w.numel(), 7000 + t, 0, -1.0, 1.0,
                                     stream.cuda_stream))
        Rs.append(R)
        ws.append(w)
    S = et.SparseEmbeddingUpdate
    plain = [S(A.lookup_type, d, R) for A, d, R in zip(tables, blocks, Rs)]
    wtd = [S(A.lookup_type, d, R, w) for A, d, R, w in zip(tables, blocks, Rs, ws)]
    ones = [S(A.lookup_type, d, R, torch.ones_like(w))
            for A, d, R, w in zip(tables, blocks, Rs, ws)]
    mean = [S(A.lookup_type, d, R, mean_weights(R, torch.float32))
            for A, d, R in zip(tables, blocks, Rs)]
    wadam, wadam_row = et.Adam(1e-3, weighted=True), et.Adam(1e-3, rowwise=True, weighted=True)
    adam, ada, wada = et.Adam(1e-3), et.AdaGrad(0.1), et.AdaGrad(0.1, weighted=True)
    for A in tables:  # the states, allocated outside the timed region
        for o in (wadam, wadam_row, adam):
            o.state(A), o.step(A)
        ada.state(A), wada.state(A)
    runs = {
        "weighted": lambda: et.update_(wadam, tables, wtd),
        "weighted_rowwise": lambda: et.update_(wadam_row, tables, wtd),
        "mean": lambda: et.update_(wadam, tables, mean),
        "unit_weights": lambda: et.update_(wadam, tables, ones),
        "unweighted": lambda: et.update_(adam, tables, plain),
        "weighted_adagrad": lambda: et.update_(wada, tables, wtd),
        "adagrad": lambda: et.update_(ada, tables, plain),
    }
    if a.only:
        runs = {a.only: runs[a.only]}
    ms = {k: [] for k in runs}
    for r in range(a.rounds):
        for k, f in runs.items():
            ms[k].append(bench._timed(f, a.steps, a.warmup if r == 0 else 1, stream))
    assert et.check_errors() == 0
    out = {"workload": f"{len(tables)} Criteo tables x {D} fp32, B = {B}, lengths uniform 0..40, "
                       "Zipf(1.05)",
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "entries": int(sum(R.nnz for R in Rs)),
           "hottest_column_entries": max(int(torch.bincount(R.values).max()) for R in Rs)}
    for k, v in ms.items():
        out[k] = {"min_ms": min(v), "median_ms": statistics.median(v), "max_ms": max(v),
                  "rounds": v}
    if not a.only:
        med = lambda k: out[k]["median_ms"]
        out["weighted_over_unweighted"] = med("weighted") / med("unweighted")
        out["unit_weights_over_unweighted"] = med("unit_weights") / med("unweighted")
        out["weighted_adagrad_over_adagrad"] = med("weighted_adagrad") / med("adagrad")
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
