"""The split sparse SGD over ragged and weighted gradients on bench.py's tables, timed with HIP
events in one process, on the batch of tools/bench_ragged.py's update section: the config-4
Zipf(1.05) indices of the 26 Criteo tables x 128 fp32, B = 65,536, cut into ragged lengths
uniform on 0..40 (case (b)).  Timed:

  exact            et_ragged_sgd (one serial chain per column), `--exact-steps` steps
  split            et.update_(Descent, ..., split=True), et_ragged_sgd_split
  adagrad          element-wise et.AdaGrad on the same ragged gradient
  fixed_split      the fixed-pool exact=False SGD on the uncut (B, 20) indices, for scale
  split_weighted   split=True with a uniform weight per entry
  adagrad_weighted AdaGrad(weighted=True) on the same weighted gradient

Every timed figure but the exact one is `--steps` steps x `--repeats` repeats, reported as
median [min, max] of the per-repeat averages.  Writes profiles/ragged_split/bench_ragged_split.json.

    python tools/bench_ragged_split.py [--steps 20] [--warmup 5] [--repeats 5] [--out PATH]
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
    p.add_argument("--exact-steps", type=int, default=3)
    p.add_argument("--batch", type=int, default=bench.BATCH)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "ragged_split",
                                                 "bench_ragged_split.json"))
    a = p.parse_args()

    dev = torch.device("cuda", 0)
    L = _lib.load()
    B, P, D = a.batch, bench.POOL, bench.DIM
    tids = list(range(len(bench.CRITEO_KAGGLE_ROWS)))
    rows = [bench.CRITEO_KAGGLE_ROWS[t] for t in tids]
    tables = bench.make_tables(et, L, tids, dev)
    stream = torch.cuda.current_stream(dev)

    # tools/bench_ragged.py's draws, in its order: case (b)'s lengths are the first draws from
    # seed 20 (case (a) draws nothing), then the Zipf(1.05) indices from seed 4000
    gen = torch.Generator(device=dev)
    gen.manual_seed(20)
    lengths = [torch.randint(0, 41, (B,), generator=gen, device=dev) for _ in tids]
    gen4 = torch.Generator(device=dev)
    gen4.manual_seed(4000)
    delta = torch.empty((B, D * len(tables)), dtype=torch.float32, device=dev)
    _lib.check(L.et_fill_uniform(_lib.ET_F32, delta.data_ptr(), delta.numel(), 4001, 0, -1.0, 1.0,
                                 stream.cuda_stream))
    Rz, fixed_z = [], []
    for t, l in zip(tids, lengths):
        z = bench.zipf_indices(rows[t], (B, P), 1.05, gen4, dev)
        fixed_z.append(z)
        n = int(l.sum())
        flat = z.view(-1)
        v = flat[:n].contiguous() if n <= flat.numel() else torch.cat(
            [flat, bench.zipf_indices(rows[t], (n - flat.numel(),), 1.05, gen4, dev)])
        Rz.append(et.RaggedIndices.from_lengths(v, l))
    blk = [delta[:, k * D:(k + 1) * D] for k in range(len(tables))]
    rgrads = [et.SparseEmbeddingUpdate(A.lookup_type, d, R) for A, d, R in zip(tables, blk, Rz)]
    fgrads = [et.SparseEmbeddingUpdate(A.lookup_type, d, i)
              for A, d, i in zip(tables, blk, fixed_z)]
    gw = torch.Generator(device=dev)
    gw.manual_seed(4002)
    wgrads = [et.SparseEmbeddingUpdate(
        A.lookup_type, d, R, 0.5 + torch.rand(R.nnz, generator=gw, device=dev))
        for A, d, R in zip(tables, blk, Rz)]

    sgd = et.Descent(0.1)
    ada = et.AdaGrad(0.1, 1e-8, weighted=True)  # one state set serves both AdaGrad timings
    for A in tables:
        ada.state(A)
    runs = {
        "split": lambda: et.update_(sgd, tables, rgrads, split=True),
        "adagrad": lambda: et.update_(ada, tables, rgrads),
        "fixed_split": lambda: et.update_(sgd, tables, fgrads, exact=False),
        "split_weighted": lambda: et.update_(sgd, tables, wgrads, split=True),
        "adagrad_weighted": lambda: et.update_(ada, tables, wgrads),
    }
    out = {"workload": f"{len(tables)} Criteo tables x {D} fp32, B = {B}, Zipf(1.05) indices "
                       "cut into lengths uniform on 0..40",
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "entries": int(sum(R.nnz for R in Rz)),
           "hottest_column_entries": int(max(int(torch.bincount(R.values).max()) for R in Rz)),
           "update": {}}
    out["update"]["exact"] = spread(lambda: et.update_(sgd, tables, rgrads), a.exact_steps, 1,
                                    min(a.repeats, 3), stream)
    out["update"]["exact"]["steps"] = a.exact_steps
    # two passes over the timed runs, interleaved, so a drift of the box shows in the spread
    # of each figure instead of between them
    half = max(a.repeats // 2, 1)
    first = {k: spread(fn, a.steps, a.warmup, half, stream) for k, fn in runs.items()}
    for k, fn in runs.items():
        rest = spread(fn, a.steps, 1, a.repeats - half, stream) if a.repeats > half else None
        ms = first[k]["repeats"] + (rest["repeats"] if rest else [])
        out["update"][k] = {"min_ms": min(ms), "median_ms": statistics.median(ms),
                            "max_ms": max(ms), "repeats": ms}
    assert et.check_errors() == 0

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: round(v["median_ms"], 3) for k, v in out["update"].items()}))


if __name__ == "__main__":
    main()
