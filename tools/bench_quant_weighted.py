"""Weighted and mean-pooled bags over quantised tables on bench.py's tables, timed with HIP
events in one process — tools/bench_mx4.py's and tools/bench_weighted.py's method.

The ragged config-3 case of tools/bench_weighted.py: 26 Criteo tables x 128, B = 65,536, bag
lengths uniform on 0..40, seeded indices and weights in [-1, 1).  Launches, ALTERNATED inside
every round so that the members of a ratio share their moment of the machine:

  int8_unweighted   et_quant_maplookup_prealloc on the ragged bags (the existing kernel)
  int8_mean         et_quant_weighted_maplookup_prealloc, mode mean
  int8_weighted / int4_weighted / e4m3_weighted / mxfp4_weighted   the same entry with weights
  int4_unweighted / e4m3_unweighted / mxfp4_unweighted             each format's own baseline
  float32_weighted / float16_weighted   et_weighted_maplookup_prealloc on float tables

Every timing is the average of `--steps` launches; `--repeats` rounds.  Ratios are formed per
round.  Writes profiles/quant_weighted/bench_quant_weighted.json.

    python tools/bench_quant_weighted.py [--steps 20] [--warmup 5] [--repeats 5] [--out PATH]
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
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--batch", type=int, default=bench.BATCH)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "quant_weighted",
                                                 "bench_quant_weighted.json"))
    a = p.parse_args()

    dev = torch.device("cuda", 0)
    L = _lib.load()
    B, D = a.batch, bench.DIM
    tids = list(range(len(bench.CRITEO_KAGGLE_ROWS)))
    T = len(tids)
    stream = torch.cuda.current_stream(dev)
    f32 = bench.make_tables(et, L, tids, dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20)
    Rs, Ws, Ms = [], [], []
    for t in tids:
        l = torch.randint(0, 41, (B,), generator=gen, device=dev)
        v = torch.empty(int(l.sum()), dtype=torch.int64, device=dev)
        _lib.check(L.et_fill_index_uniform(v.data_ptr(), v.numel(), bench.CRITEO_KAGGLE_ROWS[t],
                                           bench.INDEX_SEED + 100 + t, 0, stream.cuda_stream))
        R = et.RaggedIndices.from_lengths(v, l, check=True)
        w = torch.empty(v.numel(), dtype=torch.float32, device=dev)
        _lib.check(L.et_fill_uniform(_lib.ET_F32, w.data_ptr(), w.numel(), 7000 + t, 0, -1.0, 1.0,
                                     stream.cuda_stream))
        Rs.append(R)
        Ws.append(et.WeightedIndices(R, w))
        Ms.append(et.WeightedIndices(R, mode="mean"))
    entries = int(sum(R.nnz for R in Rs))

    quant = et.QuantizedEmbedding.quantize
    tabs = {
        "int8": [quant(A, 8, weighted=True) for A in f32],
        "int4": [quant(A, 4, weighted=True) for A in f32],
        "e4m3": [quant(A, format="e4m3", weighted=True) for A in f32],
        "mxfp4": [quant(A, format="mxfp4", weighted=True) for A in f32],
        "float16": [et.SimpleEmbedding(A.data.to(torch.float16), et.Static(D)) for A in f32],
        "float32": f32,
    }
    strat = et.PreallocationStrategy(0)
    dst = {dt: torch.empty((B, D * T), dtype=dt, device=dev) for dt in (torch.float32, torch.float16)}

    def plan(name, idx):
        return et.PreallocationPlan(strat, dst[tabs[name][0].dtype], tabs[name], idx)

    cases = {"int8_unweighted": plan("int8", Rs), "int8_mean": plan("int8", Ms)}
    for name in ("int8", "int4", "e4m3", "mxfp4"):
        cases[f"{name}_weighted"] = plan(name, Ws)
        cases.setdefault(f"{name}_unweighted", plan(name, Rs))
    for name in ("float32", "float16"):
        cases[f"{name}_weighted"] = plan(name, Ws)

    ms = {name: [] for name in cases}
    for name, fn in cases.items():  # warm-up, every launch
        for _ in range(a.warmup):
            fn()
    for r in range(a.repeats):
        for name, fn in cases.items():
            ms[name].append(bench._timed(fn, a.steps, 1, stream))
    out = {name: {"min_ms": min(v), "median_ms": statistics.median(v), "max_ms": max(v),
                  "repeats_ms": v, "ns_per_entry": 1e6 * statistics.median(v) / max(entries, 1)}
           for name, v in ms.items()}
    res = {"workload": f"{T} Criteo tables x {D}, B = {B}, lengths uniform 0..40",
           "entries": entries, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "launches": out, "weighted_over_unweighted_per_round": {
               name: [w / u for w, u in zip(ms[f"{name}_weighted"], ms[f"{name}_unweighted"])]
               for name in ("int8", "int4", "e4m3", "mxfp4")},
           "int8_mean_over_unweighted_per_round": [
               m / u for m, u in zip(ms["int8_mean"], ms["int8_unweighted"])]}
    # the Float32 output against the float weighted kernel on the dequantised table (one table)
    Q, W = tabs["int8"][3], Ws[3]
    res["int8_weighted_equals_float_weighted_on_dequantised_table"] = bool(torch.equal(
        et.lookup(Q, W), et.lookup(et.SimpleEmbedding(Q.dequantize()), W)))
    assert et.check_errors() == 0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"median_ms": {k: v["median_ms"] for k, v in out.items()},
                      "weighted_over_unweighted": {
                          k: statistics.median(v)
                          for k, v in res["weighted_over_unweighted_per_round"].items()},
                      "int8_mean_over_unweighted": statistics.median(
                          res["int8_mean_over_unweighted_per_round"]),
                      "equal": res["int8_weighted_equals_float_weighted_on_dequantised_table"]}))


if __name__ == "__main__":
    main()
