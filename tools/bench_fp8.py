"""FP8 (E4M3) tables beside INT8 and Float16 tables on bench.py's config-3 shape, timed with HIP
events in one process — tools/bench_quant.py's method.

26 Criteo tables x 128, pool 20, B = 65,536, PreallocationStrategy, bench.py's table sizes,
table seeds and seeded indices.  Five forms, quantised from the Float32 tables on the device:
Float16, INT8 fused (ld_bytes 144), INT8 split (128), E4M3 fused (144), E4M3 split (128).  The
forms are ALTERNATED: each of `--repeats` rounds times `--steps` launches of every form in
turn, so an E4M3 / INT8 pair shares its moment of the machine; the E4M3 / INT8 ratio is
reported per pair.  The bytes moved by an E4M3 form equal its INT8 form's.  Then the serving
case: 128 samples, one PreallocationPlan launch replayed from a HIP graph, INT8 fused against
E4M3 fused.  Writes profiles/fp8/bench_fp8.json.

    python tools/bench_fp8.py [--steps 20] [--warmup 5] [--repeats 5] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "embeddingtables.jl_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import bench  # noqa: E402
from bench_quant import graph_replay_us  # noqa: E402


def main():
    import torch

    import embtab as et
    from embtab import _lib

    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--batch", type=int, default=bench.BATCH)
    p.add_argument("--serving-batch", type=int, default=128)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "fp8", "bench_fp8.json"))
    a = p.parse_args()

    dev = torch.device("cuda", 0)
    L = _lib.load()
    B, P, D = a.batch, bench.POOL, bench.DIM
    tids = list(range(len(bench.CRITEO_KAGGLE_ROWS)))
    T = len(tids)
    stream = torch.cuda.current_stream(dev)
    f32 = bench.make_tables(et, L, tids, dev)
    idx = bench.make_indices(L, tids, B, dev)
    quant = et.QuantizedEmbedding.quantize
    forms = {
        "float16": ([et.SimpleEmbedding(A.data.to(torch.float16), et.Static(D)) for A in f32],
                    torch.float16, 2 * D),
        "int8_fused": ([quant(A, 8, 144) for A in f32], torch.float32, 144),
        "int8_split": ([quant(A, 8, 128, split_header=True) for A in f32], torch.float32, 128),
        "e4m3_fused": ([quant(A, 8, 144, format="e4m3") for A in f32], torch.float32, 144),
        "e4m3_split": ([quant(A, 8, 128, split_header=True, format="e4m3") for A in f32],
                       torch.float32, 128),
    }
    del f32
    strat = et.PreallocationStrategy(0)
    plans, out = {}, {}
    for name, (tabs, dt, ld) in forms.items():
        plans[name] = et.PreallocationPlan(strat, torch.empty((B, D * T), dtype=dt, device=dev),
                                           tabs, idx)
        out[name] = {"ld_bytes": ld, "repeats_ms": []}
    for name in forms:  # warm-up, every form
        for _ in range(a.warmup):
            plans[name]()
    for r in range(a.repeats):  # alternated: one round times every form in turn
        for name in forms:
            out[name]["repeats_ms"].append(bench._timed(plans[name], a.steps, 1, stream))
    for name in forms:
        ms = out[name]["repeats_ms"]
        out[name].update(min_ms=min(ms), median_ms=statistics.median(ms), max_ms=max(ms),
                         lookups_per_s=B * T * P / (statistics.median(ms) * 1e-3))
    res = {"workload": f"{T} Criteo tables x {D}, B = {B}, pool {P}, PreallocationStrategy",
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "forms": out}
    for kind in ("fused", "split"):
        res[f"e4m3_over_int8_{kind}_per_pair"] = [
            f / q for f, q in zip(out[f"e4m3_{kind}"]["repeats_ms"], out[f"int8_{kind}"]["repeats_ms"])]
    # the Float32 output against the float kernels on the dequantised table (one table)
    Q = forms["e4m3_fused"][0][3]
    res["e4m3_equals_float_lookup_of_dequantised_table"] = bool(torch.equal(
        et.lookup(Q, idx[3][:4096]), et.lookup(et.SimpleEmbedding(Q.dequantize()), idx[3][:4096])))
    del plans
    # serving: 128 samples, one launch replayed from a graph
    Bs = a.serving_batch
    sidx = bench.make_indices(L, tids, Bs, dev)
    serving = {}
    for name in ("int8_fused", "e4m3_fused"):
        dst = torch.empty((Bs, D * T), dtype=torch.float32, device=dev)
        plan = et.PreallocationPlan(strat, dst, forms[name][0], sidx)
        serving[name + "_us"] = [graph_replay_us(plan, dev) for _ in range(3)]
    res["serving"] = {"batch": Bs, **serving}
    assert et.check_errors() == 0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"ms": {k: v["median_ms"] for k, v in out.items()},
                      "e4m3_over_int8_fused_per_pair": res["e4m3_over_int8_fused_per_pair"],
                      "e4m3_over_int8_split_per_pair": res["e4m3_over_int8_split_per_pair"],
                      "serving": res["serving"]}))


if __name__ == "__main__":
    main()
