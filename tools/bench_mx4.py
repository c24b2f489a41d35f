"""MXFP4 tables beside INT4 and Float16 tables on bench.py's config-3 shape, timed with HIP
events in one process — tools/bench_quant.py's method.

26 Criteo tables x 128, pool 20, B = 65,536, PreallocationStrategy, bench.py's table sizes,
table seeds and seeded indices.  Four forms, quantised from the Float32 tables on the device:
Float16, INT4 fused (ld_bytes 80), MXFP4 fused (80: the same row bytes as INT4) and MXFP4 split
(64: two rows per 128-byte line, never straddling one).  The forms are ALTERNATED: each of
`--repeats` rounds times `--steps` launches of every form in turn, so an MXFP4 / INT4 pair shares
its moment of the machine; the ratio is reported per pair.  Writes profiles/mx4/bench_mx4.json.

    python tools/bench_mx4.py [--steps 20] [--warmup 5] [--repeats 5] [--out PATH]
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
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "mx4", "bench_mx4.json"))
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
        "int4_fused": ([quant(A, 4, 80) for A in f32], torch.float32, 80),
        "mxfp4_fused": ([quant(A, None, 80, format="mxfp4") for A in f32], torch.float32, 80),
        "mxfp4_split": ([quant(A, None, 64, split_header=True, format="mxfp4") for A in f32],
                        torch.float32, 64),
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
        res[f"mxfp4_{kind}_over_int4_fused_per_pair"] = [
            m / q for m, q in zip(out[f"mxfp4_{kind}"]["repeats_ms"], out["int4_fused"]["repeats_ms"])]
    # the Float32 output against the float kernels on the dequantised table (one table)
    Q = forms["mxfp4_fused"][0][3]
    res["mxfp4_equals_float_lookup_of_dequantised_table"] = bool(torch.equal(
        et.lookup(Q, idx[3][:4096]), et.lookup(et.SimpleEmbedding(Q.dequantize()), idx[3][:4096])))
    assert et.check_errors() == 0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"ms": {k: v["median_ms"] for k, v in out.items()},
                      "range_ms": {k: [v["min_ms"], v["max_ms"]] for k, v in out.items()},
                      "mxfp4_fused_over_int4": res["mxfp4_fused_over_int4_fused_per_pair"],
                      "mxfp4_split_over_int4": res["mxfp4_split_over_int4_fused_per_pair"],
                      "equal": res["mxfp4_equals_float_lookup_of_dequantised_table"]}))


if __name__ == "__main__":
    main()
