"""Row-wise quantised tables on bench.py's config-3 shape, timed with HIP events beside the
float tables in one process.

26 Criteo tables x 128, pool 20, B = 65,536, PreallocationStrategy, bench.py's table sizes,
table seeds and seeded indices.  Five table forms: Float32, Float16 (Julia Float16 arithmetic,
bench.py's extra line), INT8 with the header fused in the row (ld_bytes 144), INT8 with a split
header array (ld_bytes 128) and INT4 fused (ld_bytes 80); the quantised forms are quantised
from the Float32 tables on the device.  The forms are ALTERNATED: each of `--repeats` rounds
times `--steps` launches of every form in turn, so every Float32 / INT8 pair shares its
moment of the box.  Per form: milliseconds (per round, min / median / max), table bytes, bytes
gathered per launch as used and at 128-byte line granularity (the lines each row touches,
from the row addresses of the actual indices), lookups per second.  Then the serving case:
the same 26 tables, 128 samples, one PreallocationPlan launch replayed from a HIP graph,
Float32 against INT8 fused.  Writes profiles/quant/bench_quant.json.

    python tools/bench_quant.py [--steps 20] [--warmup 5] [--repeats 5] [--out PATH]
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

LINE = 128


def line_bytes(idx, ld_bytes, used, base_mod=0):
    """Bytes of the 128-byte lines the gathered rows touch (every occurrence counted), for
    rows of `used` bytes starting ld_bytes apart."""
    import torch

    start = (idx.view(-1) - 1) * ld_bytes + base_mod
    lines = (start + used - 1) // LINE - start // LINE + 1
    return int(lines.sum().item()) * LINE


def graph_replay_us(plan, stream_dev, replays=200):
    """Microseconds per replay of one captured plan launch."""
    import torch

    side = torch.cuda.Stream(stream_dev)
    side.wait_stream(torch.cuda.current_stream(stream_dev))
    with torch.cuda.stream(side):
        plan()
    torch.cuda.current_stream(stream_dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan()
    for _ in range(20):
        g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / replays


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
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "quant", "bench_quant.json"))
    a = p.parse_args()

    dev = torch.device("cuda", 0)
    L = _lib.load()
    B, P, D = a.batch, bench.POOL, bench.DIM
    tids = list(range(len(bench.CRITEO_KAGGLE_ROWS)))
    T = len(tids)
    stream = torch.cuda.current_stream(dev)
    f32 = bench.make_tables(et, L, tids, dev)
    idx = bench.make_indices(L, tids, B, dev)
    forms = {
        "float32": (f32, torch.float32, 4 * D, 4 * D),
        "float16": ([et.SimpleEmbedding(A.data.to(torch.float16), et.Static(D)) for A in f32],
                    torch.float16, 2 * D, 2 * D),
        "int8_fused": ([et.QuantizedEmbedding.quantize(A, 8, 144) for A in f32],
                       torch.float32, 144, D + 4),
        "int8_split": ([et.QuantizedEmbedding.quantize(A, 8, 128, split_header=True) for A in f32],
                       torch.float32, 128, D),
        "int4_fused": ([et.QuantizedEmbedding.quantize(A, 4, 80) for A in f32],
                       torch.float32, 80, D // 2 + 4),
    }
    strat = et.PreallocationStrategy(0)
    plans, out = {}, {}
    for name, (tabs, dt, ld, used) in forms.items():
        dst = torch.empty((B, D * T), dtype=dt, device=dev)
        plans[name] = et.PreallocationPlan(strat, dst, tabs, idx)
        rows = sum(bench.CRITEO_KAGGLE_ROWS)
        gathered = B * P * T * used + (B * P * T * 4 if name == "int8_split" else 0)
        lines = sum(line_bytes(i, ld, used) for i in idx)
        if name == "int8_split":  # the 4-byte headers live in their own array
            lines += sum(line_bytes(i, 4, 4) for i in idx)
        out[name] = {"ld_bytes": ld, "table_bytes": rows * ld + (rows * 4 if name == "int8_split" else 0),
                     "gathered_bytes_per_launch": gathered,
                     "gathered_line_bytes_per_launch": lines, "repeats_ms": []}
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
    pairs = list(zip(out["float32"]["repeats_ms"], out["int8_fused"]["repeats_ms"]))
    res = {"workload": f"{T} Criteo tables x {D}, B = {B}, pool {P}, PreallocationStrategy",
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "forms": out,
           "int8_fused_faster_than_float32_in_every_pair": all(q < f for f, q in pairs),
           "float32_over_int8_fused": out["float32"]["median_ms"] / out["int8_fused"]["median_ms"],
           "float16_over_int8_fused": out["float16"]["median_ms"] / out["int8_fused"]["median_ms"],
           "int8_split_over_int8_fused": out["int8_split"]["median_ms"] / out["int8_fused"]["median_ms"]}
    # the quantised Float32 output against the float kernels on the dequantised table (one table)
    Q = forms["int8_fused"][0][3]
    y = et.lookup(Q, idx[3][:4096])
    res["int8_equals_float_lookup_of_dequantised_table"] = bool(
        torch.equal(y, et.lookup(et.SimpleEmbedding(Q.dequantize()), idx[3][:4096])))
    del plans
    # serving: 128 samples, one launch replayed from a graph
    Bs = a.serving_batch
    sidx = bench.make_indices(L, tids, Bs, dev)
    serving = {}
    for name in ("float32", "int8_fused"):
        tabs, dt = forms[name][0], forms[name][1]
        dst = torch.empty((Bs, D * T), dtype=dt, device=dev)
        plan = et.PreallocationPlan(strat, dst, tabs, sidx)
        serving[name + "_us"] = [graph_replay_us(plan, dev) for _ in range(3)]
    res["serving"] = {"batch": Bs, **serving}
    assert et.check_errors() == 0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"ms": {k: v["median_ms"] for k, v in out.items()},
                      "int8_fused_faster_in_every_pair":
                          res["int8_fused_faster_than_float32_in_every_pair"],
                      "serving": res["serving"]}))


if __name__ == "__main__":
    main()
