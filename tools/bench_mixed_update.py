"""Float32 tables updated from BFloat16 gradients, timed with HIP events beside today's ways.

The config-4 tables (26 Criteo tables x 128 fp32, B = 65,536, pool 20) with the config-4
Zipf(1.05) batch.  For AdaGrad and Adam, element-wise and row-wise, three forms of one update
alternate in one process for `--rounds` rounds, so drift of the box lands on all alike:

  f32        the Float32 gradient, as before
  cast_f32   `delta.float()` of the BFloat16 gradient, then the Float32 update: what a
             BFloat16 step had to do
  bf16       the BFloat16 gradient as it is (ET_FLAG_DELTA_BF16)

Every timing is `--steps` updates.  Writes profiles/mixed_update/bench_mixed_update.json.

    python tools/bench_mixed_update.py [--steps 20] [--warmup 5] [--rounds 5] [--out PATH]
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
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "mixed_update",
                                                 "bench_mixed_update.json"))
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
    delta16 = delta.to(torch.bfloat16)
    gen = torch.Generator(device=dev)
    gen.manual_seed(4000)
    idx = [bench.zipf_indices(rows[t], (B, P), 1.05, gen, dev) for t in tids]

    def grads(d):
        return [et.SparseEmbeddingUpdate(A.lookup_type, d[:, k * D:(k + 1) * D], i)
                for k, (A, i) in enumerate(zip(tables, idx))]

    g32, g16 = grads(delta), grads(delta16)
    opts = {"adagrad": et.AdaGrad(0.1), "adagrad_rowwise": et.AdaGrad(0.1, rowwise=True),
            "adam": et.Adam(1e-3), "adam_rowwise": et.Adam(1e-3, rowwise=True)}
    for opt in opts.values():  # the states, allocated outside the timed region
        for A in tables:
            opt.state(A)
            if isinstance(opt, et.Adam):
                opt.step(A)
    runs = {}
    for name, opt in opts.items():
        runs[f"{name}/f32"] = lambda opt=opt: et.update_(opt, tables, g32)
        runs[f"{name}/cast_f32"] = lambda opt=opt: et.update_(opt, tables, grads(delta16.float()))
        runs[f"{name}/bf16"] = lambda opt=opt: et.update_(opt, tables, g16)
    ms = {k: [] for k in runs}
    for r in range(a.rounds):
        for k, f in runs.items():
            ms[k].append(bench._timed(f, a.steps, a.warmup if r == 0 else 1, stream))
    assert et.check_errors() == 0
    n = B * P * len(tables)
    out = {"workload": f"{len(tables)} Criteo tables x {D} fp32, B = {B}, pool {P}, Zipf(1.05)",
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "gradient_gather_bytes": {"f32": n * D * 4, "bf16": n * D * 2},
           "cast_bytes": B * D * len(tables) * (2 + 4)}
    for k, v in ms.items():
        out[k] = {"min_ms": min(v), "median_ms": statistics.median(v), "max_ms": max(v),
                  "rounds": v}
    for name in opts:
        f32, b16 = ms[f"{name}/f32"], ms[f"{name}/bf16"]
        out[f"{name}/bf16_over_f32"] = out[f"{name}/bf16"]["median_ms"] / out[f"{name}/f32"]["median_ms"]
        out[f"{name}/bf16_over_cast_f32"] = (out[f"{name}/bf16"]["median_ms"] /
                                             out[f"{name}/cast_f32"]["median_ms"])
        # the claim to check: bf16 is not slower than f32 in any round
        out[f"{name}/rounds_bf16_slower_than_f32"] = sum(x > y for x, y in zip(b16, f32))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (round(v["median_ms"], 4) if isinstance(v, dict) and "median_ms" in v
                          else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
