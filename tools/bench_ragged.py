"""Ragged lookup and update on bench.py's tables, timed with HIP events.

Forward: the fused ragged maplookup (et_ragged_maplookup_prealloc) of the config-3 tables
(26 Criteo tables x 128 fp32, B = 65,536) with (a) every bag of length 20, beside the same
run's fixed-pool maplookup_ at P = 20 on the same indices, (b) lengths uniform on 0..40,
(c) geometric lengths of mean 20 capped at 200.  Update: et_ragged_sgd of every table on the
config-4 Zipf(1.05) indices cut into case (b)'s lengths, beside the fixed-pool exact update of
the same run.  Every timing is repeated `--repeats` times (min / median / max of the per-repeat
averages: the spread of this box).  Writes profiles/ragged/bench_ragged.json.

    python tools/bench_ragged.py [--steps 20] [--warmup 5] [--repeats 5] [--out PATH]
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
    p.add_argument("--update-steps", type=int, default=3)
    p.add_argument("--batch", type=int, default=bench.BATCH)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "ragged", "bench_ragged.json"))
    a = p.parse_args()

    dev = torch.device("cuda", 0)
    L = _lib.load()
    B, P, D = a.batch, bench.POOL, bench.DIM
    tids = list(range(len(bench.CRITEO_KAGGLE_ROWS)))
    rows = [bench.CRITEO_KAGGLE_ROWS[t] for t in tids]
    tables = bench.make_tables(et, L, tids, dev)
    stream = torch.cuda.current_stream(dev)
    strat = et.PreallocationStrategy(0)
    dst = torch.empty((B, D * len(tables)), dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20)

    def lengths(case):
        if case == "a_fixed20":
            return torch.full((B,), P, dtype=torch.int64, device=dev)
        if case == "b_uniform_0_40":
            return torch.randint(0, 41, (B,), generator=gen, device=dev)
        # geometric on 0, 1, 2, ... with mean 20 (p = 1/21), capped at 200
        u = torch.rand((B,), generator=gen, device=dev, dtype=torch.float64)
        g = torch.floor(torch.log1p(-u) / torch.log(torch.tensor(20.0 / 21.0, device=dev)))
        return g.clamp_(0, 200).long()

    out = {"workload": f"{len(tables)} Criteo tables x {D} fp32, B = {B}", "steps": a.steps,
           "warmup": a.warmup, "repeats": a.repeats, "forward": {}}

    # the fixed-pool launch of this run, and case (a) on the very same indices
    fixed_idx = bench.make_indices(L, tids, B, dev)
    out["forward"]["fixed_pool_20"] = spread(lambda: et.maplookup_(strat, dst, tables, fixed_idx),
                                             a.steps, a.warmup, a.repeats, stream)
    want = dst.clone()
    for case in ("a_fixed20", "b_uniform_0_40", "c_geometric_mean20_cap200"):
        Ls = [lengths(case) for _ in tids]  # one length draw per table
        if case == "a_fixed20":
            Rs = [et.RaggedIndices.from_lengths(i.view(-1), l) for i, l in zip(fixed_idx, Ls)]
        else:
            Rs = []
            for t, l in zip(tids, Ls):
                v = torch.empty(int(l.sum()), dtype=torch.int64, device=dev)
                _lib.check(L.et_fill_index_uniform(v.data_ptr(), v.numel(), rows[t],
                                                   bench.INDEX_SEED + 100 + t, 0,
                                                   stream.cuda_stream))
                Rs.append(et.RaggedIndices.from_lengths(v, l, check=True))
        plan = et.PreallocationPlan(strat, dst, tables, Rs)
        r = spread(plan, a.steps, a.warmup, a.repeats, stream)
        r["entries"] = int(sum(int(l.sum()) for l in Ls))
        r["mean_length"] = r["entries"] / (B * len(tables))
        r["max_length"] = int(max(int(l.max()) for l in Ls))
        r["ns_per_entry"] = 1e6 * r["median_ms"] / max(r["entries"], 1)
        if case == "a_fixed20":
            r["bit_identical_to_fixed_pool"] = bool(torch.equal(dst, want))
        out["forward"][case] = r
        if case == "b_uniform_0_40":
            b_lengths = Ls
    assert et.check_errors() == 0

    # update: config-4 Zipf(1.05) indices, cut into case (b)'s lengths
    gen4 = torch.Generator(device=dev)
    gen4.manual_seed(4000)
    delta = torch.empty_like(dst)
    _lib.check(L.et_fill_uniform(_lib.ET_F32, delta.data_ptr(), delta.numel(), 4001, 0, -1.0, 1.0,
                                 stream.cuda_stream))
    Rz, fixed_z = [], []
    for t, l in zip(tids, b_lengths):
        z = bench.zipf_indices(rows[t], (B, P), 1.05, gen4, dev)
        fixed_z.append(z)
        n = int(l.sum())
        flat = z.view(-1)
        v = flat[:n].contiguous() if n <= flat.numel() else torch.cat(
            [flat, bench.zipf_indices(rows[t], (n - flat.numel(),), 1.05, gen4, dev)])
        Rz.append(et.RaggedIndices.from_lengths(v, l))
    opt = et.Descent(0.1)
    rgrads = [et.SparseEmbeddingUpdate(A.lookup_type, delta[:, k * D:(k + 1) * D], R)
              for k, (A, R) in enumerate(zip(tables, Rz))]
    fgrads = [et.SparseEmbeddingUpdate(A.lookup_type, delta[:, k * D:(k + 1) * D], i)
              for k, (A, i) in enumerate(zip(tables, fixed_z))]
    us = a.update_steps
    out["update"] = {
        "ragged_zipf_lengths_b": spread(lambda: et.update_(opt, tables, rgrads), us, 1,
                                        min(a.repeats, 3), stream),
        "fixed_pool_20_zipf_exact": spread(lambda: et.update_(opt, tables, fgrads), us, 1,
                                           min(a.repeats, 3), stream),
    }
    u = out["update"]["ragged_zipf_lengths_b"]
    u["entries"] = int(sum(R.nnz for R in Rz))
    u["hottest_column_entries"] = int(max(int(torch.bincount(R.values).max()) for R in Rz))
    # the cost of the serial hot columns: the same update without the 7 smallest tables
    # (3 to 27 rows: every column hot)
    big = [k for k, r in enumerate(rows) if r > 100]
    out["update"]["ragged_tables_over_100_rows"] = spread(
        lambda: et.update_(opt, [tables[k] for k in big], [rgrads[k] for k in big]), us, 1,
        min(a.repeats, 3), stream)
    out["update"]["ragged_tables_over_100_rows"]["tables"] = len(big)
    assert et.check_errors() == 0

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else
                          {kk: (vv["median_ms"] if isinstance(vv, dict) else vv)
                           for kk, vv in v.items()}) for k, v in out.items()}))


if __name__ == "__main__":
    main()
