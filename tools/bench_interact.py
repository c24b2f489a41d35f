"""The pairwise dot interaction on the config-3 shape, timed with HIP events beside the torch
composition a user writes without it.

B = 65,536 samples of F = 27 vectors (26 tables + the dense vector) of D = 128, copy = 128;
Float32 and BFloat16, forward and backward.  et.interact / its pullback alternate in one
process with `torch.bmm` + a `tril_indices` gather + `cat` (autograd for the backward) on the
same tensors for `--rounds` rounds, so drift of the box lands on both alike; every timing is
the mean of `--steps` calls.  Beside each time: the bytes the operation must move (X in, Y
out; X and dY in, dX out) over the time, as a share of the 6.29 TB/s copy ceiling DESIGN.md
uses.  Writes profiles/interact/bench_interact.json.

    python tools/bench_interact.py [--steps 20] [--warmup 5] [--rounds 5] [--out PATH]
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

CEILING = 6.29e12  # bytes/s: the device-to-device copy ceiling of DESIGN.md


def main():
    import torch

    import embtab as et
    from embtab.interact import interact_backward

    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--batch", type=int, default=bench.BATCH)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "interact",
                                                 "bench_interact.json"))
    a = p.parse_args()

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    B, F, D = a.batch, 27, bench.DIM
    NP = F * (F - 1) // 2
    li, lj = (t.to(dev) for t in torch.tril_indices(F, F, -1))
    out = {"workload": f"B = {B}, F = {F}, D = {D}, copy = {D}", "steps": a.steps,
           "warmup": a.warmup, "rounds": a.rounds, "ceiling_bytes_per_s": CEILING}
    for dtype, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        gen = torch.Generator(device=dev)
        gen.manual_seed(3000)
        X = torch.randn((B, F * D), generator=gen, device=dev).to(dtype)
        dY = torch.randn((B, D + NP), generator=gen, device=dev).to(dtype)
        Xg = X.clone().requires_grad_(True)
        es = X.element_size()

        def torch_fwd(x=X):
            xv = x.view(B, F, D)
            z = torch.bmm(xv, xv.transpose(1, 2))
            return torch.cat([x[:, :D], z[:, li, lj]], 1)

        def torch_fwd_bwd():
            Xg.grad = None
            torch_fwd(Xg).backward(dY)

        Y = torch.empty((B, D + NP), dtype=dtype, device=dev)
        runs = {
            "hip_forward": lambda: et.interact_(Y, X, D),
            "torch_forward": torch_fwd,
            "hip_backward": lambda: interact_backward(X, dY, D),
            "torch_forward_backward": torch_fwd_bwd,
        }
        # what was timed computes the same thing: forward against the composition
        ref = torch_fwd().float()
        err = (et.interact(X, D).float() - ref).abs().max().item()
        ms = {k: [] for k in runs}
        for r in range(a.rounds):
            for k, f in runs.items():
                ms[k].append(bench._timed(f, a.steps, a.warmup if r == 0 else 1, stream))
        must = {"forward": B * (F * D + D + NP) * es, "backward": B * (2 * F * D + D + NP) * es}
        res = {"max_abs_diff_vs_torch_forward": err, "bytes_forward": must["forward"],
               "bytes_backward": must["backward"]}
        for k, v in ms.items():
            res[k] = {"min_ms": min(v), "median_ms": statistics.median(v), "max_ms": max(v),
                      "rounds": v}
        # autograd's backward is timed with its forward; its own share is the difference
        res["torch_backward_median_ms"] = (res["torch_forward_backward"]["median_ms"] -
                                           res["torch_forward"]["median_ms"])
        for k in ("forward", "backward"):
            t = res[f"hip_{k}"]["median_ms"] * 1e-3
            res[f"hip_{k}_share_of_ceiling"] = must[k] / t / CEILING
        out[name] = res
        del X, dY, Xg, Y
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for name in ("f32", "bf16"):
        r = out[name]
        print(json.dumps({"dtype": name, **{k: (v["median_ms"] if isinstance(v, dict) else v)
                                            for k, v in r.items()}}))


if __name__ == "__main__":
    main()
