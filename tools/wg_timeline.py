"""Per-workgroup completion timeline of the headline launch (config 3: 26 Criteo tables,
B = 65536, pool 20) from the profiling build (tools/wg_timeline.sh -> tools/tl/).

Every workgroup of the striped or the queued kernel stamps its start and end (s_memrealtime,
100 MHz) with its table, XCC and hardware slot (HW_REG_HW_ID); "cu_affinity" reports how the
classes share a CU (cu_affinity below).  Reported per XCC and per table class (heavy:
> 256 MiB, mid: > 4 MiB, light): when the class's workgroups start and end, so one can
see whether the L2-bound light stripes run after the heavy stripes have drained (the
launch's tail) or beside them, and per table ("per_table": mean workgroup duration, first start,
last end).  ET_TL_CLASS=light|mid|heavy runs that class's tables alone (tools/class_pmc.py PICK).
Usage (GPU box): python tools/wg_timeline.py OUT.json"""
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "embeddingtables.jl_amd"))


def cu_hash16(hw):
    """cu_hash16 of csrc/et_lookup.hip (policy A: a CU prefers the fabric class iff its hash is
    below fab_share): 4-bit bit reversal of cu + 3 se + 5 sh."""
    cu, sh, se = (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7
    v = (cu + 3 * se + 5 * sh) & 15
    return ((v & 1) << 3) | ((v & 2) << 1) | ((v & 4) >> 1) | ((v & 8) >> 3)


def _by_count(dur, cnt):
    """Mean duration (us) of the workgroups by their time-averaged co-resident count."""
    out = {}
    for name, m in (("0", cnt <= 0.0), ("0-1", (cnt > 0.0) & (cnt <= 1.0)),
                    ("1-2", (cnt > 1.0) & (cnt <= 2.0)), (">2", cnt > 2.0)):
        out[name] = {"workgroups": int(m.sum()),
                     "wg_us_mean": float(dur[m].mean()) if m.any() else None}
    return out


def cu_affinity(s, e, c, xcc, hw, home, fab_share):
    """How the table classes share a CU.  CU key: (XCC, SE, SH, CU) of HW_REG_HW_ID.  For every
    light workgroup the number of heavy or mid (fabric-class) workgroups resident on its CU,
    averaged over the light workgroup's lifetime, and the mean light duration by that count;
    the same for fabric-class workgroups by their co-resident light count.  Purity: the share
    of a CU's workgroup-time that belongs to its majority class (0.5 = evenly mixed)."""
    hw = hw.astype(np.int64)
    key = (xcc.astype(np.int64) << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | \
        ((hw >> 8) & 15)
    light, fab = c == "light", (c == "heavy") | (c == "mid")
    dur = e - s
    co = np.zeros(len(s))  # co-resident workgroups of the OTHER class, time-averaged
    purity_num = purity_den = 0.0
    for k in np.unique(key):
        on = np.nonzero((key == k) & (light | fab))[0]
        li, fi = on[light[on]], on[fab[on]]
        if len(li) and len(fi):
            ov = np.minimum(e[li][:, None], e[fi][None, :]) - np.maximum(s[li][:, None], s[fi][None, :])
            ov = np.maximum(ov, 0.0)
            co[li] = ov.sum(1) / np.maximum(dur[li], 1e-9)
            co[fi] = ov.sum(0) / np.maximum(dur[fi], 1e-9)
        tl, tf = dur[li].sum(), dur[fi].sum()
        purity_num += max(tl, tf)
        purity_den += tl + tf
    out = {"cus": int(len(np.unique(key))),
           "light_by_coresident_fabric": _by_count(dur[light], co[light]),
           "fabric_by_coresident_light": _by_count(dur[fab], co[fab]),
           "light_coresident_fabric_mean": float(co[light].mean()) if light.any() else None,
           "fabric_coresident_light_mean": float(co[fab].mean()) if fab.any() else None,
           "cu_class_purity": purity_num / purity_den if purity_den else None,
           "light_wg_on_foreign_xcd": float(np.mean(home[light] != xcc[light])) if light.any() else None}
    # resident workgroups per XCD at the launch's middle (its capacity while every class runs)
    mid = 0.5 * float(e.max())
    out["resident_wg_per_xcd_mid_launch"] = [int(((s <= mid) & (e > mid) & (xcc == x)).sum())
                                             for x in range(8)]
    # policy A's hash on the CUs that are there: share of workgroup starts on fabric CUs
    h = cu_hash16(hw)
    out["fabric_cu_start_share_by_fab_share"] = {str(f): float(np.mean(h < f)) for f in range(1, 16)}
    if fab_share:
        oncache = h >= fab_share
        out["fab_share"] = fab_share
        out["light_wg_time_on_cache_cus"] = float(dur[light & oncache].sum() / dur[light].sum())
        out["fabric_wg_time_on_fabric_cus"] = float(dur[fab & ~oncache].sum() / dur[fab].sum())
        # until a class queue runs dry: light workgroups that start before the last fabric start
        early = light & (s < np.percentile(s[fab], 90))
        out["light_wg_time_on_cache_cus_first_90pct"] = float(
            dur[early & oncache].sum() / max(dur[early].sum(), 1e-9))
    return out


def main():
    # ET_TL_LIBRARY: another profiling build (tools/wg_timeline.sh TL_NAME=..., e.g. with the
    # experiment knobs: ET_AFFINITY, ET_FAB_SHARE are then read by the library)
    os.environ["ET_LIBRARY"] = os.environ.get("ET_TL_LIBRARY") or os.path.join(
        REPO, "tools", "tl", "libembtab_hip.so")
    os.environ["ET_TOOLS_EXPERIMENT"] = "1"
    fab_share = int(os.environ.get("ET_FAB_SHARE", "0")) if os.environ.get("ET_AFFINITY") == "A" else 0
    import torch

    import bench
    from embtab import _lib
    import embtab as et

    L = _lib.load()
    L.et_debug_timeline.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    L.et_debug_timeline.restype = ctypes.c_int
    dev = torch.device("cuda", 0)
    tids = list(range(len(bench.CRITEO_KAGGLE_ROWS)))
    tables = bench.make_tables(et, L, tids, dev)
    idx = bench.make_indices(L, tids, bench.BATCH, dev)
    if os.environ.get("ET_TL_CLASS"):
        from class_pmc import PICK
        keep = [k for k in tids if PICK[os.environ["ET_TL_CLASS"]](bench.CRITEO_KAGGLE_ROWS[k] * bench.DIM * 4)]
        tables, idx = [tables[k] for k in keep], [idx[k] for k in keep]
        bench.CRITEO_KAGGLE_ROWS[:] = [bench.CRITEO_KAGGLE_ROWS[k] for k in keep]
        tids = list(range(len(keep)))
    strat = et.PreallocationStrategy(0)
    dst = torch.empty((bench.BATCH, bench.DIM * len(tids)), dtype=torch.float32, device=dev)
    runs = []
    for it in range(6):
        et.maplookup_(strat, dst, tables, idx)
        torch.cuda.synchronize()
        buf = np.zeros((1 << 17, 8), dtype=np.uint32)
        n = L.et_debug_timeline(buf.ctypes.data, buf.shape[0])
        assert n > 0
        grid = int(buf[0, 7])
        rec = buf[:grid]
        t0 = rec[:, 0].astype(np.uint64) | (rec[:, 1].astype(np.uint64) << np.uint64(32))
        t1 = rec[:, 2].astype(np.uint64) | (rec[:, 3].astype(np.uint64) << np.uint64(32))
        runs.append((grid, t0, t1, rec[:, 4].copy(), rec[:, 5].copy(), rec[:, 6].copy()))
    grid, t0, t1, tab, xcc, hw = runs[-1]  # a warm launch
    home = (tab >> 8) & 0xff  # the queued kernel: the XCD whose queue the item came from
    tab = tab & 0xff
    xcc = xcc & 7
    base = int(t0.min())
    s = (t0.astype(np.int64) - base) / 100.0  # us (100 MHz clock)
    e = (t1.astype(np.int64) - base) / 100.0
    rows = bench.CRITEO_KAGGLE_ROWS
    nbytes = [r * bench.DIM * 4 for r in rows]

    def cls(t):
        if t == 0xff:
            return "idle"
        return "heavy" if nbytes[t] > (256 << 20) else "mid" if nbytes[t] > (4 << 20) else "light"

    c = np.array([cls(int(t)) for t in tab])
    out = {"grid": grid, "launch_us": float(e.max()), "classes": {}, "per_xcc": {},
           "class_tables": {k: [t for t in tids if cls(t) == k] for k in ("heavy", "mid", "light")}}
    for k in ("heavy", "mid", "light", "idle"):
        m = c == k
        if not m.any():
            continue
        d = e[m] - s[m]
        out["classes"][k] = {"workgroups": int(m.sum()), "first_start_us": float(s[m].min()),
                             "last_end_us": float(e[m].max()),
                             "end_p50_us": float(np.percentile(e[m], 50)),
                             "end_p90_us": float(np.percentile(e[m], 90)),
                             "wg_us_mean": float(d.mean()), "wg_us_p90": float(np.percentile(d, 90)),
                             "wg_time_sum_us": float(d.sum())}
    for x in sorted(set(int(v) for v in xcc)):
        mx = xcc == x
        ent = {"workgroups": int(mx.sum()), "last_end_us": float(e[mx].max())}
        for k in ("heavy", "mid", "light"):
            m = mx & (c == k)
            if m.any():
                ent[k] = {"n": int(m.sum()), "last_end_us": float(e[m].max()),
                          "end_p90_us": float(np.percentile(e[m], 90))}
        out["per_xcc"][str(x)] = ent
    # what is running in each 50 us bin: workgroup-time by class (occupancy profile)
    T = float(e.max())
    nb = int(T // 50) + 1
    prof = {k: [0.0] * nb for k in ("heavy", "mid", "light")}
    for k in prof:
        m = c == k
        for a, b in zip(s[m], e[m]):
            for q in range(int(a // 50), int(b // 50) + 1):
                lo, hi = max(a, q * 50.0), min(b, (q + 1) * 50.0)
                if hi > lo:
                    prof[k][q] += (hi - lo) / 50.0
    out["per_table"] = {}
    for t in tids:
        m = tab == t
        if m.any():
            d = e[m] - s[m]
            out["per_table"][str(rows[t])] = {
                "class": cls(t), "workgroups": int(m.sum()), "wg_us_mean": round(float(d.mean()), 2),
                "wg_us_p90": round(float(np.percentile(d, 90)), 2),
                "first_start_us": round(float(s[m].min()), 1), "last_end_us": round(float(e[m].max()), 1)}
    out["resident_wg_per_50us"] = {k: [round(v, 1) for v in p] for k, p in prof.items()}
    out["cu_affinity"] = cu_affinity(s, e, c, xcc, hw, home, fab_share)
    out["xcc_of_blockIdx_mod8_agrees"] = float(np.mean((np.arange(grid) % 8) == xcc))
    out["launch_us_all_runs"] = [float((r[2].astype(np.int64) - r[1].astype(np.int64).min()).max())
                                 / 100.0 for r in runs]
    json.dump(out, open(sys.argv[1], "w"), indent=1)
    print(json.dumps({k: out[k] for k in ("grid", "launch_us", "classes", "launch_us_all_runs",
                                          "cu_affinity")}))


if __name__ == "__main__":
    main()
