"""ThinK timing: the whole SnapKVCluster.update_think next to the whole update_kv on the same tensors in one process, the
three ThinK kernels next to gather_kernel of the same call, and an eager PyTorch-ROCm run of the pruner for scale.

    python tools/think_bench.py --out profiles/think/think_bench.json                          # whole calls (HIP events) + eager
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/think_bench.py --trace           # a run of its own: kernels only
    python tools/think_bench.py --kernel-trace DIR --out profiles/think/think_bench.json       # fold the trace into the record

Shape: [1, 32, 32768, 128] bf16, window 32, recent 32, ratio 0.4 (51 of 128 channels go), cap 4096, 2048 and 128.
Whole calls: medians of --reps calls bracketed by HIP events, --rounds rounds alternating update_think / update_kv.
Kernels: the dispatches' own begin / end timestamps from the kernel trace (the ThinK kernels have no pkv_prof_* class); the
traced run makes, per cap, --rounds x (warm + reps) calls of update_think, so the n-th dispatch of a kernel name belongs to a
known call.  Criterion: scan + select + compaction together are not slower than gather_kernel of the
same call beyond the spread of the gather's per-round medians.  At cap 128 the call is launch-bound: reported only."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0
H, S, D, W, RECENT, RATIO = 32, 32768, 128, 32, 32, 0.4
CAPS = (4096, 2048, 128)
WARM = 5
KERNELS = ("think_scan_kernel", "think_select_kernel", "think_compact_kernel", "gather_kernel")


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(statistics.median(xs), 2), min=round(xs[0], 2), max=round(xs[-1], 2),
                p25=round(xs[len(xs) // 4], 2), p75=round(xs[(3 * len(xs)) // 4], 2), n=len(xs))


def bytes_moved(cap):
    """Algorithmic bytes per call of the three kernels (e = 2): scan N*D*e (+ 32 query rows), compaction R*D*e + R*(D-k)*e."""
    n_prune = int(D * RATIO)
    R = cap - RECENT
    return dict(scan=H * (cap + 32) * D * 2, compact=H * (R * D + R * (D - n_prune)) * 2, gather=H * 4 * cap * D * 2)


def eager_pruner(kc, q, recent, ratio):
    """The pruner with the reference's ops (pyramidkv_utils.py:13-26), boolean-mask index included, for scale only."""
    import torch
    n, d = kc.shape[2], kc.shape[3]
    k = int(d * ratio)
    score = q[..., -32:, :].pow(2).mean(dim=2) * kc.pow(2).mean(dim=2)
    low = score.topk(k, dim=-1, largest=False).indices.sort().values
    drop = torch.zeros(score.shape, dtype=torch.bool, device=kc.device).scatter_(-1, low, True)
    rows = kc[:, :, :n - recent, :]
    return rows[~drop.unsqueeze(2).expand(-1, -1, n - recent, -1)].reshape(1, -1, n - recent, d - k), kc[:, :, n - recent:, :], ~drop


def timed(fn, reps):
    import torch
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def tensors():
    import torch
    g0 = torch.Generator(device="cuda").manual_seed(0)
    return tuple(torch.randn(1, H, S, D, device="cuda", generator=g0).to(torch.bfloat16) for _ in range(3))


def run_whole(a):
    import torch
    import pyramidkv_amd as P
    q, k, v = tensors()
    res = dict(shape=[1, H, S, D], dtype="bf16", window=W, recent=RECENT, ratio=RATIO, reps=a.reps, rounds=a.rounds,
               device=torch.cuda.get_device_name(0), caps={})
    for cap in CAPS:
        cl = P.SnapKVCluster(window_size=W, max_capacity_prompt=cap, kernel_size=5, pooling="avgpool", recent_size=RECENT, ratio=RATIO)
        rounds = []
        for _ in range(a.rounds):
            t = timed(lambda: cl.update_think(k, q, v, None, 1), a.reps)
            u = timed(lambda: cl.update_kv(k, q, v, None, 1), a.reps)
            rounds.append(dict(update_think=stats(t), update_kv=stats(u)))
        kc, _ = cl.update_kv(k, q, v, None, 1)
        e = timed(lambda: eager_pruner(kc, q, RECENT, RATIO), a.reps)
        p = timed(lambda: P.ops.think_prune(q, kc, RECENT, int(D * RATIO)), a.reps)
        tm = [r["update_think"]["median"] for r in rounds]
        um = [r["update_kv"]["median"] for r in rounds]
        res["caps"][str(cap)] = dict(
            rounds=rounds, update_think_us=statistics.median(tm), update_kv_us=statistics.median(um),
            update_kv_spread_us=round(max(um) - min(um), 2), think_prune_call_us=stats(p), eager_pruner_same_chip_us=stats(e),
            bytes=bytes_moved(cap))
    return res


def run_trace(a):
    """Under rocprofv3: per cap, rounds x (WARM + reps) calls of update_think and nothing else."""
    import torch
    import pyramidkv_amd as P
    q, k, v = tensors()
    for cap in CAPS:
        cl = P.SnapKVCluster(window_size=W, max_capacity_prompt=cap, kernel_size=5, pooling="avgpool", recent_size=RECENT, ratio=RATIO)
        for _ in range(a.rounds * (WARM + a.reps)):
            cl.update_think(k, q, v, None, 1)
        torch.cuda.synchronize()


def fold_trace(a, res):
    files = sorted(glob.glob(os.path.join(a.kernel_trace, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {a.kernel_trace}")
    by = {n: [] for n in KERNELS}
    with open(files[-1]) as f:
        for r in csv.DictReader(f):
            for n in KERNELS:
                if "pkv::" + n in r["Kernel_Name"]:
                    by[n].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    per_cap = a.rounds * (WARM + a.reps)
    for n in KERNELS:
        by[n].sort()
        if len(by[n]) != per_cap * len(CAPS):
            raise SystemExit(f"{n}: {len(by[n])} dispatches in the trace, expected {per_cap * len(CAPS)} (same --reps / --rounds as the traced run?)")
    res["kernel_trace"] = os.path.basename(files[-1])
    for ci, cap in enumerate(CAPS):
        c = res["caps"].setdefault(str(cap), dict(bytes=bytes_moved(cap)))
        rounds = []
        for rd in range(a.rounds):
            lo = ci * per_cap + rd * (WARM + a.reps) + WARM
            us = {n: [d for _, d in by[n][lo:lo + a.reps]] for n in KERNELS}
            us["think_three_kernels"] = [sum(x) for x in zip(*(us[n] for n in KERNELS[:3]))]
            rounds.append({n: stats(x) for n, x in us.items()})
        med = {n: statistics.median(r[n]["median"] for r in rounds) for n in rounds[0]}
        gm = [r["gather_kernel"]["median"] for r in rounds]
        spread = round(max(gm) - min(gm), 2)
        b = c["bytes"]
        c["kernels_us"] = dict(rounds=rounds, median=med, gather_spread_us=spread)
        c["compact_frac_of_8TBs"] = round(b["compact"] / (med["think_compact_kernel"] * 1e-6) / (HBM_TBS * 1e12), 3)
        c["scan_frac_of_8TBs"] = round(b["scan"] / (med["think_scan_kernel"] * 1e-6) / (HBM_TBS * 1e12), 3)
        c["gather_frac_of_8TBs"] = round(b["gather"] / (med["gather_kernel"] * 1e-6) / (HBM_TBS * 1e12), 3)
        c["think_not_slower_than_gather"] = bool(med["think_three_kernels"] <= med["gather_kernel"] + spread)
        c["criterion_applies"] = cap != 128               # cap 128: launch-bound, reported only
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="the kernel-trace workload only (run under rocprofv3)")
    ap.add_argument("--kernel-trace", help="directory of a rocprofv3 --kernel-trace run of --trace: fold it into --out")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.trace:
        run_trace(a)
        return
    if a.kernel_trace:
        if not a.out or not os.path.exists(a.out):
            raise SystemExit("--kernel-trace folds into an existing --out record")
        with open(a.out) as f:
            res = fold_trace(a, json.load(f))
    else:
        res = run_whole(a)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
