"""L2Norm timing: the key-norm scan next to the window-score K scan on the SAME K tensor in the same process, and the
per-kernel split of a whole L2NormCluster.update_kv (norm scan, top-k, gather).

    python tools/l2norm_bench.py [--reps 30] [--rounds 3] [--out FILE]
    PKV_LIB=pyramidkv_amd/libpkv_debug.so python tools/l2norm_bench.py --route     # which top-k route the norm rows take

Shapes: [1, 32, 32768, 128] bf16, K expanded (32 KV heads) and un-expanded at g = 4 (8 KV heads), cap 4096 and 2048.
Kernel times are the dispatch's own begin / end timestamps (pkv_prof_*, what rocprofv3 reports), one reading per call; whole
calls are bracketed by HIP events.  Every figure is the median over --reps calls after warm-up; a round = scan and norm
measured back to back, the spread of the K scan's medians over the rounds is what the norm scan is allowed to lose by.
--route decodes the top-k trace word with `decode` from tests/topk_routes.py (the one restatement of the trace layout; this
tool borrows the test helper rather than keeping a second copy)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pyramidkv_amd as P  # noqa: E402
from pyramidkv_amd import _native as N  # noqa: E402

HBM_TBS = 8.0
H, S, D, W = 32, 32768, 128, 8


def per_call(fn, reps, warm=5):
    """-> ({kernel: [us per call]}, [whole-call us per call])"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    kern, whole = {}, []
    for _ in range(reps):
        N.prof_enable(True)
        N.prof_read(True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        for name, (ms, n) in N.prof_read(True).items():
            if n:
                kern.setdefault(name, []).append(ms * 1e3)
        N.prof_enable(False)
        whole.append(a.elapsed_time(b) * 1e3)
    return kern, whole


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(statistics.median(xs), 2), min=round(xs[0], 2), max=round(xs[-1], 2),
                p25=round(xs[len(xs) // 4], 2), p75=round(xs[(3 * len(xs)) // 4], 2), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--route", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = "cuda"
    res = dict(shape=[1, H, S, D], dtype="bf16", reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), cases={})
    g0 = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(1, H, S, D, device=dev, generator=g0).to(torch.bfloat16)
    for g in (1, 4):
        k = torch.randn(1, H // g, S, D, device=dev, generator=g0).to(torch.bfloat16)
        v = torch.randn(1, H // g, S, D, device=dev, generator=g0).to(torch.bfloat16)
        kbytes = k.numel() * 2
        scan = lambda: P.ops.score_window(q, k, W, "maxpool", 7, "sum", kv_group=g)                  # noqa: E731
        norm = lambda: P.ops.compress_l2norm(k, v, 64, kv_group=g)                                   # noqa: E731
        rounds = []
        for _ in range(a.rounds):
            ks, _ = per_call(scan, a.reps)
            kn, _ = per_call(norm, a.reps)
            rounds.append(dict(k_scan=stats(ks["logits"]), norm_scan=stats(kn["l2norm"])))
        sm = [r["k_scan"]["median"] for r in rounds]
        nm = [r["norm_scan"]["median"] for r in rounds]
        case = dict(k_bytes=kbytes, rounds=rounds,
                    k_scan_us=statistics.median(sm), k_scan_spread_us=round(max(sm) - min(sm), 2),
                    norm_scan_us=statistics.median(nm), norm_scan_spread_us=round(max(nm) - min(nm), 2))
        case["k_scan_frac_of_8TBs"] = round(kbytes / (case["k_scan_us"] * 1e-6) / (HBM_TBS * 1e12), 3)
        case["norm_scan_frac_of_8TBs"] = round(kbytes / (case["norm_scan_us"] * 1e-6) / (HBM_TBS * 1e12), 3)
        case["norm_not_slower_than_scan"] = bool(case["norm_scan_us"] <= case["k_scan_us"] + case["k_scan_spread_us"])
        for cap in (4096, 2048):
            cl = P.L2NormCluster(max_capacity_prompt=cap, layer_idx=2, skip_layers=[0, 1])
            kern, whole = per_call(lambda: cl.update_kv(k, q, v, None, g), a.reps)
            case[f"update_kv_cap{cap}"] = dict(whole_call_us=stats(whole), kernels_us={n: stats(x) for n, x in kern.items()},
                                               tokens_per_s=round(S / (statistics.median(whole) * 1e-6)))
            snap = P.SnapKVCluster(window_size=W, max_capacity_prompt=cap, kernel_size=7, pooling="maxpool")
            kern, whole = per_call(lambda: snap.update_kv(k, q, v, None, g), a.reps)
            case[f"snapkv_cap{cap}_for_scale"] = dict(whole_call_us=stats(whole), kernels_us={n: stats(x) for n, x in kern.items()})
        if a.route:
            if N.lib.pkv_debug_build() != 1:
                raise SystemExit("--route needs the debug build: PKV_LIB=pyramidkv_amd/libpkv_debug.so")
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from topk_routes import decode
            trace = torch.zeros(32, dtype=torch.int64, device=dev)
            N.check(N.lib.pkv_debug_topk_trace(trace.data_ptr()), "pkv_debug_topk_trace")
            for cap in (4096, 2048, 64):
                trace.zero_()
                torch.cuda.synchronize()
                P.ops.compress_l2norm(k, v, cap, kv_group=g)
                torch.cuda.synchronize()
                exits, gave = decode(int(trace[14].item()) & 0xffffffffffffffff)
                case[f"topk_route_cap{cap}"] = dict(exits=exits, gave_up=gave)
            N.lib.pkv_debug_topk_trace(None)
        res["cases"]["expanded" if g == 1 else f"unexpanded_g{g}"] = case
        del k, v
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
