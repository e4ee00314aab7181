"""Decode attention over the ThinK cache: pkv_decode_attn_think against the eager think_decode_attention on the SAME tensors in
the same process, against pkv_decode_attn_flat on an unpruned flat cache of the same rows, and the error figures the GPU
test's bar is made of.

    python tools/think_decode_bench.py [--reps 200] [--rounds 5] [--graph-reps 50] [--no-graph] [--out FILE] [--error-out FILE]

Shapes: H = 32, D = 128, bf16, ratio 0.4 (Dk = 77), recent 32, one appended token (T = 33 full-width keys), at cap 128 / 2048 /
4096 (R = cap - 32 pruned keys).  Three functions per shape, alternated over --rounds rounds after a warm-up:
  kernel  ops.decode_attn_think
  eager   think_decode_attention on PyTorch-ROCm (gather, two matmuls, cat, fp32 softmax, cast, matmul)
  flat    ops.decode_attn_flat over R + T full-width rows per head (what the step costs without channel pruning)
Two times per function, each the median over the rounds:
  call_us    HIP events around --reps back-to-back calls through the Python wrapper, over --reps (host issue time included);
  device_us  --graph-reps of the same calls captured once into a HIP graph (a linear chain) and replayed four times: device
             time per call, launch gaps included.  "not measured" if the capture is refused.
frac_of_8TBs = the floor - per head R * Dk * e + T * D * e key bytes and (R + T) * D * e value bytes, read once - over device_us
(call_us where there is none) as a fraction of 8 TB/s; for `flat` the floor is its own, 2 (R + T) D e per head.
kernel_not_slower_than_eager: device_us(kernel) <= device_us(eager) + (max - min of the eager rounds).
--error-out: E (the eager function's largest fp32 deviation from float64 in a head, on the device) and this kernel's own worst
deviation per dtype and D on the GPU test's Gaussian inputs, with `think_decode_ref` from tests/ (the one statement of the bar)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pyramidkv_amd as P  # noqa: E402
from pyramidkv_amd import _native as N  # noqa: E402
from pyramidkv_amd.monkeypatch import think_decode_attention  # noqa: E402
from decode_attn_bench import batch_us, clock_mhz, graph_of, write  # noqa: E402

HBM_TBS = 8.0
H, D, RATIO, RECENT = 32, 128, 0.4, 32
DK = D - int(D * RATIO)
CAPS = (128, 2048, 4096)
DEV = "cuda"
WHO = ("kernel", "eager", "flat")


def bench(a):
    res = dict(H=H, D=D, Dk=DK, dtype="bf16", recent=RECENT, reps=a.reps, rounds=a.rounds, graph_reps=a.graph_reps,
               device=torch.cuda.get_device_name(0), chunk=N.PKV_DECODE_CHUNK, tile_bytes=N.DECODE_TILE_BYTES, sm_clock_mhz_before=clock_mhz(), cases={})
    g0 = torch.Generator(device=DEV).manual_seed(0)
    for cap in CAPS:
        R, T = cap - RECENT, RECENT + 1
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=g0).to(torch.bfloat16)               # noqa: E731
        q, kp, kf, v = rnd(H, D), rnd(H, R, DK), rnd(H, T, D), rnd(H, R + T, D)
        keep = torch.zeros(H, D, dtype=torch.bool, device=DEV)
        keep.scatter_(1, torch.rand(H, D, device=DEV, generator=g0).argsort(1)[:, :DK], True)
        idx = torch.sort(keep.to(torch.uint8), dim=-1, descending=True, stable=True).indices[:, :DK]
        q4, idx4, kp4, kf4, v4 = q[None, :, None, :], idx[None], kp[None], kf[None], v[None]
        k_flat = rnd(H * (R + T), D)
        v_flat = v.reshape(H * (R + T), D)
        cu = torch.arange(H + 1, dtype=torch.int32, device=DEV) * (R + T)
        fns = {"kernel": lambda: P.ops.decode_attn_think(q, keep, kp, kf, v, D ** -0.5),
               "eager": lambda: think_decode_attention(q4, idx4, kp4, kf4, v4, D ** -0.5),
               "flat": lambda: P.ops.decode_attn_flat(q, k_flat, v_flat, cu, R + T, D ** -0.5)}
        diff = float((fns["kernel"]().float() - fns["eager"]()[0, 0].float()).abs().max())
        for _ in range(3):
            for who in WHO:
                batch_us(fns[who], a.reps)
        graphs = {who: None if a.no_graph else graph_of(fns[who], a.graph_reps) for who in WHO}
        t = {who: dict(call=[], device=[]) for who in WHO}
        for _ in range(a.rounds):
            for who in WHO:
                t[who]["call"].append(batch_us(fns[who], a.reps))
                if graphs[who] is not None:
                    t[who]["device"].append(batch_us(graphs[who].replay, 4) / a.graph_reps)
        floor = H * (R * DK + T * D + (R + T) * D) * 2
        case = dict(cap=cap, R=R, T=T, floor_bytes=floor, flat_floor_bytes=H * 2 * (R + T) * D * 2,
                    splits=max(N.lib.pkv_decode_attn_splits(H, D, R + T), 1), max_abs_diff_vs_eager=diff)
        for who in WHO:
            call, dev = t[who]["call"], t[who]["device"]
            case[who] = dict(call_us=round(statistics.median(call), 2), call_us_min=round(min(call), 2), call_us_max=round(max(call), 2),
                             device_us=round(statistics.median(dev), 2) if dev else "not measured",
                             device_us_min=round(min(dev), 2) if dev else "not measured",
                             device_us_max=round(max(dev), 2) if dev else "not measured")
            best = statistics.median(dev) if dev else statistics.median(call)
            fl = case["flat_floor_bytes"] if who == "flat" else floor
            case[who]["frac_of_8TBs"] = round(fl / (best * 1e-6) / (HBM_TBS * 1e12), 4)
        kd, ed, fd = (case[who]["device_us"] for who in WHO)
        measured = all(isinstance(x, float) for x in (kd, ed, fd))
        case["eager_device_spread_us"] = round(case["eager"]["device_us_max"] - case["eager"]["device_us_min"], 2) if measured else "not measured"
        case["kernel_not_slower_than_eager"] = bool(kd <= ed + case["eager_device_spread_us"]) if measured else "not measured"
        case["eager_over_kernel_device"] = round(ed / kd, 2) if measured else "not measured"
        case["kernel_over_flat_device"] = round(kd / fd, 3) if measured else "not measured"
        case["kernel_over_flat_call"] = round(case["kernel"]["call_us"] / case["flat"]["call_us"], 3)
        res["cases"][f"cap_{cap}"] = case
        del graphs, fns
    res["sm_clock_mhz_after"] = clock_mhz()
    return res


def errors():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import think_decode_ref as R
    C = R.chunk_rows()
    Hh = 5
    out = dict(chunk=C, H=Hh, shapes=[list(s) for s in R.shapes(C)], splits=[1, 2, 3, "default"], kept="1, D - int(0.4 D), D - 1, D",
               bar="ulp_dtype(|ref|) + 4 E per element; E, dev: largest absolute deviation from float64 over all heads", cases={})
    for dtype, dt in R.DTYPES.items():
        for Dh in (64, 128, 256):
            w = dict(E=0.0, dev=0.0, worst_dev_over_bar=0.0, lse_E=0.0, lse_dev=0.0, worst_lse_dev_over_bar=0.0)
            for Dk in R.kept_widths(Dh):
                for i, (Rn, Tn) in enumerate(R.shapes(C)):
                    t = R.gauss(Hh, Rn, Tn, Dh, Dk, dt, 1000 * Dh + 17 * i + len(dtype))            # the GPU test's inputs
                    ref, ref_lse = R.ref_f64(*t, Dh ** -0.5)
                    td = tuple(x.to(DEV) for x in t)
                    E, El = R.eager_fp32_deviation(think_decode_attention, *td, Dh ** -0.5, ref, ref_lse)
                    bar, lbar = R.out_bar(dt, ref, E), R.lse_bar(ref_lse, El)
                    for sp in (1, 2, 3, None):
                        o, l = P.ops.decode_attn_think(*td, Dh ** -0.5, splits=sp, return_lse=True)
                        dev, ldev = (o.cpu().double() - ref).abs(), (l.cpu().double() - ref_lse).abs()
                        for key, val in (("E", E.max()), ("dev", dev.max()), ("worst_dev_over_bar", (dev / bar).max()), ("lse_E", El.max()),
                                         ("lse_dev", ldev.max()), ("worst_lse_dev_over_bar", (ldev / lbar).max())):
                            w[key] = max(w[key], float(val))
            out["cases"][f"{dtype}_D{Dh}"] = {k_: float(f"{x:.4g}") for k_, x in w.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--graph-reps", type=int, default=50, help="calls captured into the replayed graph")
    ap.add_argument("--no-graph", action="store_true", help="call_us only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "think_decode", "think_decode_bench.json"))
    ap.add_argument("--error-out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("think_decode_bench.py measures on the GPU; there is none here")
    if a.error_out:
        write(a.error_out, errors())
    write(a.out, bench(a))


if __name__ == "__main__":
    main()
