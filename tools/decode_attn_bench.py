"""Decode attention over the flat var-len cache: pkv_decode_attn_flat against the eager varlen_decode_attention on the SAME
tensors in the same process, and the error figures the GPU test's bar is made of.

    python tools/decode_attn_bench.py [--reps 200] [--rounds 5] [--graph-reps 50] [--no-graph] [--out FILE] [--error-out FILE]

Shapes: H = 32, D = 128, bf16 - even heads of 128 rows (BASELINE config 5's budget), even heads of 2048 rows, and one head at
8x the others with the 2048-row total.  Two times per shape and function, each the median over --rounds rounds that alternate
the two functions after a warm-up:
  call_us    HIP events around --reps back-to-back calls through the Python wrapper, over --reps: what a decode step pays per
             layer, host issue time included (at these sizes the host is the slower side for both functions);
  device_us  --graph-reps of the same calls captured once into a HIP graph (a linear chain) and replayed four times: device
             time per call, launch gaps included.  "not measured" if the capture is refused.
frac_of_8TBs = the floor (K and V read once) over device_us (call_us where there is none) as a fraction of 8 TB/s.
--error-out: E (the eager function's largest fp32 deviation from float64 in a head, on the device) and this kernel's own worst
deviation per dtype and D on the GPU test's Gaussian inputs, with `decode_attn_ref` from tests/ (the one statement of the bar;
this tool borrows the test helper rather than keeping a second copy)."""
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
from pyramidkv_amd.monkeypatch import varlen_decode_attention  # noqa: E402

HBM_TBS = 8.0
H, D = 32, 128
DEV = "cuda"


def shapes():
    skew_small = (H * 2048) // (H - 1 + 8)
    return {"even_128": [128] * H, "even_2048": [2048] * H,
            "skewed_8x": [H * 2048 - (H - 1) * skew_small] + [skew_small] * (H - 1)}


def batch_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def graph_of(fn, reps):
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # the workspace of this stream exists before the capture
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(reps):
                fn()
        g.replay()
        torch.cuda.synchronize()
        return g
    except Exception as e:                                  # noqa: BLE001
        print("graph capture refused:", repr(e)[:200], file=sys.stderr)
        torch.cuda.synchronize()
        return None


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate())
    except Exception:                                       # noqa: BLE001
        return "not read"


def bench(a):
    res = dict(H=H, D=D, dtype="bf16", reps=a.reps, rounds=a.rounds, graph_reps=a.graph_reps, device=torch.cuda.get_device_name(0), chunk=N.PKV_DECODE_CHUNK,
               sm_clock_mhz_before=clock_mhz(), cases={})
    g0 = torch.Generator(device=DEV).manual_seed(0)
    for name, lens in shapes().items():
        total, mx = sum(lens), max(lens)
        q = torch.randn(H, D, device=DEV, generator=g0).to(torch.bfloat16)
        k = torch.randn(total, D, device=DEV, generator=g0).to(torch.bfloat16)
        v = torch.randn(total, D, device=DEV, generator=g0).to(torch.bfloat16)
        cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
        native = lambda: P.ops.decode_attn_flat(q, k, v, cu, mx, D ** -0.5)                         # noqa: E731
        eager = lambda: varlen_decode_attention(q, k, v, cu, mx, D ** -0.5)                         # noqa: E731
        diff = float((native().float() - eager().float()).abs().max())
        for _ in range(3):
            batch_us(native, a.reps), batch_us(eager, a.reps)
        graphs = {"kernel": None, "eager": None} if a.no_graph else {"kernel": graph_of(native, a.graph_reps), "eager": graph_of(eager, a.graph_reps)}
        t = {"kernel": dict(call=[], device=[]), "eager": dict(call=[], device=[])}
        for _ in range(a.rounds):
            for who, fn in (("kernel", native), ("eager", eager)):
                t[who]["call"].append(batch_us(fn, a.reps))
                if graphs[who] is not None:
                    t[who]["device"].append(batch_us(graphs[who].replay, 4) / a.graph_reps)
        floor = 2 * total * D * 2
        case = dict(lens_max=mx, lens_min=min(lens), rows=total, floor_bytes=floor, splits=N.lib.pkv_decode_attn_splits(H, D, mx),
                    max_abs_diff_vs_eager=diff)
        for who in ("kernel", "eager"):
            call, dev = t[who]["call"], t[who]["device"]
            case[who] = dict(call_us=round(statistics.median(call), 2), call_us_min=round(min(call), 2), call_us_max=round(max(call), 2),
                             device_us=round(statistics.median(dev), 2) if dev else "not measured",
                             device_us_min=round(min(dev), 2) if dev else "not measured",
                             device_us_max=round(max(dev), 2) if dev else "not measured")
            best = statistics.median(dev) if dev else statistics.median(call)
            case[who]["frac_of_8TBs"] = round(floor / (best * 1e-6) / (HBM_TBS * 1e12), 4)
        kd, ed = case["kernel"]["device_us"], case["eager"]["device_us"]
        case["kernel_faster_call"] = bool(case["kernel"]["call_us"] < case["eager"]["call_us"])
        case["kernel_faster_device"] = bool(kd < ed) if isinstance(kd, float) and isinstance(ed, float) else "not measured"
        res["cases"][name] = case
        del graphs, q, k, v
    res["sm_clock_mhz_after"] = clock_mhz()
    return res


def errors():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import decode_attn_ref as R
    C = R.chunk_rows()
    out = dict(chunk=C, lens=[[1, 2, C - 1, C, C + 1], [3 * C + 5, 1, 2 * C, C + 1, 7]], splits=[1, 2, 3, "default"],
               bar="ulp_dtype(|ref|) + 4 E per element; E, dev: largest absolute deviation from float64 over all heads", cases={})
    for dtype, dt in R.DTYPES.items():
        for Dh in (64, 128, 256):
            w = dict(E=0.0, dev=0.0, worst_dev_over_bar=0.0, lse_E=0.0, lse_dev=0.0, worst_lse_dev_over_bar=0.0)
            for i, lens in enumerate(out["lens"]):
                g = torch.Generator().manual_seed(1000 * Dh + 17 * i + len(dtype))                  # the GPU test's inputs
                n = sum(lens)
                q, k, v = (torch.randn(r, Dh, generator=g).to(dt) for r in (len(lens), n, n))
                cu = R.cu_of(lens)
                ref, ref_lse = R.ref_f64(q, k, v, cu, Dh ** -0.5)
                qd, kd, vd, cud = (t.to(DEV) for t in (q, k, v, cu))
                E = R.eager_fp32_deviation(lambda *x: varlen_decode_attention(*x).cpu(), qd, kd, vd, cud, max(lens), Dh ** -0.5, ref)
                El = R.eager_fp32_lse_deviation(qd, kd, cu, Dh ** -0.5, ref_lse)
                bar, lbar = R.out_bar(dt, ref, E), R.lse_bar(ref_lse, El)
                for sp in (1, 2, 3, None):
                    o, l = P.ops.decode_attn_flat(qd, kd, vd, cud, max(lens), Dh ** -0.5, splits=sp, return_lse=True)
                    dev, ldev = (o.cpu().double() - ref).abs(), (l.cpu().double() - ref_lse).abs()
                    for key, val in (("E", E.max()), ("dev", dev.max()), ("worst_dev_over_bar", (dev / bar).max()), ("lse_E", El.max()),
                                     ("lse_dev", ldev.max()), ("worst_lse_dev_over_bar", (ldev / lbar).max())):
                        w[key] = max(w[key], float(val))
            out["cases"][f"{dtype}_D{Dh}"] = {k_: float(f"{x:.4g}") for k_, x in w.items()}
    return out


def write(path, obj):
    txt = json.dumps(obj, indent=1)
    print(txt)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(txt + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--graph-reps", type=int, default=50, help="calls captured into the replayed graph")
    ap.add_argument("--no-graph", action="store_true", help="call_us only")
    ap.add_argument("--out")
    ap.add_argument("--error-out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_attn_bench.py measures on the GPU; there is none here")
    if a.error_out:
        write(a.error_out, errors())
    write(a.out, bench(a))


if __name__ == "__main__":
    main()
