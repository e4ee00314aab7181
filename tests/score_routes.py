"""The route matrix of the window-score stage (tests/test_gpu_score_routes.py, tests/test_score_routes_plan.py).

``score_route`` restates, in plain Python, the choices do_score_window (pyramidkv_amd/csrc/pkv_api.hip), launch_logits2,
launch_logits, finalize_ppt and launch_finalize (pkv_score.hip) make for a shape, the knobs and the device's CU count.  Its
keys are the words of the debug library's route record (pkv_debug_score_route, include/pkv.h), in that order.

Run as a child process, ``python tests/score_routes.py MODE`` prints one JSON object: per case the route the debug library
recorded (None on the release library), a digest of the scores, indices and compacted K/V, and whether they pass the oracle
(score_bar.check_window_scores, the canonical top-k of the kernel's own scores, O.gather_compact).  MODE: ``matrix`` (CASES),
``sweep`` (sweep_cases(), for the PKV_LOGITS_V2_WGS runs), ``knobs`` (KNOB_CASES; ``knobs-digest``: digests only, no oracle) or
``big`` (BIG_CASE, first and last heads)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

WORDS = ["kernel", "variant", "tile", "lds_optin", "nst", "nT", "last_nh", "straddle_stage", "straddle_wg", "st_mode",
         "fin_w", "ppt", "halo_spread", "fin_blocks", "nt_load", "fexp"]
KNOBS = ["PKV_LOGITS_TILE", "PKV_LOGITS_NT", "PKV_LOGITS_V2", "PKV_LOGITS_V2_WGS", "PKV_LOGITS_FEXP", "PKV_LOGITS_ST",
         "PKV_FINALIZE_PPT"]


def _cdiv(a, b):
    return -(-a // b)


def score_route(dtype, B, H, G, S, D, w, knobs=None, cus=256):
    """-> {word: int} for a bf16 / fp16 window-score call (un-expanded K: G = kv_group)."""
    env = {n: int(v) for n, v in (knobs or {}).items() if str(v) != ""}   # env_int: unset or empty = the default
    r = dict.fromkeys(WORDS, 0)
    assert dtype in ("bf16", "fp16")
    C = G * w
    Sp = _cdiv(S, 256) * 256
    # do_score_window
    tile = 128 if D == 256 else (128 if env.get("PKV_LOGITS_TILE", 256) == 128 else 256)
    if env.get("PKV_LOGITS_V2", 1) and C <= 32 and D == 128:
        sph = _cdiv(S, 128)
        total = B * (H // G) * sph
        wgs = env.get("PKV_LOGITS_V2_WGS", 0)
        target = wgs if wgs > 0 else (4 * cus if C > 8 else (4 * cus if 4 * cus < total <= 8 * cus else total))
        nst = max(1, min(_cdiv(total, target), min(sph, 64)))
        r["nst"] = nst
        r["nT"] = _cdiv(sph, nst)
        r["nt_load"] = 1 if env.get("PKV_LOGITS_NT", 1) else 0
        r["fexp"] = env.get("PKV_LOGITS_FEXP", 1)
        r["st_mode"] = env.get("PKV_LOGITS_ST", 2) if B * H * w * Sp * 2 < 0xffffffff else 0
        L, span = S - w, nst * 128
        r["last_nh"] = min(nst, _cdiv(S - (r["nT"] - 1) * span, 128))
        r["straddle_stage"] = int(L // 128 != (S - 1) // 128)
        r["straddle_wg"] = int(L // span != (S - 1) // span)
        # launch_logits2
        r["kernel"] = 1
        r["variant"] = 0 if (w == 8 and G == 1) else (1 if _cdiv(C, 16) == 1 else 2)
    else:
        # launch_logits
        r["kernel"] = 2
        r["variant"] = {64: 2, 256: 8}.get(D, 4)
        r["tile"] = tile
        r["lds_optin"] = int(C * (tile + 8) * 2 > 64 * 1024)
        r["nT"] = _cdiv(S, tile)
        r["nt_load"] = 1 if env.get("PKV_LOGITS_NT", 0) else 0
    # finalize_ppt, launch_finalize
    forced = env.get("PKV_FINALIZE_PPT", 0)
    ppt = forced if forced in (4, 8) else (8 if B * H * _cdiv(S - w, 2048) >= 512 else 4)
    r["ppt"] = ppt
    r["fin_blocks"] = _cdiv(S - w, 256 * ppt)
    r["fin_w"] = w if w in (8, 32) else 0
    r["halo_spread"] = int((w & (w - 1)) == 0 and w <= 64)
    return r


def decode(words):
    return dict(zip(WORDS, words))


def cells(r):
    """The cells of the route matrix a route fills."""
    out = set()
    if r["kernel"] == 1:
        out.add("logits2/" + ("WG(8,1)", "NCT1", "NCT2")[r["variant"]])
        out.add("nst=1" if r["nst"] == 1 else "nst>=2")
        if r["nst"] >= 2:
            if r["last_nh"] < r["nst"]:
                out.add("ragged workgroup (nh < nst)")
            if r["straddle_stage"]:
                out.add("window straddles a stage")
            if r["straddle_wg"]:
                out.add("window straddles a workgroup")
        if r["nst"] == 64:
            out.add("nst = 64 (cap)")
        out.add("st_mode %d" % r["st_mode"])
    else:
        out.add("logits/KS%d/tile%d%s" % (r["variant"], r["tile"], "/lds>64K" if r["lds_optin"] else ""))
    out.add("finalize W%d/PPT%d" % (r["fin_w"], r["ppt"]))
    if r["fin_w"] == 0:
        out.add("finalize W0/" + ("halo spread" if r["halo_spread"] else "no halo spread"))
    return out


# (name, dtype, B, H, G, S, D, w, pool, kernel, reduce, cells it is built for at 256 CUs)
# Pooling kernel 17 reaches 8 positions (FN_HALO): a pooled window crosses finalize's 2048-position block boundaries.
CASES = [
    ("wg81_ragged", "bf16", 1, 32, 1, 6403, 128, 8, "maxpool", 17, "sum",
     {"logits2/WG(8,1)", "ragged workgroup (nh < nst)", "window straddles a stage", "window straddles a workgroup", "finalize W8/PPT4"}),
    ("nct2_w32", "fp16", 1, 32, 1, 31003, 128, 32, "avgpool", 17, "sum",
     {"logits2/NCT2", "ragged workgroup (nh < nst)", "window straddles a stage", "finalize W32/PPT8"}),
    ("nct1_w16", "bf16", 1, 32, 1, 30979, 128, 16, "maxpool", 17, "mean",
     {"logits2/NCT1", "ragged workgroup (nh < nst)", "window straddles a stage", "finalize W0/PPT8"}),
    ("gqa4_nst3", "fp16", 2, 32, 4, 20483, 128, 8, "maxpool", 7, "sum",
     {"logits2/NCT2", "ragged workgroup (nh < nst)", "window straddles a stage", "finalize W8/PPT8"}),
    ("b64_s600", "bf16", 64, 32, 1, 600, 128, 16, "avgpool", 5, "mean", {"logits2/NCT1", "nst>=2", "finalize W0/PPT8"}),
    ("b8_cap64", "fp16", 8, 32, 1, 32768, 128, 32, "maxpool", 17, "sum", {"logits2/NCT2", "nst = 64 (cap)", "finalize W32/PPT8"}),
    ("ks4_w64_halo", "bf16", 1, 32, 1, 32771, 128, 64, "maxpool", 17, "sum",
     {"logits/KS4/tile256", "finalize W0/PPT8", "finalize W0/halo spread"}),
    ("ks4_w48_nohalo", "fp16", 1, 32, 1, 32800, 128, 48, "avgpool", 17, "mean",
     {"logits/KS4/tile256", "finalize W0/PPT8", "finalize W0/no halo spread"}),
    ("ks8_d256", "bf16", 1, 32, 1, 32768, 256, 8, "maxpool", 7, "sum", {"logits/KS8/tile128", "finalize W8/PPT8"}),
    ("ks2_d64", "fp16", 1, 32, 1, 32768, 64, 8, "avgpool", 5, "sum", {"logits/KS2/tile256", "finalize W8/PPT8"}),
    # 128 columns x 264 keys x 2 bytes: logits_kernel asks for more than 64 KB of dynamic LDS
    ("ks4_lds_optin", "bf16", 1, 32, 2, 4100, 128, 64, "maxpool", 7, "sum", {"logits/KS4/tile256/lds>64K", "finalize W0/PPT4"}),
    ("nst1_w32_ppt4", "fp16", 1, 8, 1, 3000, 128, 32, "maxpool", 17, "sum", {"logits2/NCT2", "nst=1", "finalize W32/PPT4"}),
]
# every cell at the default knobs: what the cases are built for, the default store mode and single-stage workgroups
MATRIX = set().union(*(c[-1] for c in CASES)) | {"st_mode 2", "nst>=2"}

# one case with B * H * w * Sp * 2 >= 2^32 bytes of logits: st_mode falls back to plain stores (32-bit raw-buffer extent)
BIG_CASE = ("logits_4g", "bf16", 1, 32, 1, 2 ** 21 + 100, 128, 32, "maxpool", 7, "sum",
            {"logits2/NCT2", "nst = 64 (cap)", "ragged workgroup (nh < nst)", "st_mode 0", "finalize W32/PPT8"})


def sweep_cases():
    """The C <= 32, D = 128 shapes of test_gpu_small_shapes.SHAPES (B = 2, H = 4, G = 2 at odd S as there) and the small cases
    of CASES, for the runs with PKV_LOGITS_V2_WGS = 1 / 3 (many stages per workgroup, odd splits)."""
    from test_gpu_small_shapes import SHAPES
    out = []
    for i, (S, w) in enumerate(SHAPES):
        G = 2 if S % 2 else 1
        if G * w <= 32:
            pool, ks = (("maxpool", 17), ("avgpool", 17), ("maxpool", 7))[i % 3]
            out.append(("S%d_w%d" % (S, w), ("bf16", "fp16")[i % 2], 2, 4, G, S, 128, w, pool, ks, "mean" if i % 4 == 3 else "sum", set()))
    # heads of 65 stages: at 64 stages per workgroup the second workgroup holds the last stage, and the window crosses into it
    out += [("S8195_w8", "fp16", 1, 4, 1, 8195, 128, 8, "avgpool", 17, "sum", set()),
            ("S8200_w16_g2", "bf16", 1, 4, 2, 8200, 128, 16, "maxpool", 17, "mean", set())]
    return out + [c for c in CASES if c[2] * c[3] * c[5] <= 1 << 21 and c[4] * c[7] <= 32 and c[6] == 128]


KNOB_CASES = ["wg81_ragged", "gqa4_nst3", "b64_s600", "ks4_w64_halo", "ks2_d64", "nst1_w32_ppt4"]


def make_inputs(case, dev="cuda"):
    """Lattice q/k/v generated on the device from a seed of the case name: every q.k is exact in fp32 in any order.
    -> (q, k un-expanded, v un-expanded) on `dev`."""
    name, dt, B, H, G, S, D = case[:7]
    tdt = torch.bfloat16 if dt == "bf16" else torch.float16
    g = torch.Generator(device=dev).manual_seed(sum(map(ord, name)) * 7919 + S)

    def lattice(shape):
        t = torch.empty(shape, dtype=tdt, device=dev)
        flat = t.view(-1, shape[-1])
        step = max(1, (1 << 27) // shape[-1])
        for r0 in range(0, flat.shape[0], step):                  # int8 draws in slabs: a small peak beside the tensor
            x = torch.randint(-4, 5, (min(step, flat.shape[0] - r0), shape[-1]), generator=g, device=dev, dtype=torch.int8)
            flat[r0:r0 + x.shape[0]] = x.to(tdt) / 4
        return t

    return lattice((B, H, S, D)), lattice((B, H // G, S, D)), lattice((B, H // G, S, D))


def window_scores_f64(q, kx, w, reduce):
    """O.window_scores with the softmax evaluated in fp64 (the probabilities still rounded to the model dtype, the rows reduced as
    there).  At 2^21 keys the fp32 normaliser of the CPU softmax is itself ~1e-7 off: it moves 0.4-0.6 % of the bf16 scores
    by a unit, while the kernel's scores equal this reference."""
    from oracle import pkv_oracle as O
    p = torch.softmax(O.window_logits(q, kx, w).double(), dim=-1).to(q.dtype)[..., :-w]
    return p.sum(dim=-2) if reduce == "sum" else p.mean(dim=-2)


def run_case(P, O, case, check=True, heads=None):
    """Scores (the case's reduce), the sum-reduced scores, compress -> (record of the sum-reduced call or None, digest, failure
    message or "", score report).  ``heads``: check only these heads against the oracle (copying only them to the host)."""
    import numpy as np
    from inputs import checksum
    from score_bar import check_window_scores, ord16
    name, dt, B, H, G, S, D, w, pool, ks, reduce = case[:11]
    debug = P._native.lib.pkv_debug_build() == 1
    q, k, v = make_inputs(case)
    s_red = P.ops.score_window(q, k, w, pool, ks, reduce, kv_group=G)
    s_sum = s_red if reduce == "sum" else P.ops.score_window(q, k, w, pool, ks, "sum", kv_group=G)
    route = None
    if debug:
        import ctypes
        arr = (ctypes.c_int32 * len(WORDS))()
        P._native.check(P._native.lib.pkv_debug_score_route(arr, len(WORDS)), "pkv_debug_score_route")
        route = list(arr)
    kk = min(S - w, 480)
    kc, vc, idx = P.ops.compress(q, k, v, w, kk, pool, ks, kv_group=G, return_indices=True)
    torch.cuda.synchronize()
    digest = checksum(s_red, s_sum, idx, kc, vc) if heads is None else checksum(s_sum[:, heads], idx[:, heads], kc[:, heads])
    if not check:
        return route, digest, "", {}
    hs = list(range(H)) if heads is None else heads
    why, rep = "", {}
    try:
        qt = q[:, hs, -w:].cpu()
        kh = [h // G for h in hs]
        ke, ve = k[:, kh].cpu(), v[:, kh].cpu()
        for red, got in ((reduce, s_red), ("sum", s_sum)) if reduce != "sum" else (("sum", s_sum),):
            gotc = got[:, hs].cpu()
            if heads is not None:                                   # the long-row case: the fp64 reference, within 1 ulp
                d = np.abs(ord16(gotc) - ord16(O.pool_scores(window_scores_f64(qt, ke, w, red), pool, ks)))
                d32 = np.abs(ord16(gotc) - ord16(O.pool_scores(O.window_scores(qt, ke, w, red), pool, ks)))
                rep[red] = dict(mismatch_frac=float((d > 0).mean()), max_ulp=int(d.max()),
                                fp32_oracle_mismatch_frac=float((d32 > 0).mean()), fp32_oracle_max_ulp=int(d32.max()))
                assert rep[red]["max_ulp"] <= 1 and rep[red]["mismatch_frac"] <= 2e-3, (name, red, rep[red])
                continue
            rep[red] = check_window_scores(qt, ke, w, pool, ks, red, gotc,
                                           lambda red=red: P.ops.score_window(q, k, w, None, 1, red, kv_group=G)[:, hs].cpu(),
                                           what="%s %s" % (name, red))
            assert rep[red]["max_ulp"] <= 1, (name, red, "lattice inputs: beyond 1 ulp", rep[red])
        sc = s_sum[:, hs].cpu()
        ic = idx[:, hs].cpu().long()
        assert torch.equal(ic, O.topk_canonical(sc, kk)), (name, "indices are not the canonical top-k of the kernel's scores")
        kr, vr = O.gather_compact(ke, ve, ic, w)
        assert torch.equal(kc[:, hs].cpu(), kr) and torch.equal(vc[:, hs].cpu(), vr), (name, "compacted K/V")
    except AssertionError as e:
        why = repr(e)[:1500]
    return route, digest, why, rep


def main():
    mode = sys.argv[1]
    import pyramidkv_amd as P
    from oracle import pkv_oracle as O
    knob_cases = [c for c in CASES if c[0] in KNOB_CASES]
    cases = {"matrix": CASES, "sweep": sweep_cases(), "knobs": knob_cases, "knobs-digest": knob_cases, "big": [BIG_CASE]}[mode]
    props = torch.cuda.get_device_properties(0)
    res = {}
    for case in cases:
        heads = [0, case[3] - 1] if mode == "big" else None
        route, digest, why, rep = run_case(P, O, case, check=mode != "knobs-digest", heads=heads)
        res[case[0]] = {"route": route, "digest": digest, "ok": not why, "why": why, "rep": rep}
        torch.cuda.empty_cache()
    print(json.dumps({"debug": P._native.lib.pkv_debug_build() == 1, "cus": props.multi_processor_count,
                      "knobs": {n: os.environ.get(n) for n in KNOBS if os.environ.get(n) is not None}, "cases": res}))


if __name__ == "__main__":
    main()
