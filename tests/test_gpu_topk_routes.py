"""GPU: every selection route of topk_kernel (pkv_topk.hip), plain and ADA, pinned by inputs built for it and checked against the
oracle.

  a. the zero-tied route (R2) under ADA: rows with 64 < C < k positive keys (the sink, 63 distinct normals - wave 0's share of the
     ranking - and one crowded tie group) in fp16 and bf16, repeated launches, against topk_canonical, the three-launch budget path
     and the oracle's budget arithmetic; plus the two rows on which R2 gives up and the full path finishes after the ADA epilogue;
  b. the route matrix: one child process on the debug library (which records the route of row 0) runs tests/topk_routes.py; every
     (route, variant) pair that can exist is observed and every output equals the oracle;
  c. the documented knobs PKV_TOPK_ALGO=0 / PKV_TOPK_CMAX=0 (release library, one child each) give the default run's outputs."""
import json
import os
import subprocess
import sys

import pytest
import torch

from inputs import SC_CROWD, SC_ZERO, check_plan, plan_qkv
from oracle import pkv_oracle as O
from topk_routes import ROUTES, decode, race_plan

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, FLOOR, REPEAT = 8, 0.2, 20


@pytest.fixture(scope="module")
def P():
    import pyramidkv_amd
    return pyramidkv_amd


def _planned_structure(sg, plan, dt):
    """The planned structure is in the kernel's own scores: classes, positive count C, crowd size, zero count."""
    assert check_plan(sg, plan, dt) == []
    s = sg.cpu()
    for h in range(s.shape[0]):
        assert int((s[h] > 0).sum()) == int((plan[h] != SC_ZERO).sum())
        assert int((s[h] == 0).sum()) == int((plan[h] == SC_ZERO).sum())
        crowd = s[h][plan[h] == SC_CROWD]
        assert int((s[h] == crowd[0]).sum()) == int((plan[h] == SC_CROWD).sum())


def _ada_check(P, q, k, v, sg, H, base, M, norm, full):
    """REPEAT launches of pkv_ada_select agree with each other, topk_canonical, the oracle's budgets, the three-launch path (full
    lists) and AdaKVCluster's flat K/V."""
    sgc = sg.cpu()
    sidx, caps = O.adakv_head_capacity(sgc[None], base, FLOOR, norm)
    caps = caps[0].tolist()
    want_top = O.topk_canonical(sgc, M)
    first = None
    for rep in range(REPEAT):
        mirror = torch.zeros(H, dtype=torch.int64).pin_memory()
        top, capd, hl, cu, cuh = P.ops.ada_select(q, k, W, "maxpool", 1, M, base, FLOOR, norm, host_mirror=mirror, host_seq=rep + 1)
        torch.cuda.synchronize()
        words = mirror.tolist()
        assert all((x >> 32) == rep + 1 for x in words)
        assert not any(x & 0x80000000 for x in words), "a head's list ran out: the caller would discard this launch"
        got = (top.cpu(), capd.cpu(), hl.cpu(), cu.cpu())
        if first is None:
            first = got
            assert torch.equal(got[0].long(), want_top), (norm, M)
            assert got[1].tolist() == caps == [x & 0x7fffffff for x in words], (norm, got[1].tolist(), caps)
            assert got[2].tolist() == [c + W for c in caps]
            if full:
                top3 = P.ops.topk(sg, M)
                cap3, hl3, cu3 = P.ops.ada_budget_topm(sg, top3, base, FLOOR, norm, window=W)
                assert torch.equal(top3, top) and torch.equal(cap3, capd) and torch.equal(hl3, hl) and torch.equal(cu3, cu)
        else:
            assert all(torch.equal(a, b) for a, b in zip(got, first)), ("launch %d differs from the first" % rep, norm)
    cl = P.AdaKVCluster(window_size=W, kernel_size=1, pooling="maxpool", max_capacity_prompt=base + W, floor=FLOOR, normalize=norm)
    kf, vf = cl.update_kv(k, q, v)
    kr, vr, _ = O._flat_gather(k, v, [sidx[0, h, :caps[h]].to(k.device) for h in range(H)], W)
    assert torch.equal(kf, kr) and torch.equal(vf, vr), norm


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_ada_zero_tied_rows_repeat_exactly(P, dt):
    """R2 under ADA (the race between the zero walk's miscu[6] and the ranking of a crowded bucket): C = 65 / 200 / 470 positive keys
    per head - H = 4 with full lists (M = H * base = 480, the three-launch path is a second reference) and the config-5 shape
    H = 32, M = 512 (short lists with a host mirror; heads of different C so that the budget ends inside the positive keys)."""
    S, base = 32768, 120
    geos = [(4, 480, (C,), True) for C in (65, 200, 470)] + [(32, 512, (200, 470, 300, 65), False)]
    for gi, (H, M, Cs, full) in enumerate(geos):
        plan = race_plan(H, S - W, Cs, 500 + gi)
        q, k, v, _ = plan_qkv(plan, dt, device=DEV)
        sg = P.ops.score_window(q, k, W, "maxpool", 1, "mean")[0]
        _planned_structure(sg, plan, dt)
        assert all(64 < int((plan[h] != SC_ZERO).sum()) < M for h in range(H))
        for norm in (True, False):
            _ada_check(P, q, k, v, sg, H, base, M, norm, full)
        del q, k, v


def test_ada_zero_tied_route_gives_up_into_the_full_path(P):
    """R2 attempted under ADA + normalize and abandoned (the state reset before the full path, then the epilogue): more than 512
    chunks hold a positive key, most only a subnormal inside zero's histogram bin / a tie group of 600 normals packed into 75
    chunks (a bucket beyond 512 candidates).  Both rows have fewer than k chunks above zero's bin, so R2 is tried."""
    S, H, base, M = 32768, 4, 120, 480
    for seed, kw in ((74, dict(n_tiny=600)), (75, dict(crowd_chunks=75))):
        plan = race_plan(H, S - W, (164,) if "n_tiny" in kw else (664,), seed, **kw)
        q, k, v, _ = plan_qkv(plan, "fp16", device=DEV)
        sg = P.ops.score_window(q, k, W, "maxpool", 1, "mean")[0]
        _planned_structure(sg, plan, "fp16")
        for norm in (True, False):
            _ada_check(P, q, k, v, sg, H, base, M, norm, True)


def _child(env_extra):
    env = dict(os.environ)
    env.pop("PKV_LIB", None)
    env.pop("PKV_TOPK_ALGO", None)
    env.pop("PKV_TOPK_CMAX", None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "topk_routes.py")], capture_output=True, text=True, env=env,
                       timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


_RUNS = {}


def _run(name):
    """The child runs, one after another, each at most once per session."""
    if name not in _RUNS:
        debug = os.path.join(ROOT, "pyramidkv_amd", "libpkv_debug.so")
        env = {"debug": {"PKV_LIB": debug}, "debug_algo0": {"PKV_LIB": debug, "PKV_TOPK_ALGO": "0"},
               "algo0": {"PKV_TOPK_ALGO": "0"}, "cmax0": {"PKV_TOPK_CMAX": "0"}}[name]
        _RUNS[name] = _child(env)
    return _RUNS[name]


# (route, variant) pairs that cannot exist: do_topk refuses the ADA hand-over on rows beyond one workgroup (pkv_api.hip), so the ADA
# instantiation never runs on a segment; R4 under ADA needs the second counter region (`dual`), which only rows of at most 40 960
# keys have, where algo 1 takes R1 - it is reached with PKV_TOPK_ALGO=0 (the debug_algo0 run).
IMPOSSIBLE = {r + "/seg-ada" for r in ROUTES}


def test_route_matrix_on_the_debug_library(P):
    seen, gave = set(), set()
    for run in ("debug", "debug_algo0"):
        out = _run(run)
        assert out["debug"] is True
        bad = [c for c, r in out["cases"].items() if not r["ok"]]
        assert not bad, (run, bad)
        for c, r in out["cases"].items():
            ex, gv = decode(r["word"])
            assert ex, (run, c, "no route recorded")
            seen.update(ex)
            gave.update(gv)
    want = {r + "/plain" for r in ROUTES} | {r + "/ada" for r in ROUTES} | {"R1/seg"}
    print("observed routes:", sorted(seen), "gave up:", sorted(gave))
    assert want <= seen, sorted(want - seen)
    assert {"R1/plain", "R2/plain", "R3/R4/plain", "R1/ada", "R2/ada"} <= gave, sorted(gave)
    out = _run("debug")["cases"]
    # the routes each crafted case was built for (default knobs)
    expect = {"plain:r1": "R1/plain", "plain:r3_unaligned": "R3/plain", "plain:r4_unaligned": "R4/plain",
              "plain:r5_radix": "R5-radix/plain", "plain:r5_bitonic": "R5-bitonic/plain", "plain:r5_rank_short": "R5-rank/plain",
              "plain:r1_gives_up": "R5-rank/plain", "plain:r34_gives_up": "R5-rank/plain", "plain:r2_plain": "R2/plain",
              "plain:r2_c200": "R2/plain"}
    for v in ("ada", "ada_norm"):
        expect.update({v + ":r1_gauss": "R1/ada", v + ":r2_c200": "R2/ada", v + ":r2_c470_bf16": "R2/ada",
                       v + ":r2_gives_up_chunks": "R5-rank/ada", v + ":r2_gives_up_crowd": "R5-rank/ada",
                       v + ":r3_not_dual": "R3/ada", v + ":r5_rank": "R5-rank/ada", v + ":r5_radix": "R5-radix/ada",
                       v + ":r5_bitonic": "R5-bitonic/ada"})
    for c, route in expect.items():
        assert decode(out[c]["word"])[0] == [route], (c, decode(out[c]["word"]))
    for v in ("ada", "ada_norm"):
        for c in ("r2_gives_up_chunks", "r2_gives_up_crowd"):
            assert decode(out[v + ":" + c]["word"])[1] == ["R1/ada", "R2/ada"], (v, c)
    # segments of 32 768 keys, then the top-k of their 3 x 120 winners (2k > nch there: the full path)
    assert decode(out["plain:segmented"]["word"])[0] == ["R1/seg", "R5-rank/plain"]
    # ADA rows through R3/R4 and R4 under ADA: PKV_TOPK_ALGO=0
    a0 = _run("debug_algo0")["cases"]
    assert decode(a0["ada_norm:r1_gauss"]["word"])[0] in (["R3/ada"], ["R4/ada"])
    assert "R4/ada" in seen
    # the inputs of test_gpu_parity.test_topk_rows_that_are_mostly_zero: which reach R2 (each branch of its docstring at least once)
    reach = sorted(c.split(":", 1)[1] for c, r in out.items() if c.startswith("zero_") and "R2/plain" in decode(r["word"])[0])
    print("mostly-zero inputs that reach R2:", len(reach), reach)
    branches = {"fewer positives than k": lambda c: "_npos17_k64_" in c or "_npos1_k64_" in c, "k - 1 positives": lambda c: "_npos119_k120_" in c,
                "k positives": lambda c: "_npos120_k120_" in c, "more than k in fewer than k chunks": lambda c: "_bunched_k120" in c,
                "all zero": lambda c: "_npos0_" in c, "-0.0 among the zeros": lambda c: c.endswith("_negzero") and "_npos0_" not in c,
                "subnormal positives": lambda c: c.endswith("_subnormal"), "negative scores, enough zeros": lambda c: "_negative_zero_walk_" in c}
    for dt in ("fp16", "bf16"):
        mine = [c.split(":", 1)[1] for c, r in out.items() if c.startswith("zero_%s:" % dt) and "R2/plain" in decode(r["word"])[0]]
        for b, f in branches.items():
            assert any(f(c) for c in mine), (b, dt)
        few = decode(out["zero_%s:L32760_negative_too_few_zeros_k120" % dt]["word"])             # too few zeros: R2 tried, full path
        assert few == (["R5-rank/plain"], ["R1/plain", "R2/plain"]), (dt, few)
    assert not IMPOSSIBLE & seen


@pytest.mark.parametrize("knob", ["algo0", "cmax0"])
def test_topk_knobs_give_the_default_outputs(P, knob):
    base = _run("debug")["cases"]
    out = _run(knob)
    assert out["debug"] is False
    bad = [c for c, r in out["cases"].items() if not r["ok"]]
    assert not bad, (knob, bad)
    for c, r in out["cases"].items():
        assert r["digest"] == base[c]["digest"], (knob, c)
