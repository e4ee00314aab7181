"""GPU: every route of the window-score stage (do_score_window, pkv_api.hip: logits2_kernel / logits_kernel instantiations, stages
per workgroup, store modes; finalize_kernel's window constant, positions per thread and halo path), pinned by the shapes of
tests/score_routes.py and checked against the oracle.

  a. the route matrix: one child on the debug library records each case's route (pkv_debug_score_route); it must equal the
     restatement at the device's CU count, and every cell of score_routes.MATRIX must be observed;
  b. parity per case on the release library: scores within score_bar's bar (lattice inputs: also within 1 ulp), indices the
     canonical top-k of the kernel's own scores, K/V the oracle's gather; windows 32 and 64 end to end through SnapKVCluster
     and PyramidKVCluster; Ada-SnapKV at window 32, S = 32768, H = 32 (8 positions per thread) against the oracle's budgets;
  c. stage-count sweep: PKV_LOGITS_V2_WGS = 1 / 3 put many and odd stage counts per workgroup on small prompts;
  d. the documented knobs, one child each: the ones that claim identical results give the default run's bits, the others
     pass the oracle;
  e. more than 4 GiB of logits: st_mode falls back to plain stores; first and last heads against the oracle."""
import json
import os
import subprocess
import sys

import pytest
import torch

from oracle import pkv_oracle as O
from score_bar import check_window_scores
from score_routes import BIG_CASE, CASES, KNOBS, MATRIX, cells, decode, make_inputs, run_case, score_route

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "pyramidkv_amd", "libpkv_debug.so")
BY_NAME = {c[0]: c for c in CASES}


@pytest.fixture(scope="module")
def P():
    import pyramidkv_amd
    return pyramidkv_amd


def _child(mode, env_extra, timeout):
    env = dict(os.environ)
    for n in KNOBS + ["PKV_LIB"]:
        env.pop(n, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "score_routes.py"), mode], capture_output=True, text=True,
                       env=env, timeout=timeout)
    if r.returncode < 0 or r.returncode in (134, 139):         # a fault or an abort: nothing more runs on this device
        pytest.exit("score_routes.py %s %s ended with status %d: %s" % (mode, env_extra, r.returncode, r.stderr[-3000:]), 3)
    assert r.returncode == 0, (mode, env_extra, r.returncode, r.stderr[-3000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


# knob settings the DESIGN.md knob table says give identical results / only change a cache policy, and the ones that reorder
# the statistics (or change the logits kernel) and are held to the oracle's bar
SAME_BITS = {"ppt4": {"PKV_FINALIZE_PPT": "4"}, "ppt8": {"PKV_FINALIZE_PPT": "8"}, "st0": {"PKV_LOGITS_ST": "0"},
             "st1": {"PKV_LOGITS_ST": "1"}, "nt0": {"PKV_LOGITS_NT": "0"}}
ORACLE_BAR = {"fexp0": {"PKV_LOGITS_FEXP": "0"}, "v2_0": {"PKV_LOGITS_V2": "0"}, "tile128": {"PKV_LOGITS_TILE": "128"}}
_RUNS = {}


def _run(name):
    """The child runs, one after another, each at most once per session."""
    if name not in _RUNS:
        if name == "matrix":
            _RUNS[name] = _child("matrix", {"PKV_LIB": DEBUG_LIB}, 600)
        elif name.startswith("sweep_wgs"):
            _RUNS[name] = _child("sweep", {"PKV_LOGITS_V2_WGS": name[len("sweep_wgs"):]}, 300)
        elif name == "knobs_default":
            _RUNS[name] = _child("knobs-digest", {}, 300)
        elif name in SAME_BITS:
            _RUNS[name] = _child("knobs-digest", SAME_BITS[name], 300)
        elif name in ORACLE_BAR:
            _RUNS[name] = _child("knobs", ORACLE_BAR[name], 300)
        elif name == "big":
            _RUNS[name] = _child("big", {"PKV_LIB": DEBUG_LIB}, 600)
    return _RUNS[name]


def _routes_match(out, cases, knobs=None):
    cus = out["cus"]
    seen = set()
    for case in cases:
        r = out["cases"][case[0]]
        assert r["route"] is not None, (case[0], "no route recorded")
        got = decode(r["route"])
        want = score_route(case[1], *case[2:8], knobs=knobs, cus=cus)
        assert got == want, (case[0], "recorded route differs from the restatement at %d CUs" % cus,
                             {k: (got[k], want[k]) for k in got if got[k] != want[k]})
        c = cells(got)
        assert case[-1] <= c, "case %s is off its intended cell(s) %s at this device's %d CUs" % (case[0], sorted(case[-1] - c), cus)
        seen |= c
    return seen


def test_route_matrix_on_the_debug_library(P):
    out = _run("matrix")
    assert out["debug"] is True
    bad = {c: r["why"] for c, r in out["cases"].items() if not r["ok"]}
    assert not bad, bad
    seen = _routes_match(out, CASES)
    print("observed route cells at %d CUs:" % out["cus"], sorted(seen))
    assert MATRIX <= seen, sorted(MATRIX - seen)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_route_case_against_the_oracle(P, name):
    """The case's scores, selection and compacted K/V on the release library (release kernels, main process)."""
    case = BY_NAME[name]
    route, digest, why, rep = run_case(P, O, case)
    assert route is None and not why, why
    print(name, rep)


@pytest.mark.parametrize("name", ["nct2_w32", "ks4_w64_halo"])
def test_window_32_and_64_end_to_end(P, name):
    """SnapKVCluster and PyramidKVCluster (layer 3 of 32) at windows 32 and 64 (finalize_kernel<T, 32, 8> / <T, 0, 8> with the
    halo spread): the kernel's scores within the bar, the caches the oracle's gather of the canonical top-k of those scores."""
    _, dt, B, H, G, S, D, w, pool, ks = BY_NAME[name][:10]
    q, k, v = make_inputs(BY_NAME[name])
    s = P.ops.score_window(q, k, w, pool, ks, "sum")
    qc, kc, vc, sc = q[:, :, -w:].cpu(), k.cpu(), v.cpu(), s.cpu()
    check_window_scores(qc, kc, w, pool, ks, "sum", sc, lambda: P.ops.score_window(q, k, w, None, 1, "sum").cpu(), what=name)
    cap = 2048 + w
    snap = P.SnapKVCluster(window_size=w, max_capacity_prompt=cap, kernel_size=ks, pooling=pool)
    ko, vo = snap.update_kv(k, q, v, None, 1)
    kr, vr = O.gather_compact(kc, vc, O.topk_canonical(sc, cap - w), w)
    assert torch.equal(ko.cpu(), kr) and torch.equal(vo.cpu(), vr), (name, "SnapKVCluster")
    pyr = P.PyramidKVCluster(num_hidden_layers=32, window_size=w, max_capacity_prompt=cap, kernel_size=ks, pooling=pool, layer_idx=3)
    branch, kk = pyr.layer_budget(S)
    assert branch == "pyramid" and kk != cap - w
    ko, vo = pyr.update_kv(k, q, v, None, 1)
    kr, vr = O.gather_compact(kc, vc, O.topk_canonical(sc, kk), w)
    assert torch.equal(ko.cpu(), kr) and torch.equal(vo.cpu(), vr), (name, "PyramidKVCluster")


def test_ada_snapkv_window_32_at_eight_positions_per_thread(P):
    """Ada-SnapKV reads finalize_kernel's per-workgroup fp64 row sums (rowsum_part), whose count follows the positions per
    thread: w = 32, S = 32768, H = 32 runs finalize_kernel<T, 32, 8>.  Budgets = the oracle's on the kernel's scores, flat K/V
    exact."""
    case = ("ada_w32", "bf16", 1, 32, 1, 32768, 128, 32, "maxpool", 7, "mean")
    _, dt, B, H, G, S, D, w, pool, ks = case[:10]
    assert score_route(dt, B, H, G, S, D, w)["ppt"] == 8 and score_route(dt, B, H, G, S, D, w)["fin_w"] == 32
    q, k, v = make_inputs(case)
    sg = P.ops.score_window(q, k, w, pool, ks, "mean")
    qc, kc, vc, sgc = q[:, :, -w:].cpu(), k.cpu(), v.cpu(), sg.cpu()
    check_window_scores(qc, kc, w, pool, ks, "mean", sgc, lambda: P.ops.score_window(q, k, w, None, 1, "mean").cpu(), what="ada")
    base, floor = 120, 0.2
    M = H * base
    for norm in (True, False):
        sidx, caps = O.adakv_head_capacity(sgc, base, floor, norm)
        top, cap, hl, cu, cuh = P.ops.ada_select(q, k, w, pool, ks, M, base, floor, norm)
        assert torch.equal(top.cpu().long(), O.topk_canonical(sgc[0], M)), norm
        assert cap.cpu().tolist() == caps[0].tolist(), (norm, cap.cpu().tolist(), caps[0].tolist())
        cl = P.AdaKVCluster(window_size=w, kernel_size=ks, pooling=pool, max_capacity_prompt=base + w, floor=floor, normalize=norm)
        kf, vf = cl.update_kv(k, q, v)
        kr, vr, _ = O._flat_gather(kc, vc, [sidx[0, h, :int(caps[0, h])] for h in range(H)], w)
        assert torch.equal(kf.cpu(), kr) and torch.equal(vf.cpu(), vr), norm


@pytest.mark.parametrize("wgs", ["1", "3"])
def test_stage_count_sweep(P, wgs):
    out = _run("sweep_wgs" + wgs)
    assert out["debug"] is False and out["knobs"] == {"PKV_LOGITS_V2_WGS": wgs}
    bad = {c: r["why"] for c, r in out["cases"].items() if not r["ok"]}
    assert not bad, bad
    assert len(out["cases"]) >= 20


@pytest.mark.parametrize("knob", sorted(SAME_BITS) + sorted(ORACLE_BAR))
def test_knobs(P, knob):
    base = _run("knobs_default")
    out = _run(knob)
    assert out["debug"] is False and out["knobs"] == {**SAME_BITS, **ORACLE_BAR}[knob]
    assert set(out["cases"]) == set(base["cases"])
    if knob in SAME_BITS:
        diff = [c for c, r in out["cases"].items() if r["digest"] != base["cases"][c]["digest"]]
        assert not diff, (knob, "claims identical results, differs on", diff)
    else:
        bad = {c: r["why"] for c, r in out["cases"].items() if not r["ok"]}
        assert not bad, (knob, bad)
        same = sorted(c for c, r in out["cases"].items() if r["digest"] == base["cases"][c]["digest"])
        print(knob, "bit-identical to the default run on", same, "of", sorted(out["cases"]))


def test_logits_workspace_beyond_4gib(P):
    name, dt, B, H, G, S, D, w = BIG_CASE[:8]
    logits = B * H * w * ((S + 255) // 256 * 256) * 2
    assert logits >= 2 ** 32
    need = 3 * B * H * S * D * 2 + int(1.5 * logits) + 4 * 2 ** 30            # q, k, v + the workspace + slack
    P.ops.release_workspaces()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("the 4 GiB logits case needs %.1f GB of free device memory, %.1f GB are free" % (need / 1e9, free / 1e9))
    out = _run("big")
    assert out["debug"] is True
    r = out["cases"][name]
    assert r["ok"], r["why"]
    seen = _routes_match(out, [BIG_CASE])
    assert decode(r["route"])["st_mode"] == 0 and "st_mode 0" in seen
    print("4 GiB case:", decode(r["route"]), r["rep"])
