"""GPU: every path of pass 1 of the H2O score kernels (h2o_stats_kernel, pkv_h2o.hip: frozen reference point, the repeat after
an overflow - by an infinite lane sum or by the 2^120 threshold after the lane merge -, tracked from the start, short prompt),
pinned by the cases of tests/h2o_routes.py.

  a. the route matrix: one child on the debug library records each case's host words and the path code of every pass-1
     workgroup (pkv_debug_h2o_route, pkv_debug_h2o_rows); the codes must equal h2o_route_plan, the host words their restatement,
     the four counts sum to the pass-1 grid, and every cell of h2o_routes.MATRIX must be observed;
  b. c_row, the output of pass 1, against float64 per case (same child): worst |c_row - c_ref| / u_i at most
     K = 4 x max(worst ratio of the numpy-float32 restatement of the kernel's formulas, 1).  profiles/h2o/crow_error.json holds
     the ratios of both per case, as measured on an MI355X: the float32 restatement is at most 0.563 units
     (repeat_one_row-fp16), so K = 4; the GPU is at most 0.831 on the exact lattice cases (repeat_d256-bf16 and the GQA case)
     and 1.917 overall (legacy_outlier_in_the_look_of_wg0-fp16: Gaussian inputs, whose products are not exact);
  c. scores per case on the release library, in this process: score_bar's bar against the oracle (lattice inputs: within 1 ulp),
     two calls bit-identical, the H2O selection the canonical top-k of the kernel's own scores, K/V the oracle's gather;
  d. the release library refuses both hooks."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from oracle import pkv_oracle as O
from h2o_routes import BY_ID, CASES, MATRIX, WORDS, REPEAT, case_id, case_plan, cells, crow_bar, h2o_route_words, run_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "pyramidkv_amd", "libpkv_debug.so")
_RUNS = {}


@pytest.fixture(scope="module")
def P():
    import pyramidkv_amd
    return pyramidkv_amd


def _child(mode, env_extra, timeout):
    env = dict(os.environ)
    env.pop("PKV_LIB", None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "h2o_routes.py"), mode], capture_output=True, text=True,
                       env=env, timeout=timeout)
    if r.returncode < 0 or r.returncode in (134, 139):         # a fault or an abort: nothing more runs on this device
        pytest.exit("h2o_routes.py %s %s ended with status %d: %s" % (mode, env_extra, r.returncode, r.stderr[-3000:]), 3)
    assert r.returncode == 0, (mode, env_extra, r.returncode, r.stderr[-3000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def _plan(c):
    if case_id(c) not in _RUNS:
        _RUNS[case_id(c)] = case_plan(c)[1]
    return _RUNS[case_id(c)]


def _matrix():
    if "matrix" not in _RUNS:
        _RUNS["matrix"] = _child("matrix", {"PKV_LIB": DEBUG_LIB}, 300)
    return _RUNS["matrix"]


def test_route_matrix_on_the_debug_library(P):
    out = _matrix()
    assert out["debug"] is True
    seen = set()
    for c in CASES:
        cid = case_id(c)
        r = out["cases"][cid]
        assert r["words"] is not None and r["codes"] is not None, (cid, "no route recorded", r["why"])
        got = dict(zip(WORDS, r["words"]))
        want = h2o_route_words(c["dt"], c["B"], c["H"], c["S"], c["D"], c["w"])
        assert {k: got[k] for k in want} == want, (cid, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        plan = _plan(c)
        assert r["codes"] == [p["route"] for p in plan], (cid, "recorded per-workgroup codes differ from the restatement", r["codes"])
        counts = [got[k] for k in ("n_frozen", "n_repeat", "n_wide", "n_short")]
        assert counts == [r["codes"].count(code) for code in (1, 2, 3, 4)], (cid, counts)
        assert sum(counts) == got["stats_grid_x"] * got["stats_grid_y"], (cid, counts)
        seen |= cells(plan, c["D"] // 32)                       # the plan's cells are the observed ones: the codes are equal
    print("observed H2O pass-1 cells:", sorted(seen))
    assert MATRIX <= seen, sorted(MATRIX - seen)
    repeats = [case_id(c) for c in CASES if REPEAT in [p["route"] for p in _plan(c)]]
    assert len(repeats) >= 20 and all(2 in out["cases"][cid]["codes"] for cid in repeats)


def test_c_row_against_float64_on_the_debug_library(P):
    out = _matrix()
    cpu = {cid: r["crow_cpu"] for cid, r in out["cases"].items()}
    gpu = {cid: r["crow_gpu"] for cid, r in out["cases"].items()}
    assert all(v is not None for v in cpu.values()) and all(v is not None for v in gpu.values())
    K = crow_bar(list(cpu.values()))
    print("c_row, worst |delta| / u per case (GPU, float32 restatement):", {cid: (round(gpu[cid], 3), round(cpu[cid], 3)) for cid in gpu})
    print("worst: GPU %.3f, float32 restatement %.3f, bar K = %.3f" % (max(gpu.values()), max(cpu.values()), K))
    assert out["crow_bar"] == K
    bad = {cid: v for cid, v in gpu.items() if not v <= K}
    assert not bad, ("c_row beyond K = %g units" % K, bad)


def test_every_case_passes_on_the_debug_library(P):
    out = _matrix()
    bad = {cid: r["why"] for cid, r in out["cases"].items() if not r["ok"]}
    assert not bad, bad


@pytest.mark.parametrize("cid", sorted(BY_ID))
def test_route_case_scores_on_the_release_library(P, cid):
    """Scores, determinism, selection and compacted K/V of the case on the release kernels (this process)."""
    r = run_case(P, O, BY_ID[cid])
    assert r["words"] is None and r["codes"] is None
    assert r["ok"], r["why"]
    print(cid, r["rep"])


def test_release_library_refuses_the_hooks(P):
    assert P._native.lib.pkv_debug_build() == 0
    arr = (ctypes.c_int32 * len(WORDS))()
    assert P._native.lib.pkv_debug_h2o_route(arr, len(WORDS)) == -5            # PKV_ERR_UNSUPPORTED (include/pkv.h)
    crow = (ctypes.c_float * 4)()
    assert P._native.lib.pkv_debug_h2o_rows(arr, 1, crow, 4) == -5
