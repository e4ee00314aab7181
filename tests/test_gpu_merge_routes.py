"""GPU: every route of the LOOK-M pivot merge (launch_merge / launch_merge_t / launch_merge_f32_t, pkv_merge.hip: two drop-list
kernels, merge_pivot2_kernel's instantiations, stage counts and data-dependent paths, merge_pivot_kernel, the fp32 kernels, the
bucket fast / ranged paths, merge_scatter_kernel's passes and tails), pinned by the cases of tests/merge_routes.py and checked
against the oracle.

  a. the route matrix: one child on the debug library records each case's route and device flags (pkv_debug_merge_route); the host
     words must equal the restatement at the device's CU count, and every cell of merge_routes.MATRIX must be observed;
  b. parity per case on the release library: the drop list is the complement of the union, merge_bar.check_merge passes (exact
     cases: bit-identical K/V and the oracle's own pivots; fp32: test_gpu_f32.py's bar), planted rows sit on their planted pivot;
  c. the input classes of the pivot arithmetic are the "cls_*" cases of (b): all-negative rows, zero maxima of either sign, a
     tiniest positive maximum, next to ordinary, zero-norm and kept_bad neighbours, in first, prefetched and last stages;
  d. stage sweep: PKV_MERGE_NST = 2 / 3 / 5 x PKV_MERGE_PF = 1 / 2 over the small D = 128 cases, all held to (b)'s checks;
  e. the knobs that claim identical results, one child each, held to the default run's digests (K_m, V_m, drop list, pivots);
  f. the unit-row division in its three forms (pkv_debug_unit_div) against the division, over every 16-bit element and every
     significand of the norm."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from inputs import from_bits
from merge_routes import BY_NAME, CASES, KNOB_CASES, KNOB_MATRIX, KNOBS, MATRIX, WORDS, cells, decode, route_of, run_case, sweep_cases
from oracle import pkv_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "pyramidkv_amd", "libpkv_debug.so")


@pytest.fixture(scope="module")
def P():
    import pyramidkv_amd
    return pyramidkv_amd


def _child(mode, env_extra, timeout):
    env = dict(os.environ)
    for n in KNOBS + ["PKV_LIB"]:
        env.pop(n, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "merge_routes.py"), mode], capture_output=True, text=True,
                       env=env, timeout=timeout)
    if r.returncode < 0 or r.returncode in (134, 139):         # a fault or an abort: nothing more runs on this device
        pytest.exit("merge_routes.py %s %s ended with status %d: %s" % (mode, env_extra, r.returncode, r.stderr[-3000:]), 3)
    assert r.returncode == 0, (mode, env_extra, r.returncode, r.stderr[-3000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


# knob settings the source says give identical results
SAME_BITS = {"pivot2_0": {"PKV_MERGE_PIVOT2": "0"}, "pf2": {"PKV_MERGE_PF": "2"}, "nt0": {"PKV_MERGE_NT": "0"},
             "droplist2_0": {"PKV_MERGE_DROPLIST2": "0"}, "pf2_nt0": {"PKV_MERGE_PF": "2", "PKV_MERGE_NT": "0"}}
SWEEP = [(nst, pf) for nst in (2, 3, 5) for pf in (1, 2)]
_RUNS = {}


def _run(name):
    """The child runs, one after another, each at most once per session."""
    if name not in _RUNS:
        if name == "matrix":
            _RUNS[name] = _child("matrix", {"PKV_LIB": DEBUG_LIB}, 900)
        elif name[0] in ("rel", "dbg"):                     # the knob children: release library (what ships) and debug library (route record)
            env = dict(SAME_BITS.get(name[1], {}), **({"PKV_LIB": DEBUG_LIB} if name[0] == "dbg" else {}))
            _RUNS[name] = _child("knobs-digest", env, 300)
        else:
            nst, pf = name
            _RUNS[name] = _child("sweep", {"PKV_MERGE_NST": str(nst), "PKV_MERGE_PF": str(pf)}, 600)
    return _RUNS[name]


def _routes_match(out, cases, knobs=None):
    cus = out["cus"]
    seen = set()
    for case in cases:
        r = out["cases"][case["name"]]
        assert r["route"] is not None, (case["name"], "no route recorded")
        got = decode(r["route"])
        want = route_of(case, knobs=knobs, cus=cus)
        diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
        assert not diff, (case["name"], "recorded route differs from the restatement at %d CUs: (recorded, restated)" % cus, diff)
        c = cells(got, case["dt"], case["k"] + case["w"])
        if knobs is None:
            assert case["cells"] <= c, "case %s is off its intended cell(s) %s at this device's %d CUs" % (case["name"], sorted(case["cells"] - c), cus)
        seen |= c
    return seen


def test_route_matrix_on_the_debug_library(P):
    out = _run("matrix")
    assert out["debug"] is True
    bad = {c: r["why"] for c, r in out["cases"].items() if not r["ok"]}
    seen = _routes_match(out, CASES)
    print("observed route cells at %d CUs:" % out["cus"], sorted(seen))
    print("moved pivots per case:", {c: r["moved"] for c, r in out["cases"].items() if r["moved"]})
    print("CPU oracle seconds per case (> 5 s):", {c: r["oracle_s"] for c, r in out["cases"].items() if r["oracle_s"] > 5})
    assert MATRIX <= seen, sorted(MATRIX - seen)
    assert not bad, bad


def test_release_library_has_no_route_record(P):
    assert P._native.lib.pkv_debug_build() == 0
    arr = (ctypes.c_int32 * len(WORDS))()
    assert P._native.lib.pkv_debug_merge_route(arr, len(WORDS)) == -5          # PKV_ERR_UNSUPPORTED (include/pkv.h)


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_route_case_against_the_oracle(P, name):
    """The case on the release library (release kernels, main process).  Moved pivots: 0 for the exact cases; a Gaussian case that
    needs merge_bar's allowance prints how many it used."""
    r = run_case(P, O, BY_NAME[name])
    print(name, "moved pivots:", r["moved"], "oracle seconds:", r["oracle_s"])
    assert r["route"] is None and r["ok"], r["why"]


@pytest.mark.parametrize("nst,pf", SWEEP)
def test_stage_sweep(P, nst, pf):
    out = _run((nst, pf))
    assert out["debug"] is False and out["knobs"] == {"PKV_MERGE_NST": str(nst), "PKV_MERGE_PF": str(pf)}
    bad = {c: r["why"] for c, r in out["cases"].items() if not r["ok"]}
    assert not bad, bad
    assert set(out["cases"]) == {c["name"] for c in sweep_cases()}
    print("nst", nst, "pf", pf, "moved pivots:", {c: r["moved"] for c, r in out["cases"].items() if r["moved"]})


@pytest.mark.parametrize("knob", sorted(SAME_BITS))
def test_knobs_reproduce_the_default_bits(P, knob):
    """Each knob on the release library (the kernels that ship) and on the debug library (whose route record shows that the knob took
    effect): both reproduce the release library's default digests on every knob case, the Gaussian ones included."""
    base = _run(("rel", "default"))
    assert base["debug"] is False and base["knobs"] == {} and set(base["cases"]) == set(KNOB_CASES)
    for lib in ("rel", "dbg"):
        out = _run((lib, knob))
        assert out["debug"] is (lib == "dbg") and out["knobs"] == SAME_BITS[knob] and set(out["cases"]) == set(KNOB_CASES)
        diff = [c for c, r in out["cases"].items() if r["digest"] != base["cases"][c]["digest"]]
        assert not diff, (knob, lib, "claims identical results, differs on", diff)
    _routes_match(_run(("dbg", knob)), [BY_NAME[n] for n in KNOB_CASES], knobs=SAME_BITS[knob])


def test_knob_children_fill_their_cells(P):
    seen = set()
    for knob in ["default"] + sorted(SAME_BITS):
        out = _run(("dbg", knob))
        if knob == "default":
            base = _run(("rel", "default"))
            diff = [c for c, r in out["cases"].items() if r["digest"] != base["cases"][c]["digest"]]
            assert not diff, ("the debug library's results differ from the release library's on", diff)
        seen |= _routes_match(out, [BY_NAME[n] for n in KNOB_CASES], knobs=SAME_BITS.get(knob, {}))
    print("cells of the knob children:", sorted(seen & KNOB_MATRIX))
    assert KNOB_MATRIX <= seen, sorted(KNOB_MATRIX - seen)


def _unit_div(P, dt, x16, n16):
    dev = torch.device("cuda", torch.cuda.current_device())
    xd, nd = torch.from_numpy(x16.view(np.int16)).to(dev), torch.from_numpy(n16.view(np.int16)).to(dev)
    outs = [torch.empty_like(xd) for _ in range(3)]
    ok = torch.empty(xd.numel(), dtype=torch.uint8, device=dev)
    P._native.check(P._native.lib.pkv_debug_unit_div(P._native.dtype_code(dt), xd.data_ptr(), nd.data_ptr(), outs[0].data_ptr(),
                                                     outs[1].data_ptr(), outs[2].data_ptr(), ok.data_ptr(), xd.numel(), P._native.stream_ptr()),
                    "pkv_debug_unit_div")
    torch.cuda.synchronize()
    return [o.cpu().numpy().view(np.uint16) for o in outs] + [ok.cpu().numpy()]


@pytest.mark.parametrize("dtn", ["bf16", "fp16"])
def test_unit_row_division_exhaustive(P, dtn):
    """dtype(x / n) for every 16-bit x against every significand of the norm n at a middle exponent, and against the extreme
    exponents, subnormal, zero and non-finite norms, in the three forms the merge kernels use (pkv_common.hpp), compared with
    (x.float() / n.float()).to(dtype) on the CPU:
      unit_div (merge_targets_kernel)             on every pair, bit for bit;
      unit_div_const (both pivot kernels)         on every pair a dropped row can hold: a finite element with |x| <= 1.01 n (the norm
                                                  is at least the largest element, up to its own rounding) and a finite norm of
                                                  at least 2^-75: the square root of an fp32 sum of squares is zero or at least
                                                  2^-74.5, so a bf16 norm below that, where 1/n overflows, cannot occur, and a zero
                                                  norm makes the row "bad" (its similarities are NaN in the reference too: 0/0
                                                  among its elements).  Zeros are compared by value: div_const gives
                                                  +0 for a -0 element, which cannot reach a similarity (the MFMA accumulates from +0);
      unit_mul (merge_pivot2_kernel, bf16 only)   on the same pairs wherever the kernel's guard lets a lane take it.
    The pairs outside (quotients that overflow, a norm of +inf - an fp16 row longer than 65504 gives NaN here and zeros in the
    reference, DESIGN.md known deviations) are counted and printed, not asserted."""
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[dtn]
    mant, ebits = (7, 8) if dtn == "bf16" else (10, 5)
    emax = (1 << ebits) - 1
    sig = np.arange(1 << mant, dtype=np.uint32)
    norms = np.concatenate([sig | ((emax // 2) << mant),                    # every significand at a middle exponent
                            sig[::max(1, len(sig) // 64)] | (1 << mant), sig[::max(1, len(sig) // 64)] | ((emax - 1) << mant),   # extreme exponents
                            sig[:: max(1, len(sig) // 32)],                 # zero and subnormals
                            np.array([emax << mant, (emax << mant) | 1, 0x8000, 1, (1 << mant) - 1, (1 << mant), ((emax - 1) << mant) | ((1 << mant) - 1)], dtype=np.uint32)
                            ]).astype(np.uint16)
    xs = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    bad_div = bad_divc = bad_mul = n_mul = outside = 0
    first = {}
    for c0 in range(0, len(norms), 64):
        nn = norms[c0:c0 + 64]
        x16, n16 = np.tile(xs, len(nn)), np.repeat(nn, len(xs))
        xf, nf = from_bits(x16, dt).float(), from_bits(n16, dt).float()
        want = (xf / nf).to(dt)
        wb = want.view(torch.int16).numpy().view(np.uint16)
        wnan = torch.isnan(want).numpy()
        div, divc, mul, ok = _unit_div(P, dt, x16, n16)
        is_nan = (lambda a: torch.isnan(from_bits(a, dt)).numpy())
        same = lambda a: (a == wb) | (wnan & is_nan(a))     # noqa: E731
        samev = lambda a: same(a) | (((a | wb) & 0x7fff) == 0)     # noqa: E731  (zeros by value)
        in_row = (torch.isfinite(xf) & (xf.abs() <= nf * 1.01) & torch.isfinite(nf) & (nf >= 2.0 ** -75)).numpy()
        for name, miss in (("div", ~same(div)), ("divc", ~samev(divc) & in_row), ("mul", ~samev(mul) & in_row & (ok == 1))):
            if miss.any() and name not in first:
                i = int(np.argmax(miss))
                first[name] = (hex(int(x16[i])), hex(int(n16[i])), hex(int(wb[i])), hex(int({"div": div, "divc": divc, "mul": mul}[name][i])))
        bad_div += int((~same(div)).sum())
        bad_divc += int((~samev(divc) & in_row).sum())
        bad_mul += int((~samev(mul) & in_row & (ok == 1)).sum())
        n_mul += int((in_row & (ok == 1)).sum())
        outside += int((~same(divc) & ~in_row).sum())
        # the guard: a lane may multiply iff its norm is a finite normal number
        normal = (torch.isfinite(nf) & (nf >= 2.0 ** -126)).numpy()
        assert np.array_equal(ok == 1, normal), dtn
    print(dtn, "pairs:", len(norms) * 65536, "multiply allowed on", n_mul, "mismatches div / div_const / mul:", bad_div, bad_divc, bad_mul, first,
          "div_const off the division on pairs no row can hold:", outside)
    assert bad_div == 0 and bad_divc == 0, (dtn, first)
    if dtn == "bf16":
        assert bad_mul == 0 and n_mul > 0, (dtn, first)
