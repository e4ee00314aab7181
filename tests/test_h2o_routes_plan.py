"""CPU: the route restatement of tests/h2o_routes.py - every case sits on its intended cells, the cases fill the matrix, every
deciding margin is clear of its threshold, the four legacy outlier inputs take the routes stated in
test_gpu_parity.py::test_h2o_scores_key_norm_outliers, and the c_row bar of tests/test_gpu_h2o_routes.py bites: the float32
restatement of pass 1 passes it, and fails it with one key dropped, one key counted twice, or the reset before the second loop
left out."""
import numpy as np
import pytest

from h2o_routes import (BY_ID, CASES, FROZEN, LEGACY_NAMES, MATRIX, NAMES, REPEAT, WIDE, case_id, case_plan, cells, crow_bar, crow_f32, crow_ratio,
                        crow_ref, crow_unit, h2o_route_words, margins_clear, want_routes)

_PLANS = {}


def _plan(cid):
    """(logits, plan, c_ref, unit, worst ratio of the float32 restatement) of a case, computed once."""
    if cid not in _PLANS:
        c = BY_ID[cid]
        x, plan = case_plan(c)
        cref = crow_ref(x)
        unit = crow_unit(x, cref)
        _PLANS[cid] = (x, plan, cref, unit, crow_ratio(crow_f32(x, c["w"], [r["route"] for r in plan]), cref, unit))
    return _PLANS[cid]


def _case_cells(c):
    ks = c["D"] // 32
    return {n if " " in n else "%s/KS%d" % (n, ks) for n in c["cells"]}


@pytest.mark.parametrize("cid", sorted(BY_ID))
def test_case_is_on_its_cells_with_clear_margins(cid):
    c = BY_ID[cid]
    _, plan, _, _, _ = _plan(cid)
    got = [r["route"] for r in plan]
    assert got == want_routes(c), (cid, [NAMES[r] for r in got])
    assert _case_cells(c) <= cells(plan, c["D"] // 32), (cid, sorted(_case_cells(c) - cells(plan, c["D"] // 32)))
    close = {(r["bh"], r["wg"]): margins_clear(r) for r in plan if margins_clear(r)}
    assert not close, (cid, close)


def test_cases_fill_the_matrix():
    seen = set()
    for c in CASES:
        seen |= cells(_plan(case_id(c))[1], c["D"] // 32)
    assert MATRIX <= seen, sorted(MATRIX - seen)


def test_legacy_outlier_cases_take_the_stated_routes():
    """What test_h2o_scores_key_norm_outliers' four inputs exercise: no repeat anywhere."""
    for dt in ("bf16", "fp16"):
        routes = {n: [r["route"] for r in _plan("legacy_%s-%s" % (n, dt))[1]] for n in LEGACY_NAMES}
        assert routes[LEGACY_NAMES[0]] == [FROZEN] * 10                               # the outlier keys score exactly 0
        assert routes[LEGACY_NAMES[1]] == [WIDE, FROZEN, FROZEN, FROZEN, FROZEN] * 2  # key 7 is inside the 16-key look
        assert routes[LEGACY_NAMES[2]] == [WIDE] * 10 and routes[LEGACY_NAMES[3]] == [WIDE] * 10
        assert max(r["lane_lnz"] for r in _plan("legacy_%s-%s" % (LEGACY_NAMES[0], dt))[1]) < 6.2
        spans = [r["span"] for r in _plan("legacy_%s-%s" % (LEGACY_NAMES[1], dt))[1] if r["route"] == WIDE]
        assert all(390 < s < 405 for s in spans), spans


def test_host_words_restatement():
    assert h2o_route_words("bf16", 1, 1, 1200, 128, 8) == dict(
        dtype=0, KS=4, stats_grid_x=5, stats_grid_y=1, colsum_grid_x=5, colsum_grid_y=1, ntiles=19, t_plain=18, stats_lds=32768,
        colsum_lds=33280, stats_dyn_lds=0, colsum_dyn_lds=0)
    r = h2o_route_words("fp16", 2, 4, 700, 256, 16)                      # 64 KB / 64.5 KB: both passes ask for the LDS opt-in
    assert (r["stats_lds"], r["colsum_lds"], r["stats_dyn_lds"], r["colsum_dyn_lds"], r["KS"], r["dtype"]) == (65536, 66048, 1, 1, 8, 1)
    assert (r["stats_grid_x"], r["stats_grid_y"], r["colsum_grid_x"], r["t_plain"], r["ntiles"]) == (3, 8, 3, 10, 11)
    assert h2o_route_words("bf16", 1, 1, 40, 64, 8)["t_plain"] == 0 and h2o_route_words("bf16", 1, 1, 100, 128, 8)["t_plain"] == 1
    assert h2o_route_words("bf16", 1, 1, 1032, 128, 8)["colsum_grid_x"] == 4 and h2o_route_words("bf16", 1, 1, 1033, 128, 8)["colsum_grid_x"] == 5


def test_the_crow_bar_bites():
    """K = 4 x max(worst ratio of the float32 restatement over all cases, 1).  The restatement is below 1 unit everywhere
    (measured: 0.56), so K = 4; one key of 1200 miscounted in one row moves c_row by ~1e-3 = hundreds of units."""
    worst = {case_id(c): _plan(case_id(c))[4] for c in CASES}
    print("float32 restatement, worst |c_row - c_ref| / u per case:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, "the float32 restatement itself is beyond one unit: the unit is wrong"
    K = crow_bar(list(worst.values()))
    assert K == 4.0
    # (case, first row to look at, key): the row is the first one from there on that no key dominates (maximum logit below 3:
    # every key then holds about 1 / S of the row), in a frozen, a repeating, a ragged and a GQA workgroup; the short prompt's
    # rows all look at the planted key, which is the one miscounted there
    for cid, row, key in (("repeat_wg0-bf16", 300, 500), ("repeat_one_row-fp16", 520, 37), ("frozen_large_Z-bf16", 1100, 1199),
                          ("repeat_d256-fp16", 256, 650), ("repeat_gqa_strided-bf16", 256, 10), ("short-bf16", 5, 20)):
        c = BY_ID[cid]
        x, plan, cref, unit, _ = _plan(cid)
        routes = [r["route"] for r in plan]
        H = x.shape[1]
        bh = 1 if c["data"] == "gqa" else 0                                   # GQA: head 1, whose workgroup 1 repeats
        if cid != "short-bf16":
            row = next(r for r in range(row, c["S"]) if x[bh // H, bh % H, r].max() < 3)
        for mut in ("drop", "twice"):
            r = crow_ratio(crow_f32(x, c["w"], routes, **{mut: (bh, row, key)}), cref, unit)
            print(cid, "row", row, NAMES[routes[bh * ((c["S"] + 255) // 256) + row // 256]], mut, "-> %.0f units" % r)
            assert r > K, (cid, mut, r, K)
    for cid in ("repeat_wg0-bf16", "finite_above_2p120-fp16", "repeat_t_plain1-bf16", "repeat_gqa_strided-fp16"):
        c = BY_ID[cid]
        x, plan, cref, unit, ok = _plan(cid)
        routes = [r["route"] for r in plan]
        assert REPEAT in routes
        r = crow_ratio(crow_f32(x, c["w"], routes, no_reset="all"), cref, unit)
        assert r > K, (cid, "no reset before the second loop", r, K)
        # leaving out the reset of Z alone changes nothing: the second loop starts from m = -inf, and the first rescale of the
        # tracked form sets Z = 0 for such a lane (`Z = m == -inf ? 0 : ...`); the reset of m is what the repeat needs
        assert crow_ratio(crow_f32(x, c["w"], routes, no_reset="Z"), cref, unit) == ok
