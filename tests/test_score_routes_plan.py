"""CPU: the route restatement of tests/score_routes.py at 256 CUs - each case is on the route its comment names, the cases
together fill every cell of the matrix, and the knobs and clamps of do_score_window / finalize_ppt move a route the way the
C++ says."""
from score_routes import BIG_CASE, CASES, KNOB_CASES, MATRIX, cells, score_route, sweep_cases


def _route(case, knobs=None, cus=256):
    return score_route(case[1], *case[2:8], knobs=knobs, cus=cus)


def test_every_case_is_on_its_intended_cells():
    for case in CASES + [BIG_CASE]:
        got = cells(_route(case))
        assert case[-1] <= got, (case[0], sorted(case[-1] - got))


def test_the_cases_fill_every_cell():
    seen = set().union(*(cells(_route(c)) for c in CASES))
    assert seen == MATRIX, sorted(seen ^ MATRIX)
    assert {"logits2/WG(8,1)", "logits2/NCT1", "logits2/NCT2", "logits/KS2/tile256", "logits/KS4/tile256", "logits/KS8/tile128",
            "logits/KS4/tile256/lds>64K", "ragged workgroup (nh < nst)", "window straddles a stage", "window straddles a workgroup",
            "nst = 64 (cap)", "finalize W0/halo spread", "finalize W0/no halo spread"} <= MATRIX
    assert {"finalize W%d/PPT%d" % (w, p) for w in (8, 32, 0) for p in (4, 8)} <= MATRIX


def test_the_issue_table_rows():
    """(nst, chunks, stages of the last workgroup) and the finalize form of each row of the case table."""
    want = {"wg81_ragged": (2, 26, 1, 8, 4), "nct2_w32": (8, 31, 3, 32, 8), "nct1_w16": (8, 31, 3, 0, 8), "gqa4_nst3": (3, 54, 2, 8, 8),
            "b64_s600": (5, 1, 5, 0, 8), "b8_cap64": (64, 4, 64, 32, 8)}
    by = {c[0]: c for c in CASES}
    for name, (nst, nT, last, fw, ppt) in want.items():
        r = _route(by[name])
        assert (r["kernel"], r["nst"], r["nT"], r["last_nh"], r["fin_w"], r["ppt"]) == (1, nst, nT, last, fw, ppt), (name, r)
    r = _route(by["wg81_ragged"])
    assert r["straddle_stage"] and r["straddle_wg"] and r["variant"] == 0
    for name in ("nct2_w32", "nct1_w16", "gqa4_nst3"):
        r = _route(by[name])
        assert r["straddle_stage"] and not r["straddle_wg"], name
    r = _route(by["ks4_w64_halo"])
    assert (r["kernel"], r["variant"], r["tile"], r["fin_w"], r["ppt"], r["halo_spread"]) == (2, 4, 256, 0, 8, 1)
    r = _route(by["ks4_w48_nohalo"])
    assert (r["kernel"], r["variant"], r["tile"], r["fin_w"], r["ppt"], r["halo_spread"]) == (2, 4, 256, 0, 8, 0)
    assert (_route(by["ks8_d256"])["variant"], _route(by["ks8_d256"])["tile"]) == (8, 128)
    assert (_route(by["ks2_d64"])["variant"], _route(by["ks2_d64"])["tile"]) == (2, 256)


def test_the_4gib_case_falls_back_to_plain_stores():
    name, dt, B, H, G, S, D, w = BIG_CASE[:8]
    assert B * H * w * ((S + 255) // 256 * 256) * 2 >= 2 ** 32
    r = _route(BIG_CASE)
    assert (r["st_mode"], r["nst"], r["nT"], r["last_nh"]) == (0, 64, 257, 1)
    # one sequence fewer and the logits fit the 32-bit extent: the default store mode comes back
    assert score_route(dt, B, H, G, 2 ** 20, D, w)["st_mode"] == 2


def test_knobs_move_the_route_as_documented():
    by = {c[0]: c for c in CASES}
    c = by["wg81_ragged"]
    assert _route(c, {"PKV_FINALIZE_PPT": "8"})["ppt"] == 8 and _route(by["nct2_w32"], {"PKV_FINALIZE_PPT": "4"})["ppt"] == 4
    assert _route(c, {"PKV_FINALIZE_PPT": "5"})["ppt"] == 4                  # anything but 4 / 8 is ignored
    assert _route(c, {"PKV_LOGITS_ST": "0"})["st_mode"] == 0 and _route(c, {"PKV_LOGITS_ST": "1"})["st_mode"] == 1
    assert _route(c, {"PKV_LOGITS_NT": "0"})["nt_load"] == 0 and _route(c)["nt_load"] == 1
    assert _route(c, {"PKV_LOGITS_FEXP": "0"})["fexp"] == 0
    r = _route(c, {"PKV_LOGITS_V2": "0"})
    assert (r["kernel"], r["variant"], r["tile"], r["nst"]) == (2, 4, 256, 0)
    r = _route(by["ks4_w64_halo"], {"PKV_LOGITS_TILE": "128"})
    assert (r["variant"], r["tile"], r["nT"]) == (4, 128, 257)
    assert _route(by["ks2_d64"], {"PKV_LOGITS_TILE": "128"})["tile"] == 128
    assert _route(c, {"PKV_LOGITS_TILE": "64"})["tile"] == 0 and _route(by["ks2_d64"], {"PKV_LOGITS_TILE": "64"})["tile"] == 256
    # PKV_LOGITS_V2_WGS = 1: one workgroup per head group as far as the 64-stage cap allows
    for case in sweep_cases():
        r = _route(case, {"PKV_LOGITS_V2_WGS": "1"})
        sph = -(-case[5] // 128)
        assert r["kernel"] == 1 and r["nst"] == min(sph, 64) and r["nT"] == -(-sph // min(sph, 64)), case[0]


def test_the_sweep_reaches_ragged_and_straddling_workgroups():
    seen = {1: set(), 3: set()}
    for wgs in (1, 3):
        for case in sweep_cases():
            seen[wgs] |= cells(_route(case, {"PKV_LOGITS_V2_WGS": str(wgs)}))
    for wgs in (1, 3):
        assert {"ragged workgroup (nh < nst)", "window straddles a stage", "window straddles a workgroup", "nst>=2"} <= seen[wgs], wgs


def test_cu_count_moves_the_default_split():
    """The default split follows the device's CU count: 4 workgroups per CU for C > 8, the two-round rule at C <= 8."""
    by = {c[0]: c for c in CASES}
    assert _route(by["nct2_w32"], cus=128)["nst"] == 16 and _route(by["nct2_w32"], cus=256)["nst"] == 8
    assert _route(by["wg81_ragged"], cus=512)["nst"] == 1                    # fewer stages than 4 per CU: one stage per workgroup
    assert set(KNOB_CASES) <= set(by)
