"""CPU: the route restatement of tests/merge_routes.py at 256 CUs - each case is on the cells it names, the cases fill the matrix,
the boundaries of launch_merge_t are where the C++ puts them - and the planted rows of the exact cases: oracle.merge_pivots (the
very ops of the reference) must give the pivot each planted row is built for, so that the reference alone is unambiguous before
any kernel is asked."""
import pytest
import torch

from merge_routes import (BY_NAME, CASES, FLAGS, KNOB_CASES, KNOB_MATRIX, MATRIX, cells, class_consts, drop_list, make_inputs, merge_route,
                          plant_plan, route_of, sweep_cases)
from oracle import pkv_oracle as O


def _cells(case, knobs=None, cus=256):
    return cells(route_of(case, knobs, cus), case["dt"], case["k"] + case["w"])


def test_every_case_is_on_its_intended_cells():
    for case in CASES:
        want = {c for c in case["cells"] if not c.startswith("flag: ")}
        assert want <= _cells(case), (case["name"], sorted(want - _cells(case)))


def test_the_cases_fill_the_matrix():
    seen = set().union(*(_cells(c) for c in CASES)) | set().union(*(c["cells"] for c in CASES))
    assert MATRIX <= seen, sorted(MATRIX - seen)
    assert {"flag: " + n for n in FLAGS} <= MATRIX and len(FLAGS) == 16


def test_the_knob_children_fill_their_cells():
    seen = set()
    for knobs in ({"PKV_MERGE_PIVOT2": "0"}, {"PKV_MERGE_PF": "2"}, {"PKV_MERGE_NT": "0"}, {"PKV_MERGE_DROPLIST2": "0"},
                  {"PKV_MERGE_PF": "2", "PKV_MERGE_NT": "0"}, {}):
        for name in KNOB_CASES:
            seen |= _cells(BY_NAME[name], knobs)
    assert KNOB_MATRIX <= seen, sorted(KNOB_MATRIX - seen)


def test_stage_count_at_256_cus():
    r = merge_route("bf16", 1, 32, 1, 32768, 128, 8, 128)
    assert (r["pivot"], r["nst"], r["wg_per_head"], r["last_nh"], r["pf"], r["nt_load"]) == (2, 11, 24, 3, 1, 1)
    # B * H * ceil(S / 128) stages up to the 768 slots of 256 CUs: one stage per workgroup
    assert merge_route("bf16", 1, 8, 1, 12288, 128, 8, 128)["nst"] == 1 and merge_route("bf16", 1, 8, 1, 12289, 128, 8, 128)["nst"] == 2
    r = route_of(BY_NAME["nst2_ragged_fp16"])
    assert (r["nst"], r["wg_per_head"], r["last_nh"]) == (2, 50, 1)
    assert route_of(BY_NAME["nst2_ragged_fp16"], cus=304)["nst"] == 1                  # the split follows the CU count
    r = merge_route("fp16", 1, 2, 1, 40001, 128, 8, 64)                               # test_merge_long_odd_prompt's kind of shape
    assert r["nst"] == min(313, -(-626 // 768)) == 1
    for nst in (2, 3, 5):
        r = route_of(BY_NAME["nt144"], {"PKV_MERGE_NST": str(nst)})
        assert (r["nst"], r["wg_per_head"]) == (nst, -(-706 // (128 * nst)))


def test_boundaries():
    base = dict(dtype="bf16", B=1, H=2, G=1, S=2000, D=128, w=8)
    for nt, tiles_odd, tail in ((16, 1, 0), (17, 0, 1), (32, 0, 0), (33, 1, 1), (143, 1, 1), (144, 1, 0)):
        r = merge_route(k=nt - 8, **base)
        c = cells(r, "bf16", nt)
        assert r["pivot"] == 2 and ("pivot2 tiles: odd" in c) == bool(tiles_odd) and ("pivot2 tail tile: yes" in c) == bool(tail), nt
    assert merge_route(k=137, **base)["pivot"] == 1                                    # 145 kept rows: merge_pivot_kernel<T, 4>
    assert merge_route(k=136, knobs={"PKV_MERGE_PIVOT2": "0"}, **base)["pivot"] == 1
    assert merge_route(k=136, ks_s=2 ** 30, **base)["pivot"] == 1 and merge_route(k=136, ks_s=2 ** 30 - 1, **base)["pivot"] == 2   # restatement only
    assert merge_route(k=136, ks_s=0, **base)["pivot"] == 1
    for D in (64, 256):
        assert merge_route("fp16", 1, 2, 1, 2000, D, 8, 64)["pivot"] == 1 and merge_route("fp32", 1, 2, 1, 2000, D, 8, 64)["pivot"] == 3
    # bucket: fast up to 256 kept rows and 32768 positions; one pass per 8192 kept rows
    f = lambda nt, S: (lambda r: (r["bucket_fast"], r["bucket_ranges"]))(merge_route("bf16", 1, 1, 1, S, 128, 8, nt - 8))   # noqa: E731
    assert f(256, 32768) == (1, 1) and f(257, 32768) == (0, 1) and f(256, 32769) == (0, 1) and f(8192, 20000) == (0, 1) and f(8193, 20000) == (0, 2)
    # drop list slices, scatter bitmap, ntp
    g = lambda S: merge_route("bf16", 1, 1, 1, S, 128, 8, 8)     # noqa: E731
    assert [g(S)["drop_grid"] for S in (4095, 4096, 4097, 8193)] == [1, 1, 2, 3]
    assert g(4097, )["bitmap_bytes"] == 129 * 4 and g(4096)["bitmap_bytes"] == 128 * 4
    assert merge_route("bf16", 1, 1, 1, 900, 128, 8, 1)["ntp"] == 16 and merge_route("bf16", 1, 1, 1, 900, 128, 8, 8)["ntp"] == 16
    r = merge_route("bf16", 1, 1, 1, 900, 128, 8, 8, knobs={"PKV_MERGE_DROPLIST2": "0", "PKV_MERGE_PF": "2", "PKV_MERGE_NT": "0"})
    assert (r["droplist"], r["drop_grid"], r["pf"], r["nt_load"]) == (1, 1, 2, 0)
    assert merge_route("bf16", 1, 1, 1, 900, 128, 8, 8, knobs={"PKV_MERGE_PF": "3"})["pf"] == 1        # anything but 2 is 1
    assert merge_route("bf16", 1, 1, 1, 900, 64, 8, 8)["scatter_block"] == 64 and merge_route("fp32", 1, 1, 1, 900, 64, 8, 8)["scatter_block"] == 128


def test_the_sweep_reaches_one_two_and_three_stage_workgroups():
    """PKV_MERGE_NST = 2 / 3 / 5 over sweep_cases(): workgroups of nh = 1, 2, 3 stages (the preB / idn hand-over under PF = 2), odd and
    even nh, by the number of dropped rows of each case."""
    seen = {}
    for nst in (2, 3, 5):
        nhs = set()
        for case in sweep_cases():
            n = case["S"] - case["k"]                               # at least: the union of several heads only shortens it
            full, rest = divmod(-(-n // 128), nst)
            nhs |= ({nst} if full else set()) | ({rest} if rest else set())
        seen[nst] = nhs
    assert {1, 2} <= seen[2] and {1, 2, 3} <= seen[3] and {1, 2, 3, 4, 5} <= seen[5], seen
    assert len(sweep_cases()) >= 25


EXACT = [c["name"] for c in CASES if c["data"] in ("classes", "groups")]


@pytest.mark.parametrize("name", EXACT)
def test_planted_rows_against_the_oracle(name):
    """The reference's own pivots (oracle.merge_pivots) of every planted row are the planted ones."""
    case = BY_NAME[name]
    K, V, idx, expect = make_inputs(case)
    piv = O.merge_pivots(K, V, idx, case["w"]).reshape(case["B"] * case["H"], -1)
    wrong = [(hr, want, int(piv[hr])) for hr, want in expect.items() if int(piv[hr]) != want]
    assert expect and not wrong, (name, wrong[:10], len(wrong))
    if case["data"] == "classes":
        n = len(drop_list(case, idx))
        classes = {cls for _, cls in plant_plan(case, n)}
        assert {"pz", "sub", "zero"} <= classes and (case["dt"] == "fp32" or "nz" in classes)
        assert {"Z", "N1", "N2", "K"} <= set(case["heads"])


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_the_signed_zero_row_in_the_oracle(dt):
    """The "-0" row of the Z heads: kept row 0 comes first among the zeros, so the reference's pivot is 0 whatever the sign of that
    zero.  fp16: the reference's similarity there IS -0.0 (a dot product of -2^-34).  bf16: a zero similarity needs an fp32 sum
    below 2^-134, a subnormal; ATen's CPU product gives +0.0 for every such input tried here (products -2^-136 .. -2^-148), so the
    bf16 row does not discriminate on the reference's side - it is kept because the kernel's own similarity may still be -0."""
    case = BY_NAME["cls_small_" + dt]
    K, V, idx, expect = make_inputs(case)
    drop = drop_list(case, idx)
    rank = next(r for r, cls in plant_plan(case, len(drop)) if cls == "nz")
    _, _, k_hh, _, piv = O._merge_front(K, V, idx, case["w"])
    x = K[:, :1, drop[rank]][:, :, None]                             # head 0 is a Z head
    sim = (x / torch.norm(x, dim=-1, keepdim=True)) @ (k_hh[:, :1] / torch.norm(k_hh[:, :1], dim=-1, keepdim=True)).transpose(-1, -2)
    s = sim[0, 0, 0]
    assert float(s.max()) == 0.0 and int(piv[0, 0, rank]) == 0
    neg0 = bool(torch.signbit(s[0]))
    print(dt, "similarity at kept row 0:", float(s[0]), "signbit", neg0)
    if dt == "fp16":
        assert neg0 and not bool(torch.signbit(s[1]))
        assert class_consts(dt)[0] * class_consts(dt)[1] == 2.0 ** -34
