"""Which error wins: the status of every validating entry point of include/pkv.h over a deterministic table of descriptors and
scalar arguments, compared cell by cell with tests/golden/abi_status_table.json.

The fixture is the record of the order of the checks in pyramidkv_amd/csrc/pkv_api.hip.  It was written ONCE, by record()
below driving a libpkv.so built from the commit BEFORE the API layer's validation was folded into check_desc flags and
builders, and is never regenerated from later code:

    PKV_LIB=<libpkv.so of that commit> python -c "import sys; sys.path[:0] = ['.', 'tests']; \
        import test_abi_status_table as t; t.write_fixture()"

Every call is in a form that returns before any launch (a defect in the descriptor, a null or misaligned pointer, a short
workspace or a short stride), so no row may answer PKV_OK or PKV_ERR_HIP; record() asserts that.  Host only: with a GPU a row
this build refuses could launch on the fake pointers (as in test_abi_argument_fuzz_never_crashes)."""
import ctypes
import itertools
import json
import os
import random

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_status_table.json")
P16, BAD = 16, 24                 # a fake aligned device pointer, a misaligned one


def _a(x, n):
    return (x + n - 1) // n * n


def _clone(N, d):
    return N.PkvDesc.from_buffer_copy(bytes(d))


def _base(N, dtype, D, g, l2norm):
    """A valid descriptor: [1, 4, 64, D] contiguous, window 8 / topk 4 (L2Norm: window 0, no pooling)."""
    d = N.PkvDesc()
    d.dtype, d.B, d.H, d.S, d.D, d.kv_group = dtype, 1, 4, 64, D, g
    d.q_stride = (ctypes.c_int64 * 3)(4 * 64 * D, 64 * D, D)
    d.k_stride = (ctypes.c_int64 * 3)(4 // g * 64 * D, 64 * D, D)
    d.v_stride = (ctypes.c_int64 * 3)(4 // g * 64 * D, 64 * D, D)
    d.window, d.topk = (0, 4) if l2norm else (8, 4)
    d.pool_kind, d.pool_kernel = (0, 0) if l2norm else (2, 7)
    return d


def _perturbations(d):
    """One-at-a-time changes of a base (a few need a second field to let the check under test decide)."""
    g, w, S = d.kv_group, d.window, d.S
    out = [{"dtype": 3}, {"dtype": -1}, {"D": 96}, {"B": 0}, {"B": 70000}, {"H": 0}, {"H": 33, "kv_group": 4},
           {"S": 1}, {"S": 2}, {"S": 8}, {"kv_group": 0}, {"kv_group": 3}]
    for S2 in (S, 512):           # at S = 64 `window >= S` answers first; S = 512 lets the window limits decide
        out += [{"S": S2, "window": x} for x in (0, 64, 129, 260 // g)]
    out += [{"topk": x} for x in (0, S - w, S - w + 1, S, S + 1)]
    out += [{"S": 8192, "topk": 4097}, {"S": 8192, "topk": 5000}]
    out += [{"pool_kind": -1}, {"pool_kind": 3}]
    out += [{"pool_kind": 1, "pool_kernel": x} for x in (0, 2, 17, 19)]
    out += [{"tie_order": 2}]
    out += [{(arr, i): x} for arr in ("q_stride", "k_stride", "v_stride") for i in range(3) for x in (4, 130, 132)]
    out += [{"struct_size": 132}, {"struct_size": 140}, {"reserved0": 1}]
    return out


def _descriptors(N):
    """-> [(label, descriptor)] in a fixed order."""
    rows = []
    for l2norm in (False, True):
        for dtype, D, g in itertools.product((0, 1, 2), (64, 128, 256), (1, 4)):
            base = _base(N, dtype, D, g, l2norm)
            tag = f"{'l2' if l2norm else 'win'}/dt{dtype}/D{D}/g{g}"
            rows.append((tag, base))
            for p in _perturbations(base):
                d = _clone(N, base)
                for f, x in p.items():
                    if isinstance(f, tuple):
                        getattr(d, f[0])[f[1]] = x
                    else:
                        setattr(d, f, x)
                rows.append((f"{tag} {p}", d))
    rnd = random.Random(1)        # the descriptors of test_abi_argument_fuzz_never_crashes, draw for draw
    for n in range(3000):
        d = N.PkvDesc()
        d.dtype = rnd.choice([0, 1, 2, 3, -1])
        d.B, d.H, d.S = rnd.choice([0, 1, 2, 8, 70000]), rnd.choice([0, 1, 8, 32, 33]), rnd.choice([1, 2, 9, 64, 4096, 32768, 200000])
        d.D, d.kv_group = rnd.choice([32, 64, 96, 128, 256, 512]), rnd.choice([0, 1, 2, 3, 4, 8])
        for arr in (d.q_stride, d.k_stride, d.v_stride):
            for i in range(3):
                arr[i] = rnd.choice([0, 4, 8, 128, 130, 4096, 1 << 33])
        d.window, d.pool_kind, d.pool_kernel = rnd.choice([0, 1, 8, 64, 65, 100000]), rnd.choice([-1, 0, 1, 2, 3]), rnd.choice([0, 1, 2, 7, 17, 19])
        d.reduce, d.scale_mode, d.topk = rnd.choice([0, 1]), rnd.choice([0, 1]), rnd.choice([0, 1, 5, 4096, 5000, 1 << 30])
        rnd.choice([None, 16, 24, 1 << 20]), rnd.choice(range(6))       # the fuzz test's pointer and entry point draws
        rows.append((f"random {n}", d))
    return rows


# name, number of pointers (the workspace last where there is one), which of them are checked for alignment
DESC_CALLS = [
    ("score_window", 4, (0, 1, 2, 3)), ("score_h2o", 4, (0, 1, 3)), ("compress", 6, (0, 1, 2, 3, 4, 5)),
    ("compress_h2o", 6, (0, 1, 2, 3, 4, 5)), ("select", 4, (0, 1, 3)), ("select_h2o", 4, (0, 1, 3)),
    ("compress_l2norm", 5, (0, 1, 2, 3, 4)), ("merge_compact", 6, (0, 1, 3, 4, 5)), ("ada_select", 7, (0, 1, 6)),
    ("gather_compact", 5, (0, 1, 3, 4)), ("gather_streaming", 4, (0, 1, 2, 3)), ("gather_flat", 7, (0, 1, 5, 6)),
]
COLUMNS = []                      # filled by the first _drive()


def _drive(N, d, i):
    """Every descriptor-taking entry point on `d` -> (one status character per call, the three workspace sizes)."""
    L = N.lib
    tot, mtot, ltot = L.pkv_workspace_bytes(d), L.pkv_merge_workspace_bytes(d), L.pkv_l2norm_workspace_bytes(d)
    es = 4 if d.dtype == 2 else 2
    rows = d.B * d.H * d.window
    no_rowstat = tot - _a(d.B * d.H * d.S * 8, 256)                  # ws_layout: everything in front of the H2O row statistics
    score_need = _a(rows * _a(d.S, 256) * es, 256) + _a(rows * _a(d.S, 64 if d.dtype == 2 else 128) // (64 if d.dtype == 2 else 128) * 8, 256)
    Lp, k = max(_a(d.S - d.window, 8), 8), d.topk
    fn = {
        "score_window": lambda p, n, s=Lp: L.pkv_score_window(d, p[0], p[1], p[2], s, p[3], n, None),
        "score_h2o": lambda p, n, s=d.S - d.window: L.pkv_score_h2o(d, p[0], p[1], p[2], s, p[3], n, None),
        "compress": lambda p, n: L.pkv_compress(d, p[0], p[1], p[2], p[3], p[4], None, p[5], n, None),
        "compress_h2o": lambda p, n: L.pkv_compress_h2o(d, p[0], p[1], p[2], p[3], p[4], None, p[5], n, None),
        "select": lambda p, n: L.pkv_select(d, p[0], p[1], 0, p[2], p[3], n, None),
        "select_h2o": lambda p, n: L.pkv_select(d, p[0], p[1], 1, p[2], p[3], n, None),
        "compress_l2norm": lambda p, n, no=None: L.pkv_compress_l2norm(d, p[0], p[1], p[2], p[3], None, no, p[4], n, None),
        "merge_compact": lambda p, n, s=k: L.pkv_merge_compact(d, p[0], p[1], p[2], s, p[3], p[4], p[5], n, None),
        # Ada-SnapKV with base 1: M = topk >= min(L, H) holds on the bases
        "ada_select": lambda p, n, given=None, mirror=None, seq=0: L.pkv_ada_select(d, p[0], p[1], 1, 0.2, 1, given, p[2], p[3], p[4], p[5], None, mirror, seq, p[6], n, None),
        "gather_compact": lambda p, n, s=k: L.pkv_gather_compact(d, p[0], p[1], p[2], s, p[3], p[4], None),
        "gather_streaming": lambda p, n: L.pkv_gather_streaming(d, p[0], p[1], p[2], p[3], None),
        "gather_flat": lambda p, n: L.pkv_gather_flat(d, p[0], p[1], p[2], k, p[3], p[4], p[5], p[6], 0, None),
    }
    need = {"score_window": score_need, "score_h2o": tot, "compress": no_rowstat, "compress_h2o": tot, "select": no_rowstat,
            "select_h2o": tot, "compress_l2norm": ltot, "merge_compact": mtot, "ada_select": no_rowstat}
    out, cols = [], []

    def rec(col, rc):
        cols.append(col)
        out.append(rc)
    for name, nptr, aligned in DESC_CALLS:
        ok = [P16] * nptr
        null = list(ok); null[i % nptr] = None
        mis = list(ok); mis[aligned[i % len(aligned)]] = BAD
        f = fn[name]
        if name in need:
            n = max(need[name], 0)
            rec(name + ":ws0", f(ok, 0)); rec(name + ":need-1", f(ok, max(n - 1, 0)))
        else:
            n = 0
        rec(name + ":null", f(null, n)); rec(name + ":misaligned", f(mis, n))
        if name == "score_window":        # the stride check sits behind the workspace check
            rec(name + ":stride-8", f(ok, n, Lp - 8)); rec(name + ":stride+4", f(ok, n, Lp + 4))
        if name in ("score_h2o", "merge_compact", "gather_compact"):
            rec(name + ":stride-1", f(ok, n, (d.S - d.window if name == "score_h2o" else k) - 1))
        if name == "compress_l2norm":
            rec(name + ":norm_out", f(ok, n, BAD))
        if name == "ada_select":
            nocap = list(ok); nocap[3] = None
            rec(name + ":no_capacity", f(nocap, n)); rec(name + ":mirror+4", f(ok, n, None, 20)); rec(name + ":seq-1", f(ok, n, None, P16, -1))
            rec(name + ":short_mirror:ws0", f(ok, 0, None, P16)); rec(name + ":headkv:ws0", f(nocap, 0, P16)); rec(name + ":headkv:null:ws0", f(null, 0, P16))
    if not COLUMNS:
        COLUMNS.extend(cols)
    assert cols == COLUMNS
    return "".join(_ch(rc, f"{COLUMNS[j]} row {i}") for j, rc in enumerate(out)), (tot, mtot, ltot)


def _ch(rc, what):
    assert rc not in (0, -6) and -9 <= rc < 0, f"{what}: status {rc} - this call reached a launch (or is no status)"
    return str(-rc)


def _ada_need(H, fp32=False):
    return 1024 + (4 * H * 256 * 4 + 4 * H * 4 if fp32 else 2 * H * 256 * 4)


def _scalars(N):
    """The entry points without a descriptor over a grid of their own limits -> {name: status characters}, and the
    pkv_topk_workspace_bytes sizes."""
    L = N.lib
    res = {}

    def run(name, calls):
        res[name] = "".join(_ch(rc, f"{name} call {j}") for j, rc in enumerate(calls))
    # pkv_topk has no check behind its launch-free ones: only calls that some check refuses (valid arguments: a null pointer)
    bad_topk = [(3, 1, 64, 4, 64, 4), (-1, 1, 64, 4, 64, 4), (0, 0, 64, 4, 64, 4), (0, 1, 0, 0, 0, 0), (0, 1, 64, 0, 64, 0),
                (1, 1, 64, 65, 64, 65), (0, 1, 64, 4, 63, 4), (0, 1, 64, 4, 64, 3), (2, 1, 8192, 4097, 8192, 4097),
                (2, 1, 64, 65, 64, 65), (2, 0, 64, 4, 64, 4)]
    long_rows = [(0, 1, 57345, 4), (1, 2, 65536, 64), (0, 1, 65537, 4096), (0, 1, 65537, 4097), (0, 1, 32760, 16385), (1, 1, 200000, 32769)]
    t = [L.pkv_topk(dt, r, n, k, P16, ss, None, P16, iss, None) for dt, r, n, k, ss, iss in bad_topk]
    t += [L.pkv_topk(dt, r, n, k, P16, n, None, P16, k, None) for dt, r, n, k in long_rows]             # no scratch: UNSUPPORTED
    t += [L.pkv_topk(0, 1, 64, 4, None, 64, None, P16, 4, None), L.pkv_topk(2, 1, 64, 4, P16, 64, None, None, 4, None),
          L.pkv_topk(3, 1, 64, 4, None, 64, None, None, 4, None), L.pkv_topk(0, 0, 0, 0, None, 0, None, None, 0, None)]
    run("topk", t)
    t = [L.pkv_topk_ws(dt, r, n, k, P16, ss, None, P16, iss, P16, 1 << 30, None) for dt, r, n, k, ss, iss in bad_topk]
    for dt, r, n, k in long_rows:
        need = L.pkv_topk_workspace_bytes(r, n, k)
        assert need > 0
        t += [L.pkv_topk_ws(dt, r, n, k, P16, n, None, P16, k, P16, need - 1, None), L.pkv_topk_ws(dt, r, n, k, P16, n, None, P16, k, None, need, None),
              L.pkv_topk_ws(dt, r, n, k, P16, n, None, P16, k, BAD, need, None), L.pkv_topk_ws(dt, r, n, k, P16, n, P16, P16, k, P16, need, None),
              L.pkv_topk_ws(dt, r, n, k, None, n, None, P16, k, P16, need, None), L.pkv_topk_ws(dt, r, n, k, P16, n - 1, None, P16, k, P16, need, None)]
    run("topk_ws", t)
    sizes = [L.pkv_topk_workspace_bytes(r, n, k) for r in (0, 1, 8) for n in (0, 1, 57344, 57345, 65536, 65537, 200000)
             for k in (0, 1, 4096, 4097, 16384, 16385, 32768, 32769)]
    t = [L.pkv_sort_rows(dt, r, n, P16, ss, P16, None, None) for dt, r, n, ss in
         [(2, 1, 64, 64), (3, 1, 64, 64), (-1, 1, 64, 64), (0, 0, 64, 64), (0, 1, 0, 0), (1, 1, 64, 63), (0, 1, 32769, 32769), (1, 1, 65537, 65537)]]
    t += [L.pkv_sort_rows(0, 1, 64, None, 64, P16, P16, None), L.pkv_sort_rows(1, 1, 32768, P16, 32768, None, None, None),
          L.pkv_sort_rows(0, 0, 65537, None, 0, None, None, None), L.pkv_sort_rows(2, 0, 65537, None, 0, None, None, None)]
    run("sort_rows", t)
    Hs, Ls = (0, 1, 8, 256, 257), (0, 1, 64, 32768, 32769, 65536, 65537)
    t = []
    for dt, H, n in itertools.product((0, 1, 2, 3), Hs, Ls):
        for base in (0, 1, n, n + 1):
            t.append(L.pkv_ada_budget(dt, H, n, P16, base, 0.2, 1, P16, P16, _ada_need(H) - 1, None))
        t.append(L.pkv_ada_budget(dt, H, n, *[(None, 1, 0.2, 1, P16, P16), (P16, 1, 0.2, 1, None, P16), (P16, 1, 0.2, 1, P16, None)][len(t) % 3], _ada_need(H), None))
    run("ada_budget", t)
    t = []
    for dt, H, n, base in itertools.product((0, 1, 2, 3), Hs, Ls, (0, 1, 300)):
        m = min(n, H * base)                                         # what M must cover
        for M, ss, iss in ((m - 1, n, m), (m, n, m), (n, n, n), (n + 1, n, n + 1), (m, n - 1, m), (m, n, m - 1)):
            t.append(L.pkv_ada_budget_topm(dt, H, n, M, P16, ss, P16, iss, base, 0.2, 1, 8, P16, P16, P16, P16, _ada_need(H) - 1, None))
        ptrs = [[P16] * 6 for _ in range(6)]
        ptrs[0][0] = ptrs[1][1] = ptrs[2][2] = ptrs[3][3] = ptrs[4][4] = ptrs[5][5] = None     # scores, top_idx, head_capacity, head_lens, cu_klen, ws
        p = ptrs[len(t) % 6]
        t.append(L.pkv_ada_budget_topm(dt, H, n, m, p[0], n, p[1], m, base, 0.2, 1, 8, p[2], p[3], p[4], p[5], _ada_need(H), None))
    run("ada_budget_topm", t)
    t = []
    for dt, H, n, base in itertools.product((0, 1, 2, 3), Hs, Ls, (0, 1, 300)):
        need = _ada_need(H, dt == 2)
        for ss, mirror, seq, nb in ((n, None, 0, need - 1), (n - 1, None, 0, need - 1), (n, 20, 0, need - 1), (n, P16, -1, need - 1), (n, None, -1, need - 1),
                                    (n, P16, 0, _ada_need(H) - 1)):
            t.append(L.pkv_ada_budget_rows(dt, H, n, P16, ss, base, 0.2, 1, 8, P16, P16, P16, None, mirror, seq, P16, nb, None))
        p = [[None, P16, P16, P16, P16], [P16, None, P16, P16, P16], [P16, P16, None, P16, P16], [P16, P16, P16, None, P16], [P16, P16, P16, P16, None]][len(t) % 5]
        t.append(L.pkv_ada_budget_rows(dt, H, n, p[0], n, base, 0.2, 1, 8, p[1], p[2], p[3], None, 20, 0, p[4], need, None))
    run("ada_budget_rows", t)
    t = []
    for dt, H, n in itertools.product((0, 1, 2, 3), Hs, Ls):
        for M, base, ss, iss in ((0, 1, n, 0), (1, 1, n, 1), (n, 1, n, n), (n + 1, 1, n, n + 1), (n, 0, n, n), (n, n, n, n), (n, n + 1, n, n),
                                 (n, 1, n - 1, n), (n, 1, n, n - 1)):
            t.append(L.pkv_ada_adaptive_lists(dt, H, n, M, P16, ss, P16, iss, base, 1, P16, P16, _ada_need(H) - 1, None))
        p = [[None, P16, P16, P16], [P16, None, P16, P16], [P16, P16, None, P16], [P16, P16, P16, None]][len(t) % 4]
        t.append(L.pkv_ada_adaptive_lists(dt, H, n, n, p[0], n, p[1], n, 1, 1, p[2], p[3], _ada_need(H), None))
    run("ada_adaptive_lists", t)
    run("ada_metadata", [L.pkv_ada_metadata(0, 8, P16, P16, P16, None), L.pkv_ada_metadata(-1, 8, P16, P16, P16, None), L.pkv_ada_metadata(4, 8, None, P16, P16, None),
                         L.pkv_ada_metadata(4, 8, P16, None, P16, None), L.pkv_ada_metadata(4, 8, P16, P16, None, None), L.pkv_ada_metadata(0, 8, None, P16, P16, None)])
    t = [L.pkv_update_flatten_view(dt, H, hd, P16, P16, P16, P16, P16, None) for dt, H, hd in
         [(3, 4, 128), (-1, 4, 128), (0, 0, 128), (1, 4, 0), (2, 4, 4), (0, 4, 12), (2, 257, 130)]]
    for j in range(5):
        p = [P16] * 5; p[j] = None
        t.append(L.pkv_update_flatten_view(j % 3, 4, 128, *p, None))
    for j in (0, 1, 4):
        p = [P16] * 5; p[j] = BAD
        t.append(L.pkv_update_flatten_view(j % 3, 4, 128, *p, None))
    t += [L.pkv_update_flatten_view(0, 4, 12, BAD, P16, P16, P16, P16, None), L.pkv_update_flatten_view(0, 0, 128, None, P16, P16, P16, P16, None)]
    run("update_flatten_view", t)
    return res, sizes


def record(N):
    """The whole table, in the fixture's form: rows point into a list of distinct status strings / size triples."""
    patterns, sizes, rows, size_rows, labels = {}, {}, [], [], []
    for i, (label, d) in enumerate(_descriptors(N)):
        st, sz = _drive(N, d, i)
        rows.append(patterns.setdefault(st, len(patterns)))
        size_rows.append(sizes.setdefault(sz, len(sizes)))
        labels.append(label)
    scalars, topk_sizes = _scalars(N)
    table = {"columns": list(COLUMNS), "patterns": list(patterns), "rows": rows, "sizes": [list(s) for s in sizes], "size_rows": size_rows,
             "scalars": scalars, "topk_workspace_bytes": topk_sizes}
    return table, labels


def write_fixture():
    from pyramidkv_amd import _native as N
    assert not torch.cuda.is_available()
    table, _ = record(N)
    table = dict(generator="tests/test_abi_status_table.py write_fixture(), from the library of the commit before the check_desc flags", **table)
    with open(FIXTURE, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")


def test_every_status_equals_the_recorded_one():
    """Every cell - status or size - equals what the library answered before the API layer's validation was rewritten."""
    if torch.cuda.is_available():
        pytest.skip("rows this build refuses could launch on the fake pointers with a device present: a host-only test")
    if not os.path.exists(os.path.join(ROOT, "pyramidkv_amd", "libpkv.so")):
        import __graft_entry__ as g
        g.build()
    from pyramidkv_amd import _native as N
    want = json.load(open(FIXTURE))
    got, labels = record(N)
    assert got["columns"] == want["columns"]
    assert len(got["rows"]) == len(want["rows"]) == len(labels) and len(labels) > 5000
    for i, label in enumerate(labels):
        g, w = got["patterns"][got["rows"][i]], want["patterns"][want["rows"][i]]
        if g != w:
            diff = [(want["columns"][j], f"recorded -{w[j]}", f"now -{g[j]}") for j in range(len(w)) if g[j] != w[j]]
            pytest.fail(f"row {i} ({label}): {diff}")
        assert got["sizes"][got["size_rows"][i]] == want["sizes"][want["size_rows"][i]], (i, label, "workspace / merge / l2norm bytes")
    assert got["scalars"].keys() == want["scalars"].keys()
    for name, w in want["scalars"].items():
        g = got["scalars"][name]
        assert len(g) == len(w), name
        assert g == w, (name, [(j, f"recorded -{w[j]}", f"now -{g[j]}") for j in range(len(w)) if g[j] != w[j]][:10])
    assert got["topk_workspace_bytes"] == want["topk_workspace_bytes"]
