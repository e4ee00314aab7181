"""The route matrix of the LOOK-M pivot merge (tests/test_gpu_merge_routes.py, tests/test_merge_routes_plan.py).

``merge_route`` restates, in plain Python, the choices launch_merge, launch_merge_t and launch_merge_f32_t
(pyramidkv_amd/csrc/pkv_merge.hip) and merge_ws (pkv_api.hip) make for a shape, the knobs and the device's CU count.  Its keys are
the first 15 words of the debug library's route record (pkv_debug_merge_route, include/pkv.h), in that order; word 15 holds the
device flags (FLAGS: one bit per data-dependent path a merge kernel took).

One cell of the matrix cannot be reached by the host at a sane size and stays restatement-only: a K row stride of 2^30 elements
or more (tens of GB of keys) sends D = 128 / nt <= 144 to merge_pivot_kernel (test_merge_routes_plan.py pins the restatement).

Run as a child process, ``python tests/merge_routes.py MODE`` prints one JSON object: per case the recorded route (None on the
release library), a digest of K_m, V_m, the drop list and the pivots read from the workspace, whether the case passes its checks,
the number of moved pivots and the seconds spent in the CPU oracle.  MODE: ``matrix`` (CASES), ``sweep`` (sweep_cases(), for the
PKV_MERGE_NST / PKV_MERGE_PF runs) or ``knobs-digest`` (KNOB_CASES, digests only)."""
import json
import os
import sys
import time
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

WORDS = ["droplist", "drop_grid", "pivot", "ks", "nt_load", "pf", "nst", "pivot_grid", "wg_per_head", "last_nh", "bucket_fast",
         "bucket_ranges", "scatter_block", "bitmap_bytes", "ntp", "flags"]
KNOBS = ["PKV_MERGE_PIVOT2", "PKV_MERGE_NST", "PKV_MERGE_PF", "PKV_MERGE_NT", "PKV_MERGE_DROPLIST2"]
FLAGS = ["pivot2 signed-key loop", "pivot2 redo", "pivot2 exact by NaN", "bf16 multiply form", "bf16 div_const form", "prefetch issued",
         "ragged workgroup (nh < nst)", "workgroup past the drop list", "merge_pivot_kernel exact", "bucket fast", "bucket ranges > 1",
         "scatter group of 0 rows", "scatter group > 2048 rows", "scatter tail 1..31", "scatter tail 33..63", "zero maximum second look"]
MD_SLICE, MP2_TN, MP2_HT, MB_RANGE = 4096, 144, 128, 8192
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def _cdiv(a, b):
    return -(-a // b)


def merge_route(dtype, B, H, G, S, D, w, k, ks_s=None, knobs=None, cus=256):
    """-> {word: int} for a pkv_merge_compact call (H query heads, un-expanded K/V: G = kv_group; ks_s = K's row stride in elements)."""
    env = {n: int(v) for n, v in (knobs or {}).items() if str(v) != ""}        # merge_env: unset or empty = the default
    r = dict.fromkeys(WORDS[:-1], 0)
    nt = k + w
    ks_s = D if ks_s is None else ks_s
    # launch_merge
    dl2 = env.get("PKV_MERGE_DROPLIST2", 1) != 0
    r["droplist"], r["drop_grid"] = (2, _cdiv(S, MD_SLICE)) if dl2 else (1, 1)
    r["ntp"] = _cdiv(nt, 8) * 8                                                 # merge_ws
    r["bitmap_bytes"] = _cdiv(S, 32) * 4
    fast = nt * 32 <= MB_RANGE and S <= 32768
    r["bucket_fast"], r["bucket_ranges"] = int(fast), 1 if fast else _cdiv(nt, MB_RANGE)
    if dtype == "fp32":                                                         # launch_merge_f32_t
        r["pivot"], r["ks"], r["scatter_block"] = 3, D // 16, 2 * D
        gx = _cdiv(S, 64)
    else:                                                                       # launch_merge_t
        KS = D // 32
        r["ks"], r["scatter_block"] = KS, KS * 32
        if KS == 4 and nt <= MP2_TN and env.get("PKV_MERGE_PIVOT2", 1) != 0 and 0 < ks_s < 2 ** 30:
            sph = _cdiv(S, MP2_HT)
            stages, slots = B * H * sph, 3 * cus
            nst = env.get("PKV_MERGE_NST", 0)
            if nst <= 0:
                rounds = max(1, (stages + slots * 6) // (slots * 12))
                nst = max(1, min(sph, _cdiv(stages, slots * rounds)))
            gx = _cdiv(S, nst * MP2_HT)
            r["pivot"], r["nst"] = 2, nst
            r["nt_load"] = int(env.get("PKV_MERGE_NT", 1) != 0)
            r["pf"] = 2 if env.get("PKV_MERGE_PF", 1) == 2 else 1
            r["last_nh"] = min(nst, _cdiv(S - (gx - 1) * nst * MP2_HT, MP2_HT))
        else:
            r["pivot"] = 1
            gx = _cdiv(S, 64 * (2 if KS == 8 else 4))
    r["pivot_grid"], r["wg_per_head"] = gx * B * H, gx
    return r


def decode(words):
    return dict(zip(WORDS, words))


def cells(r, dtype, nt):
    """The cells of the route matrix a route (with or without the flags word) fills."""
    out = {"droplist2" if r["droplist"] == 2 else "droplist (one workgroup)"}
    if r["droplist"] == 2:
        out.add("droplist2: %s" % ("one slice" if r["drop_grid"] == 1 else "several slices"))
    if r["pivot"] == 2:
        out.add("pivot2<%s, NT%d, PF%d>" % (dtype, r["nt_load"], r["pf"]))
        out.add("nst=1" if r["nst"] == 1 else "nst>=2")
        if r["last_nh"] < r["nst"]:
            out.add("ragged grid (last_nh < nst)")
        out.add("pivot2 tiles: %s" % ("odd" if _cdiv(nt, 16) % 2 else "even"))
        out.add("pivot2 tail tile: %s" % ("yes" if nt % 16 else "no"))
    elif r["pivot"] == 1:
        out.add("pivot<%s, KS%d>: %s" % (dtype, r["ks"], "one tile" if nt <= (80 if r["ks"] == 8 else 144) else "several tiles"))
    else:
        out.add("pivot_f32<KSF%d>" % r["ks"])
    out.add("bucket fast" if r["bucket_fast"] else ("bucket ranged: one range" if r["bucket_ranges"] == 1 else "bucket ranged: several ranges"))
    for i, name in enumerate(FLAGS):
        if r.get("flags", 0) >> i & 1:
            out.add("flag: " + name)
    return out


def _flag(*names):
    return {"flag: " + n for n in names}


def C(name, dt, B, H, G, S, D, w, k, data="lattice", idx="rand", layout="bhsd", big=False, cells=(), **kw):
    return dict(name=name, dt=dt, B=B, H=H, G=G, S=S, D=D, w=w, k=k, data=data, idx=idx, layout=layout, big=big, cells=set(cells), **kw)


# planted scatter groups (data="groups"): rows that merge into kept row j, the window rows (j < w = 4) counting themselves
GROUP_SIZES = [1, 31, 32, 33, 0, 63, 64, 65, 2048, 2049, 4100, 0, 5, 95, 97, 130]
_GROUPS_S = 12 + sum(GROUP_SIZES)
_SC = _flag("scatter group of 0 rows", "scatter group > 2048 rows", "scatter tail 1..31", "scatter tail 33..63")
_CLS_HEADS = ["Z", "N1", "N2", "K", "Z", "N1", "N2", "Z"]
_P2 = _flag("pivot2 signed-key loop", "pivot2 redo", "pivot2 exact by NaN")
_P1 = _flag("merge_pivot_kernel exact", "zero maximum second look")

# Each case names the cells it is built for at 256 CUs.  data: "groups" / "classes" are built from exact rows (bit-identical,
# pivots included); "lattice" and "gauss" are held to merge_bar.check_merge (16-bit) / test_gpu_f32.py's bar (fp32).
CASES = [
    # D = 128 at the default knobs
    C("nst1_bf16", "bf16", 2, 4, 1, 1500, 128, 8, 40, cells={"pivot2<bf16, NT1, PF1>", "nst=1", "pivot2 tiles: odd", "pivot2 tail tile: no",
                                                             "bucket fast", "droplist2: one slice"} | _flag("bf16 multiply form")),
    C("nst2_ragged_fp16", "fp16", 1, 8, 1, 12600, 128, 8, 128,
      cells={"pivot2<fp16, NT1, PF1>", "nst>=2", "ragged grid (last_nh < nst)", "droplist2: several slices"} |
      _flag("prefetch issued", "ragged workgroup (nh < nst)", "workgroup past the drop list", "pivot2 signed-key loop")),
    C("gauss_bf16", "bf16", 1, 8, 1, 12700, 128, 8, 128, data="gauss", cells={"pivot2<bf16, NT1, PF1>", "nst>=2"} | _flag("prefetch issued")),
    C("gauss_fp16", "fp16", 2, 4, 2, 3001, 128, 16, 100, data="gauss", cells={"pivot2<fp16, NT1, PF1>", "nst=1"}),
    # the production shape: 32 heads of 32768 keys, budget 128 + window 8 (nst = 11 at 256 CUs).  The CPU oracle takes ~3 s on 8
    # cores for merge_kv and ~1 s more for merge_pivots when a pivot moved (building the Gaussian inputs takes 6 s).
    C("prod_bf16", "bf16", 1, 32, 1, 32768, 128, 8, 128, data="gauss", big=True, cells={"pivot2<bf16, NT1, PF1>", "nst>=2", "bucket fast"}),
    # tile parity and tail of merge_pivot2_kernel, hand-over to merge_pivot_kernel at 145 kept rows
    C("nt9", "fp16", 1, 2, 1, 700, 128, 8, 1, cells={"pivot2 tiles: odd", "pivot2 tail tile: yes"}),
    C("nt16", "bf16", 1, 2, 1, 701, 128, 8, 8, cells={"pivot2 tiles: odd", "pivot2 tail tile: no"}),
    C("nt17", "fp16", 1, 2, 1, 702, 128, 1, 16, cells={"pivot2 tiles: even", "pivot2 tail tile: yes"}),
    C("nt32", "bf16", 1, 2, 1, 703, 128, 16, 16, cells={"pivot2 tiles: even", "pivot2 tail tile: no"}),
    C("nt33", "fp16", 1, 2, 1, 704, 128, 32, 1, cells={"pivot2 tiles: odd", "pivot2 tail tile: yes"}),
    C("nt143", "bf16", 1, 2, 1, 705, 128, 8, 135, cells={"pivot2 tiles: odd", "pivot2 tail tile: yes"}),
    C("nt144", "fp16", 1, 2, 1, 706, 128, 8, 136, cells={"pivot2<fp16, NT1, PF1>", "pivot2 tiles: odd", "pivot2 tail tile: no"}),
    C("nt145_bf16", "bf16", 1, 2, 1, 707, 128, 8, 137, cells={"pivot<bf16, KS4>: several tiles"}),
    C("nt145_fp16", "fp16", 1, 2, 1, 708, 128, 9, 136, cells={"pivot<fp16, KS4>: several tiles"}),
    # head sizes 64 / 256 below and above one LDS tile of merge_pivot_kernel (144 / 80 kept rows)
    C("d64_nt144", "bf16", 1, 4, 2, 1300, 64, 8, 136, cells={"pivot<bf16, KS2>: one tile"}),
    C("d64_nt145", "bf16", 1, 4, 1, 1304, 64, 8, 137, cells={"pivot<bf16, KS2>: several tiles"}),
    C("d64_nt208", "fp16", 1, 4, 1, 1301, 64, 8, 200, cells={"pivot<fp16, KS2>: several tiles"}),
    C("d256_nt80", "fp16", 1, 4, 1, 1302, 256, 8, 72, cells={"pivot<fp16, KS8>: one tile"}),
    C("d256_nt81", "fp16", 1, 4, 1, 1305, 256, 8, 73, cells={"pivot<fp16, KS8>: several tiles"}),
    C("d256_nt100", "bf16", 1, 4, 4, 1303, 256, 4, 96, cells={"pivot<bf16, KS8>: several tiles"}),
    # un-expanded GQA through a [B, S, Hk, D] view on the pivot2 route: the K row stride is Hk * D
    C("gqa_view_bf16", "bf16", 2, 8, 4, 2100, 128, 8, 60, layout="bshd", cells={"pivot2<bf16, NT1, PF1>"}),
    C("gqa_view_fp16", "fp16", 1, 6, 2, 2101, 128, 8, 60, layout="bshd", cells={"pivot2<fp16, NT1, PF1>"}),
    # bucket: fast path up to 256 kept rows and 32768 positions, one pass per 8192 kept rows beyond
    C("bucket_nt256", "bf16", 1, 1, 1, 32768, 128, 8, 248, cells={"bucket fast", "pivot<bf16, KS4>: several tiles"} | _flag("bucket fast")),
    C("bucket_nt257", "fp16", 1, 2, 1, 3000, 128, 8, 249, cells={"bucket ranged: one range"}),
    C("bucket_s32769", "bf16", 1, 1, 1, 32769, 128, 8, 56, cells={"bucket ranged: one range", "pivot2<bf16, NT1, PF1>"}),
    C("bucket_2ranges", "fp16", 1, 1, 1, 9000, 64, 8, 8192, cells={"bucket ranged: several ranges"} | _flag("bucket ranges > 1")),
    # scatter: planted groups of exactly GROUP_SIZES rows (bf16 counts round above 256, fp16 above 2048)
    C("groups_bf16", "bf16", 1, 2, 1, _GROUPS_S, 128, 4, 12, data="groups", idx="shared", cells=_SC),
    C("groups_fp16", "fp16", 1, 2, 1, _GROUPS_S, 128, 4, 12, data="groups", idx="shared", cells=_SC),
    C("groups_d64_fp16", "fp16", 1, 1, 1, _GROUPS_S, 64, 4, 12, data="groups", idx="shared", cells=_SC),
    # drop list: S around the 16-byte words and the 4096-position slices; one dropped row besides the window; the union over
    # batch and heads with overlapping and disjoint selections
    C("S_one_dropped", "bf16", 1, 2, 1, 11, 128, 4, 6, idx="shared"),
    C("S15", "fp16", 1, 2, 1, 15, 128, 4, 6),
    C("S16", "bf16", 1, 2, 1, 16, 128, 4, 6),
    C("S17", "fp16", 1, 2, 1, 17, 128, 4, 6),
    C("S4095", "bf16", 1, 2, 1, 4095, 128, 8, 24, cells={"droplist2: one slice"}),
    C("S4096", "fp16", 1, 2, 1, 4096, 128, 8, 24, cells={"droplist2: one slice"}),
    C("S4097", "bf16", 1, 2, 1, 4097, 128, 8, 24, cells={"droplist2: several slices"}),
    C("S8193", "fp16", 1, 2, 1, 8193, 128, 8, 24, cells={"droplist2: several slices"}),
    C("overlap", "bf16", 2, 6, 1, 2000, 128, 8, 64, idx="overlap"),
    # input classes of the pivot arithmetic (make_classes): exact kept rows, lattice rows and planted rows
    C("cls_bf16", "bf16", 1, 8, 1, 12700, 128, 8, 128, data="classes", idx="shared", heads=_CLS_HEADS,
      cells={"nst>=2"} | _P2 | _flag("bf16 multiply form", "bf16 div_const form", "prefetch issued", "ragged workgroup (nh < nst)")),
    C("cls_fp16", "fp16", 1, 8, 1, 12700, 128, 8, 128, data="classes", idx="shared", heads=_CLS_HEADS,
      cells={"nst>=2"} | _P2 | _flag("prefetch issued", "ragged workgroup (nh < nst)")),
    C("cls_small_bf16", "bf16", 1, 4, 1, 1000, 128, 8, 64, data="classes", idx="shared", heads=_CLS_HEADS[:4], cells={"nst=1"} | _P2),
    C("cls_small_fp16", "fp16", 1, 4, 1, 1000, 128, 8, 64, data="classes", idx="shared", heads=_CLS_HEADS[:4], cells={"nst=1"} | _P2),
    C("cls_nt145_fp16", "fp16", 1, 4, 1, 1000, 128, 8, 137, data="classes", idx="shared", heads=_CLS_HEADS[:4],
      cells={"pivot<fp16, KS4>: several tiles"} | _P1),
    C("cls_nt145_bf16", "bf16", 1, 4, 1, 1000, 128, 8, 137, data="classes", idx="shared", heads=_CLS_HEADS[:4],
      cells={"pivot<bf16, KS4>: several tiles"} | _P1),
    C("cls_d64_fp16", "fp16", 1, 4, 1, 900, 64, 8, 40, data="classes", idx="shared", heads=_CLS_HEADS[:4],
      cells={"pivot<fp16, KS2>: one tile"} | _P1),
    C("cls_d64_bf16", "bf16", 1, 4, 1, 900, 64, 8, 40, data="classes", idx="shared", heads=_CLS_HEADS[:4], cells={"pivot<bf16, KS2>: one tile"} | _P1),
    C("cls_d256_bf16", "bf16", 1, 4, 1, 900, 256, 8, 40, data="classes", idx="shared", heads=_CLS_HEADS[:4], cells={"pivot<bf16, KS8>: one tile"} | _P1),
    C("cls_d256_fp16", "fp16", 1, 4, 1, 900, 256, 8, 40, data="classes", idx="shared", heads=_CLS_HEADS[:4], cells={"pivot<fp16, KS8>: one tile"} | _P1),
    # fp32: one case per head size (test_gpu_f32.py's bar); the classes that exist in fp32 on all-exact rows
    C("f32_d64", "fp32", 1, 4, 2, 1000, 64, 8, 64, data="gauss", cells={"pivot_f32<KSF4>"}),
    C("f32_d128_cls", "fp32", 1, 4, 1, 1000, 128, 8, 64, data="classes", idx="shared", heads=_CLS_HEADS[:4], cells={"pivot_f32<KSF8>"}),
    C("f32_d256", "fp32", 1, 2, 1, 1100, 256, 8, 64, data="gauss", cells={"pivot_f32<KSF16>"}),
]
BY_NAME = {c["name"]: c for c in CASES}

# every cell the default knobs reach; PF2 / NT0 / the one-workgroup drop list are reached by the knob children
MATRIX = (
    {"droplist2", "droplist2: one slice", "droplist2: several slices", "nst=1", "nst>=2", "ragged grid (last_nh < nst)",
     "pivot2 tiles: odd", "pivot2 tiles: even", "pivot2 tail tile: yes", "pivot2 tail tile: no",
     "bucket fast", "bucket ranged: one range", "bucket ranged: several ranges"}
    | {"pivot2<%s, NT1, PF1>" % dt for dt in ("bf16", "fp16")}
    | {"pivot<%s, KS%d>: %s" % (dt, ks, t) for dt in ("bf16", "fp16") for ks in (2, 4, 8) for t in ("one tile", "several tiles")}
    - {"pivot<bf16, KS4>: one tile", "pivot<fp16, KS4>: one tile"}              # PKV_MERGE_PIVOT2=0 only (KNOB_MATRIX)
    | {"pivot_f32<KSF%d>" % k for k in (4, 8, 16)}
    | {"flag: " + n for n in FLAGS}
)
KNOB_MATRIX = {"pivot<bf16, KS4>: one tile", "pivot<fp16, KS4>: one tile", "droplist (one workgroup)"} | \
    {"pivot2<%s, NT%d, PF%d>" % (dt, nt, pf) for dt in ("bf16", "fp16") for nt in (0, 1) for pf in (1, 2)}

KNOB_CASES = ["nst1_bf16", "nst2_ragged_fp16", "gauss_bf16", "gauss_fp16", "nt17", "nt144", "gqa_view_bf16", "groups_fp16", "S4097",
              "S17", "cls_bf16", "cls_fp16", "cls_small_bf16", "d64_nt144"]


def sweep_cases():
    """The D = 128 cases on the pivot2 route that are small enough for six children (PKV_MERGE_NST = 2 / 3 / 5 x PKV_MERGE_PF = 1 / 2)."""
    return [c for c in CASES if c["dt"] != "fp32" and c["D"] == 128 and c["k"] + c["w"] <= MP2_TN and c["S"] <= 13000]


def route_of(case, knobs=None, cus=256):
    Hk = case["H"] // case["G"]
    ks_s = Hk * case["D"] if case["layout"] == "bshd" else case["D"]
    return merge_route(case["dt"], case["B"], case["H"], case["G"], case["S"], case["D"], case["w"], case["k"], ks_s=ks_s, knobs=knobs, cus=cus)


# ---------------------------------------------------------------------------------------------------------------- inputs
def _gen(case, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(case["name"].encode()) + salt)


def make_idx(case):
    """int64 [B, H, k] selected past positions (top-k order: unsorted)."""
    B, H, S, w, k = case["B"], case["H"], case["S"], case["w"], case["k"]
    g = _gen(case, 1)
    L = S - w
    if case["idx"] == "shared":
        one = torch.randperm(L, generator=g)[:k]
        return one[None, None].repeat(B, H, 1)
    if case["idx"] == "overlap":            # heads 0, 3, ..: one set; 1, 4, ..: half of it and new positions; 2, 5, ..: disjoint from both
        perm = torch.randperm(L, generator=g)
        a, b2, c = perm[:k], torch.cat([perm[:k // 2], perm[k:k + k - k // 2]]), perm[2 * k:3 * k]
        rows = [[(a, b2, c)[(h + b) % 3][torch.randperm(k, generator=g)] for h in range(H)] for b in range(B)]
        return torch.stack([torch.stack(r) for r in rows])
    return torch.stack([torch.stack([torch.randperm(L, generator=g)[:k] for _ in range(H)]) for _ in range(B)])


def drop_list(case, idx):
    union = set(idx.flatten().tolist())
    return [p for p in range(case["S"]) if p not in union]


def _exact_row(g, D, count, lo=8, with0=False):
    """One magnitude 2^a, `count` non-zeros with random signs on random coordinates >= lo (with0: coordinate 0 too, positive)."""
    v = torch.zeros(D)
    need = count - 1 if with0 else count
    pool = torch.arange(1 if with0 else 0, D) if need > D - lo else torch.arange(lo, D)
    co = pool[torch.randperm(len(pool), generator=g)[:need]]
    a = float(2.0 ** int(torch.randint(-2, 3, (1,), generator=g)))
    v[co] = (torch.randint(0, 2, (need,), generator=g).float() * 2 - 1) * a
    if with0:
        v[0] = a
    return v


def class_consts(dt):
    """(tiny, xz, sub_t, sub_x): kept row 0 holds -tiny e0, the "-0" row xz e0 (their product rounds to -0 in the model dtype);
    kept row 6 holds sub_t e4 and the "subnormal" row sub_x e4: their product is the smallest positive subnormal of fp16 (2^-24);
    for bf16 and fp32 the smallest positive NORMAL (2^-126), because every bf16 subnormal is an fp32 subnormal and ATen's
    CPU product of bf16 matrices flushes those to zero (measured: a product of 2^-133 comes back as 0)."""
    return {"fp16": (2.0 ** -24, 2.0 ** -10, 2.0 ** -12, 2.0 ** -12), "bf16": (2.0 ** -70, 2.0 ** -66, 2.0 ** -63, 2.0 ** -63),
            "fp32": (0.0, 0.0, 2.0 ** -63, 2.0 ** -63)}[dt]


def plant_plan(case, n):
    """[(rank in the drop list, class)]: single planted rows among ordinary ones in the first stage, a wave of 32 planted rows, a
    planted row sharing its wave with a zero-norm row, rows in the second (prefetched at nst >= 2) stage, in the last stage and in
    the last partially filled 16-row group before the window rows; bf16 / fp32: a non-zero row whose norm underflows to zero."""
    w = case["w"]
    cyc = ["pz", "nz", "sub"] if case["dt"] != "fp32" else ["pz", "sub", "pz"]
    plan = [(3, cyc[0]), (70, cyc[1]), (75, "zero"), (130, cyc[2]), (200, cyc[0]), (n - w - 30, cyc[1]), (n - w - 2, cyc[2]), (n - w - 1, cyc[0])]
    plan += [(32 + i, cyc[i % 3]) for i in range(32)]
    if case["dt"] != "fp16":
        plan.append((140, "under"))
    assert n - w - 30 > 210
    return plan


def make_classes(case):
    """-> (K, V [1, H, S, D] model dtype, idx, expect {(head, rank): pivot}).  Head kinds (case["heads"]):
      Z   kept row 0 = -tiny e0 + e1, kept row 1 = four halves incl. e1, kept row 6 = sub_t e4 + e6, every other kept row an exact
          row on coordinates >= 8.  Planted: "pz" -2^b e1 (similarities -1, -1/2, then +0: maximum +0 -> kept row 2), "nz"
          xz e0 + e2 (-0 at kept row 0, +0 elsewhere: zero is the maximum, the first zero wins -> 0), "sub" sub_x e4 + e5 (the
          smallest subnormal at kept row 6, +0 elsewhere -> 6; must not take the redo path).
      K   a Z head whose kept row zc is zero: its unit form is NaN, every dropped row chooses zc (kept_bad)
      N1  every kept row holds +e0 among 4 or 16 non-zeros, kept row j1 among 64: the planted row -2^b e0 has only negative
          similarities (-1/2, -1/4, -1/8) with a unique maximum at j1
      N2  the same with three 64-non-zero rows: the maximum is tied, the first wins
    Ordinary dropped rows are lattice rows (fp32: exact rows): against exact kept rows every similarity is order-independent.
    A "zero" row is zero in every head (all similarities NaN -> kept row 0); "under" is 2^-80 e9 (norm^2 underflows)."""
    B, H, S, D, w, k, dt = case["B"], case["H"], case["S"], case["D"], case["w"], case["k"], case["dt"]
    assert B == 1 and case["G"] == 1 and k + w >= 12 and w >= 2
    g = _gen(case)
    idx = make_idx(case)
    drop = drop_list(case, idx)
    n, nt = len(drop), k + w
    tiny, xz, sub_t, sub_x = class_consts(dt)
    if dt == "fp32":
        K = torch.zeros(1, H, S, D)
        for h in range(H):
            for s in range(S):
                K[0, h, s] = _exact_row(g, D, (1, 4, 16)[s % 3], lo=0)
    else:
        K = torch.randint(-4, 5, (1, H, S, D), generator=g).float() / 4
        K[:, :, ::3] *= 0.5
    V = torch.randint(-4, 5, (1, H, S, D), generator=g).float() / 4
    kept_pos = [S - w + j for j in range(w)] + idx[0, 0].tolist()
    counts = (1, 4, 16) if D == 64 else (1, 4, 16, 64)
    zc = next(j for j in (w + 1, w + 2, w + 3) if j not in (0, 1, 6))
    j1 = min(w + 3, nt - 1)
    first64 = sorted({5, w + 2, min(w + 7, nt - 1)})
    plan = plant_plan(case, n)
    expect = {}
    e = lambda c, val=1.0: torch.zeros(D).index_fill_(0, torch.tensor([c]), val)      # noqa: E731
    for h in range(H):
        kind = case["heads"][h]
        for j, pos in enumerate(kept_pos):
            if kind in ("Z", "K"):
                row = _exact_row(g, D, counts[int(torch.randint(0, len(counts), (1,), generator=g))])
                if j == 0:
                    row = e(1) - tiny * e(0)
                elif j == 1:
                    row = 0.5 * (e(1) + e(8) + e(9) + e(10))
                elif j == 6:
                    row = sub_t * e(4) + e(6)
                if kind == "K" and j == zc:
                    row = torch.zeros(D)
            else:
                c64 = (j == j1) if kind == "N1" else (j in first64)
                row = _exact_row(g, D, 64 if c64 else (4, 16)[int(torch.randint(0, 2, (1,), generator=g))], with0=True)
            K[0, h, pos] = row
        for rank, cls in plan:
            b = float(2.0 ** int(torch.randint(-3, 4, (1,), generator=g)))
            if cls == "zero":
                row, want = torch.zeros(D), 0
            elif cls == "under":
                row, want = 2.0 ** -80 * e(9), 0
            elif kind in ("N1", "N2"):
                row, want = -b * e(0), (j1 if kind == "N1" else first64[0])
            else:
                row = {"pz": -b * e(1), "nz": xz * e(0) + e(2), "sub": sub_x * e(4) + e(5)}[cls]
                want = zc if kind == "K" else {"pz": 2, "nz": 0, "sub": 6}[cls]
            K[0, h, drop[rank]] = row
            expect[(h, rank)] = want
    return K.to(DT[dt]), V.to(DT[dt]), idx, expect


def make_groups(case):
    """Kept row j is 2^a e_j; sizes[j] dropped rows 2^b e_j (similarity 1 with kept row j, +0 with every other) are spread over the
    dropped positions in a per-head order; the window rows merge onto themselves.  -> (K, V, idx, expect)."""
    B, H, S, D, w, k, dt = case["B"], case["H"], case["S"], case["D"], case["w"], case["k"], case["dt"]
    sizes = case.get("sizes", GROUP_SIZES)
    assert B == 1 and case["G"] == 1 and len(sizes) == k + w <= D and all(sizes[j] >= 1 for j in range(w)) and S == k + sum(sizes)
    g = _gen(case)
    idx = make_idx(case)
    drop = drop_list(case, idx)
    n = len(drop)
    kept_pos = [S - w + j for j in range(w)] + idx[0, 0].tolist()
    K = torch.zeros(1, H, S, D)
    V = torch.randint(-4, 5, (1, H, S, D), generator=g).float() / 4
    expect = {}
    for h in range(H):
        sz = sizes[:w] + sizes[w + h:] + sizes[w:w + h]                                # the selected rows' sizes rotate per head
        for j, pos in enumerate(kept_pos):
            K[0, h, pos, j] = float(2.0 ** int(torch.randint(-2, 3, (1,), generator=g)))
        grp = torch.tensor([j for j in range(k + w) for _ in range(sz[j] - (1 if j < w else 0))])
        grp = grp[torch.randperm(len(grp), generator=g)]
        assert len(grp) == n - w
        mag = 2.0 ** torch.randint(-3, 4, (n - w,), generator=g).float()
        K[0, h, torch.tensor(drop[:n - w]), grp] = mag
        for r in range(n):
            expect[(h, r)] = int(grp[r]) if r < n - w else r - (n - w)
    return K.to(DT[dt]), V.to(DT[dt]), idx, expect


def make_inputs(case):
    """-> (K, V un-expanded [B, H / G, S, D] on the CPU, idx int64 [B, H, k], expect {(b * H + h, rank): pivot})."""
    from inputs import make_qkv
    if case["data"] == "classes":
        return make_classes(case)
    if case["data"] == "groups":
        return make_groups(case)
    B, H, G, S, D = case["B"], case["H"], case["G"], case["S"], case["D"]
    _, K, V = make_qkv(B, H // G, S, D, case["dt"], case["data"], zlib.crc32(case["name"].encode()) % 100000)
    if case["data"] == "lattice":
        K[:, :, ::3] = (K[:, :, ::3].float() * 0.5).to(K.dtype)                      # different norms, still exact
    return K, V, make_idx(case), {}


def is_exact(case):
    """Built from exact rows: every norm, unit row and similarity is the same number in any summation order.  (Lattice rows against
    lattice rows are not: their unit rows are not lattice values, a similarity may round differently under another fp32 order.)"""
    return case["dt"] != "fp32" and case["data"] in ("groups", "classes")


def run_case(P, O, case, check=True, dev=None):
    """-> dict(route, digest, ok, why, moved, oracle_s)."""
    import numpy as np
    from inputs import checksum
    from merge_bar import check_merge, kernel_pivots
    B, H, G, S, D, w, k = (case[x] for x in ("B", "H", "G", "S", "D", "w", "k"))
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev
    K, V, idx, expect = make_inputs(case)
    kd, vd = K.to(dev), V.to(dev)
    if case["layout"] == "bshd":
        kd, vd = kd.transpose(1, 2).contiguous().transpose(1, 2), vd.transpose(1, 2).contiguous().transpose(1, 2)
        assert kd.stride(2) == (H // G) * D
    km, vm = P.ops.merge_compact(kd, vd, idx.to(dev).int(), w, kv_group=G)
    drop_k, piv_k = kernel_pivots(P.ops, dev, B, H, S)
    route = None
    if P._native.lib.pkv_debug_build() == 1:
        import ctypes
        arr = (ctypes.c_int32 * len(WORDS))()
        P._native.check(P._native.lib.pkv_debug_merge_route(arr, len(WORDS)), "pkv_debug_merge_route")
        route = list(arr)
    km, vm = km.cpu(), vm.cpu()
    res = dict(route=route, digest=checksum(km, vm, torch.from_numpy(drop_k), torch.from_numpy(np.ascontiguousarray(piv_k))), ok=True, why="",
               moved=None, oracle_s=0.0)
    if not check:
        return res
    t0 = time.time()
    try:
        assert drop_k.tolist() == drop_list(case, idx), (case["name"], "drop list is not the complement of the union over batch and heads")
        ke, ve = K.repeat_interleave(G, dim=1), V.repeat_interleave(G, dim=1)
        if case["dt"] == "fp32":                                   # tests/test_gpu_f32.py's bar
            kr, vr = O.merge_kv(ke, ve, idx, w, "pivot")
            close = torch.isclose(km, kr, rtol=2e-5, atol=1e-6).all(-1) & torch.isclose(vm, vr, rtol=2e-5, atol=1e-6).all(-1)
            frac = float(close.float().mean())
            assert frac >= 1.0 - 4.0 / close.numel(), (case["name"], "kept rows off the oracle", frac)
            res["moved"] = int((~close).sum())
        else:
            res["moved"] = check_merge(P.ops, ke, ve, idx, w, km, vm, what=case["name"])
        if is_exact(case):
            assert res["moved"] == 0, (case["name"], "exact rows: K/V must be bit-identical", res["moved"])
            piv_ref = O.merge_pivots(ke, ve, idx, w).reshape(B * H, -1).numpy()
            bad = np.argwhere(piv_ref != piv_k)
            assert len(bad) == 0, (case["name"], "pivots differ from the oracle's at (head, rank, oracle, kernel)",
                                   [(int(a), int(b), int(piv_ref[a, b]), int(piv_k[a, b])) for a, b in bad[:12]], len(bad))
        wrong = [(hr, want, int(piv_k[hr])) for hr, want in expect.items() if int(piv_k[hr]) != want]
        assert not wrong, (case["name"], "planted rows off their pivot: ((head, rank), planted, kernel)", wrong[:12], len(wrong))
    except AssertionError as e:
        res["ok"], res["why"] = False, repr(e)[:1500]
    res["oracle_s"] = round(time.time() - t0, 1)
    return res


def main():
    mode = sys.argv[1]
    import pyramidkv_amd as P
    from oracle import pkv_oracle as O
    cases = {"matrix": CASES, "sweep": sweep_cases(), "knobs-digest": [BY_NAME[n] for n in KNOB_CASES]}[mode]
    props = torch.cuda.get_device_properties(0)
    debug = P._native.lib.pkv_debug_build() == 1
    res = {}
    for case in cases:
        res[case["name"]] = run_case(P, O, case, check=mode != "knobs-digest")
        torch.cuda.empty_cache()
    print(json.dumps({"debug": debug, "cus": props.multi_processor_count,
                      "knobs": {n: os.environ.get(n) for n in KNOBS if os.environ.get(n) is not None}, "cases": res}))


if __name__ == "__main__":
    main()
