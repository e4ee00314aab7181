"""The route matrix of pass 1 of the H2O score kernels (tests/test_gpu_h2o_routes.py, tests/test_h2o_routes_plan.py).

Every workgroup of h2o_stats_kernel (pyramidkv_amd/csrc/pkv_h2o.hip: 256 query rows of one head) takes one of four paths:

  frozen  no row's first 16 logits span more than H2O_WIDE = 40: tile 0 with the tracked maximum, all later tiles with the
          frozen reference point (per lane group: the maximum over its 16 keys of tile 0), finish(true) finds no overflow;
  repeat  frozen, but some row's Z overflowed: a lane's sum beyond the fp32 maximum ("repeat-inf"), or only the merged sum
          of the four lane groups above 2^120 ("repeat-2p120"); tile 0 is staged again and the rows run once more, tracked;
  wide    some row's first 16 logits span more than 40: tracked maximum from the start;
  short   t_plain == 0 (S - w < 64): tracked maximum, every tile through the edge body.

``h2o_route_plan`` restates that per workgroup from the oracle's own rounded, scaled, corner-masked logits in float64, with the
margins that decide it; ``h2o_route_words`` restates the host words of the debug library's record (pkv_debug_h2o_route,
include/pkv.h); ``crow_f32`` restates the kernel's pass-1 arithmetic in numpy float32 (reference point per lane group, 4-key
partial sums, the two-step merge, c_row = -(m log2e + log2 Z)) and ``crow_ref`` is the float64 reference of c_row.

The new cases are lattice inputs with one planted key (only dimension 0 non-zero) and dimension 0 of a range of query rows set
to 4.0: every product is exact, so the kernel's logits are the oracle's bit for bit and the route cannot depend on a rounding.

Run as a child process, ``python tests/h2o_routes.py matrix`` prints one JSON object: per case the recorded host words and
per-workgroup codes (None on the release library), a digest of the scores, ok / why, and the worst c_row error in units of
``crow_unit`` for the GPU and for the float32 restatement.  ``matrix --record PATH`` also writes those ratios to PATH."""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

WORDS = ["dtype", "KS", "stats_grid_x", "stats_grid_y", "colsum_grid_x", "colsum_grid_y", "ntiles", "t_plain", "stats_lds", "colsum_lds",
         "stats_dyn_lds", "colsum_dyn_lds", "n_frozen", "n_repeat", "n_wide", "n_short"]
FROZEN, REPEAT, WIDE, SHORT = 1, 2, 3, 4
NAMES = {FROZEN: "frozen", REPEAT: "repeat", WIDE: "wide", SHORT: "short"}
H2O_WIDE = 40.0                       # pkv_h2o.hip
LN_F32_MAX = math.log(3.4028234663852886e38)      # 88.72: a lane's Z beyond it is inf
LN_2P120 = 120 * math.log(2.0)                    # 83.18: finish() calls a merged zz above 2^120 an overflow
MARGIN_LN, MARGIN_SPAN = 2.0, 5.0
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
L2E32 = np.float32(1.44269504088896340736)


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------- restatements
def h2o_logits(q, kx, w):
    """The oracle's logits of pyramidkv_utils.py:544-551 (model-dtype matmul, / sqrt(D), both rounded) as float64 numpy
    [B, H, S, S]; the masked corner (finfo.min added there) is -inf."""
    from oracle import pkv_oracle as O
    S, D = q.shape[-2], q.shape[-1]
    x = O._scale(torch.matmul(q, kx.transpose(2, 3)), D, "div").double().numpy()
    r = np.arange(w)
    x[:, :, S - w:, S - w:][:, :, r[None, :] > r[:, None]] = -np.inf
    return x


def _lse(a, axis):
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.log(np.sum(np.exp(a - m), axis=axis)) + np.squeeze(m, axis)


def plan_from_logits(x, w):
    """-> one dict per (b * H + h, workgroup): route, kind, and the margins that decide it.  Lane group lg owns the keys with
    (j % 16) // 4 == lg; its reference point is its maximum over keys < 64; rows past S are row S - 1 (the kernel clamps)."""
    B, H, S, _ = x.shape
    L = S - w
    t_plain = L // 64
    x = x.reshape(B * H, S, S)
    grp = (np.arange(S) % 16) // 4
    out = []
    for bh in range(B * H):
        for g in range(_cdiv(S, 256)):
            rows = np.minimum(np.arange(g * 256, g * 256 + 256), S - 1)
            xr = x[bh, rows]                                                  # [256, S]
            rec = dict(bh=bh, wg=g, ragged=g * 256 + 256 > S, corner=g * 256 + 256 > L, span=None, lane_lnz=None, merged_lnzz=None)
            if t_plain == 0:
                rec.update(route=SHORT, kind="short")
                out.append(rec)
                continue
            span = float(np.max(xr[:, :16].max(1) - xr[:, :16].min(1)))
            rec["span"] = span
            if span > H2O_WIDE:
                rec.update(route=WIDE, kind="wide")
                out.append(rec)
                continue
            m = np.stack([xr[:, :64][:, grp[:64] == lg].max(1) for lg in range(4)], 1)                  # [256, 4] frozen points
            lnz = np.stack([_lse(xr[:, grp == lg] - m[:, lg:lg + 1], 1) for lg in range(4)], 1)        # ln Z per lane group
            lnzz = _lse(lnz + m, 1) - m.max(1)                                                        # after the lane merge
            rec["lane_lnz"], rec["merged_lnzz"] = float(lnz.max()), float(lnzz.max())
            if rec["lane_lnz"] > LN_F32_MAX:
                rec.update(route=REPEAT, kind="repeat-inf")
            elif rec["merged_lnzz"] > LN_2P120:
                rec.update(route=REPEAT, kind="repeat-2p120")
            else:
                rec.update(route=FROZEN, kind="frozen")
            out.append(rec)
    return out


def h2o_route_plan(q, kx, w):
    """q [B, H, S, D], kx = K expanded to the H query heads, both on the CPU."""
    return plan_from_logits(h2o_logits(q, kx, w), w)


def margins_clear(rec):
    """'' when every margin that decides ``rec``'s route is clear of its threshold (2.0 in ln units, 5 in span units), so that no
    difference in exp or summation order can flip it; else what is too close."""
    if rec["route"] == SHORT:
        return ""
    if abs(rec["span"] - H2O_WIDE) < MARGIN_SPAN:
        return "span %.2f within %g of %g" % (rec["span"], MARGIN_SPAN, H2O_WIDE)
    if rec["route"] == WIDE:
        return ""
    if abs(rec["lane_lnz"] - LN_F32_MAX) < MARGIN_LN:
        return "lane ln Z %.2f within %g of %.2f" % (rec["lane_lnz"], MARGIN_LN, LN_F32_MAX)
    if rec["kind"] != "repeat-inf" and abs(rec["merged_lnzz"] - LN_2P120) < MARGIN_LN:       # an inf lane decides alone
        return "merged ln zz %.2f within %g of %.2f" % (rec["merged_lnzz"], MARGIN_LN, LN_2P120)
    return ""


def h2o_route_words(dt, B, H, S, D, w):
    """The twelve host words of pkv_debug_h2o_route (launch_h2o_stats, launch_h2o_colsum)."""
    ks = D // 32
    lds1 = 2 * 64 * 4 * ks * 16
    lds2 = lds1 + 2 * 64 * 4
    return dict(dtype={"bf16": 0, "fp16": 1}[dt], KS=ks, stats_grid_x=_cdiv(S, 256), stats_grid_y=B * H, colsum_grid_x=_cdiv(S - w, 256),
                colsum_grid_y=B * H, ntiles=_cdiv(S, 64), t_plain=(S - w) // 64, stats_lds=lds1, colsum_lds=lds2,
                stats_dyn_lds=int(lds1 >= 65536), colsum_dyn_lds=int(lds2 >= 65536))


def cells(plan, ks):
    out = set()
    for r in plan:
        out.add("%s/KS%d" % (r["kind"], ks))
        if r["route"] == REPEAT and r["ragged"]:
            out.add("repeat in a ragged workgroup")
        if r["route"] == REPEAT and r["corner"]:
            out.add("repeat with the corner in the workgroup")
    if len({r["route"] for r in plan}) > 1:
        out.add("paths mixed in one launch")
    return out


def crow_ref(x):
    """c_ref[i] = -log2 sum_j exp(x_ij) in float64, [B*H, S]."""
    B, H, S, _ = x.shape
    return -_lse(x.reshape(B * H, S, S), 2) / math.log(2.0)


def crow_unit(x, cref):
    """The unit of the c_row comparison: the rounding of the exponent argument (|x| log2e), of m log2e and the result (|c_row|),
    and the worst-case fp32 sum of a lane's S/16 partial adds plus the merge."""
    B, H, S, _ = x.shape
    ax = np.abs(np.where(np.isfinite(x), x, 0.0)).max(-1).reshape(B * H, S)
    return 2.0 ** -24 * (ax * math.log2(math.e) + np.abs(cref) + 1.0) + 2.0 ** -24 * (S / 16 + 6) / math.log(2.0)


def _fma32(a, b, c):
    """fp32 fma of fp32 a (at most 11 significant bits: a model-dtype logit), b, c: the product is exact in float64."""
    with np.errstate(invalid="ignore"):
        return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def crow_f32(x, w, routes, drop=None, twice=None, no_reset=None):
    """pass 1 of h2o_stats_kernel in numpy float32 for the per-workgroup ``routes`` (plan order) -> c_row [B*H, S] float32.
    Mutations, to prove that the c_row bar bites: ``drop`` = (bh, row, key) leaves one key out of one row, ``twice`` counts it
    twice; ``no_reset`` = "all" leaves out the reset of m / mL / Z before the second loop of a repeating workgroup, "Z" leaves
    out the reset of Z alone (which the kernel absorbs: with m = -inf the first rescale sets Z = 0)."""
    B, H, S, _ = x.shape
    L = S - w
    BH, nwg, t_plain = B * H, _cdiv(S, 256), (S - w) // 64
    xs = x.reshape(BH, S, S).astype(np.float32)
    Sp = _cdiv(S, 64) * 64
    xp = np.full((BH, S, Sp), -np.inf, np.float32)               # keys past S: -inf (the edge body)
    xp[:, :, :S] = xs
    extra = np.zeros((BH, S, Sp), np.float32)                    # the mutations, as a weight on exp
    if drop:
        extra[drop] = -1.0
    if twice:
        extra[twice] = 1.0
    route_of_row = np.repeat(np.asarray(routes, np.int32).reshape(BH, nwg), 256, axis=1)[:, :S]      # [BH, S]

    def loop(m, mL, Z, tracked_rows):
        """all steps of 4 keys per lane group; ``tracked_rows`` [BH, S] bool: tracked maximum in every tile (else tile 0 only)"""
        with np.errstate(over="ignore", invalid="ignore"):
            for s0 in range(0, Sp, 16):
                x4 = xp[:, :, s0:s0 + 16].reshape(BH, S, 4, 4)                       # [.., lane group, r]
                e4 = extra[:, :, s0:s0 + 16].reshape(BH, S, 4, 4)
                track = (tracked_rows | (s0 < 64))[:, :, None]
                mx = np.maximum(x4.max(-1), m)
                up = track & (mx > m)
                scale = np.exp2(((np.where(np.isfinite(m), m, np.float32(0)) - mx) * L2E32).astype(np.float32)).astype(np.float32)
                Zs = np.where(np.isneginf(m), np.float32(0), (Z * scale).astype(np.float32))
                Z = np.where(up, Zs, Z)
                m = np.where(up, mx, m)
                mL = np.where(up, np.where(np.isneginf(mx), np.float32(0), (-mx * L2E32).astype(np.float32)), mL)
                y = _fma32(x4, L2E32, np.broadcast_to(mL[..., None], x4.shape))
                e = np.exp2(y).astype(np.float32)
                e = (e + e * e4).astype(np.float32)
                Z = (Z + ((e[..., 0] + e[..., 1]).astype(np.float32) + (e[..., 2] + e[..., 3]).astype(np.float32)).astype(np.float32)).astype(np.float32)
        return m, mL, Z

    def merged(m, Z):
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            def step(ma, za, mb, zb):
                mn = np.maximum(ma, mb)
                fa = np.where(np.isneginf(ma), np.float32(0), (za * np.exp2(((ma - mn) * L2E32).astype(np.float32))).astype(np.float32))
                fb = np.where(np.isneginf(mb), np.float32(0), (zb * np.exp2(((mb - mn) * L2E32).astype(np.float32))).astype(np.float32))
                return mn, (fa + fb).astype(np.float32)
            m01, z01 = step(m[..., 0], Z[..., 0], m[..., 1], Z[..., 1])              # lanes xor 16
            m23, z23 = step(m[..., 2], Z[..., 2], m[..., 3], Z[..., 3])
            mm, zz = step(m01, z01, m23, z23)                                        # lanes xor 32
            return -((mm * L2E32).astype(np.float32) + np.log2(zz).astype(np.float32)).astype(np.float32)

    init = lambda: (np.full((BH, S, 4), -np.inf, np.float32), np.zeros((BH, S, 4), np.float32), np.zeros((BH, S, 4), np.float32))   # noqa: E731
    tracked = (route_of_row == WIDE) | (route_of_row == SHORT)
    m, mL, Z = loop(*init(), tracked)
    c = merged(m, Z)
    rep = route_of_row == REPEAT
    if rep.any():
        if no_reset == "all":
            m2, mL2, Z2 = m, mL, Z
        else:
            m2, mL2, Z2 = init()
            if no_reset == "Z":
                Z2 = Z
        m2, _, Z2 = loop(m2, mL2, Z2, np.ones_like(rep))
        c = np.where(rep, merged(m2, Z2), c)
    assert t_plain > 0 or (route_of_row == SHORT).all()
    return c


def crow_ratio(c, cref, unit):
    with np.errstate(invalid="ignore"):
        r = np.abs(c.astype(np.float64) - cref) / unit
    return float(np.nan_to_num(r, nan=np.inf).max())


# ---------------------------------------------------------------------------------------------- cases
def _case(name, S, w, D, rows, key, k0, want, cell, **kw):
    return dict(name=name, S=S, w=w, D=D, rows=rows, key=key, k0=k0, want=want, cells=set(cell), B=1, H=1, G=1, data="planted_lattice", **kw)


# want: {workgroup: route}; every other workgroup is frozen.  cells: what the case is built for (KS is appended by the tests).
PLANTED = [
    _case("repeat_wg0", 1200, 8, 128, (0, 256), 700, 424, {0: REPEAT}, ["repeat-inf", "frozen", "paths mixed in one launch"]),
    _case("repeat_one_row", 1200, 8, 128, (600, 601), 100, 424, {2: REPEAT}, ["repeat-inf"]),
    _case("repeat_last_wg_edge_key", 1200, 8, 128, (1100, 1200), 1190, 424, {4: REPEAT}, ["repeat-inf", "repeat in a ragged workgroup"]),
    _case("repeat_corner_key", 1200, 8, 128, (1024, 1200), 1196, 424, {4: REPEAT}, ["repeat-inf", "repeat with the corner in the workgroup"]),
    _case("finite_above_2p120", 1200, 8, 128, (300, 400), 900, 244, {1: REPEAT}, ["repeat-2p120"]),
    _case("frozen_large_Z", 1200, 8, 128, (300, 400), 900, 198, {}, ["frozen"]),
    _case("tile0_beyond_look", 1200, 8, 128, (0, 256), 40, 424, {}, ["frozen"]),
    # the rows outside the planted range look away from the planted key (q0 = 0): with the lattice's q0 = +-1 their first 16
    # logits span 38.5 - 38.8 in workgroups 1-4, a frozen route 1.2 below H2O_WIDE - the right cell, but not by the margin of 5
    # the plan test asks for
    _case("wide_look", 1200, 8, 128, (0, 256), 7, 424, {0: WIDE}, ["wide", "frozen", "paths mixed in one launch"], q0_else=0.0),
    _case("repeat_d64", 700, 8, 64, (256, 512), 300, 300, {1: REPEAT}, ["repeat-inf", "frozen"]),
    _case("repeat_d256", 700, 16, 256, (256, 512), 300, 600, {1: REPEAT}, ["repeat-inf", "frozen"]),
    _case("repeat_t_plain1", 100, 8, 128, (0, 100), 80, 424, {0: REPEAT}, ["repeat-inf", "repeat in a ragged workgroup"]),
    _case("short", 40, 8, 128, (0, 40), 20, 424, {0: SHORT}, ["short"]),
    # the corner (keys 1136..1199) straddles tiles 17 and 18 inside the repeating last workgroup; rows >= 1150 see the key
    _case("repeat_w64_corner_two_tiles", 1200, 64, 128, (1024, 1200), 1150, 424, {4: REPEAT},
          ["repeat-inf", "repeat with the corner in the workgroup", "repeat in a ragged workgroup"]),
    # the other head sizes of the 2^120 threshold, the look and the short prompt (logit 86.0: exact in both dtypes at both sizes)
    _case("finite_above_2p120_d64", 700, 8, 64, (300, 400), 600, 172, {1: REPEAT}, ["repeat-2p120"]),
    _case("finite_above_2p120_d256", 700, 8, 256, (300, 400), 600, 344, {1: REPEAT}, ["repeat-2p120"]),
    _case("wide_look_d64", 700, 8, 64, (0, 256), 7, 300, {0: WIDE}, ["wide"], q0_else=0.0),
    _case("wide_look_d256", 700, 8, 256, (0, 256), 7, 600, {0: WIDE}, ["wide"], q0_else=0.0),
    _case("short_d64", 40, 8, 64, (0, 40), 20, 300, {0: SHORT}, ["short"]),
    _case("short_d256", 50, 16, 256, (0, 50), 20, 600, {0: SHORT}, ["short"]),
]
# B = 2, H = 4, G = 2 on token-major strided views (tests/test_gpu_configs.py::test_h2o_strided_views_gqa_batch): the planted rows
# differ per head - workgroup 1 of head 1 repeats, workgroup 1 of head 0 (same keys) does not; head 2 looks at no planted row
GQA = dict(name="repeat_gqa_strided", S=700, w=8, D=128, B=2, H=4, G=2, data="gqa", key=300, k0=424,
           rows={0: (512, 700), 1: (256, 512), 3: (0, 256)},
           want={(0, 2): REPEAT, (1, 1): REPEAT, (3, 0): REPEAT}, cells={"repeat-inf", "frozen", "paths mixed in one launch", "repeat in a ragged workgroup"})
# the four inputs of tests/test_gpu_parity.py::test_h2o_scores_key_norm_outliers, unchanged; the cells are what the record shows
LEGACY_NAMES = ["outlier_keys_no_row_looks_at", "outlier_in_the_look_of_wg0", "large_logits", "wide_rows_tracked"]
LEGACY = [dict(name="legacy_" + n, legacy=n, S=1200, w=8, D=128, B=1, H=2, G=1, data="legacy", cells=set(c),
               want=({(h, g): r for h in range(2) for g, r in wg.items()}))
          for n, wg, c in (
              (LEGACY_NAMES[0], {}, ["frozen"]),
              (LEGACY_NAMES[1], {0: WIDE}, ["wide", "frozen", "paths mixed in one launch"]),
              (LEGACY_NAMES[2], {g: WIDE for g in range(5)}, ["wide"]),
              (LEGACY_NAMES[3], {g: WIDE for g in range(5)}, ["wide"]))]
CASES = [dict(c, dt=dt) for c in PLANTED + [GQA] + LEGACY for dt in ("bf16", "fp16")]
MATRIX = {"%s/KS%d" % (r, ks) for r in ("frozen", "repeat-inf", "repeat-2p120", "wide", "short") for ks in (2, 4, 8)} | {
    "repeat in a ragged workgroup", "repeat with the corner in the workgroup", "paths mixed in one launch"}


def case_id(c):
    return "%s-%s" % (c["name"], c["dt"])


BY_ID = {case_id(c): c for c in CASES}


def want_routes(c):
    """The intended route of every workgroup, in the order of the record (slot bh * grid.x + workgroup)."""
    nwg = _cdiv(c["S"], 256)
    out = []
    for bh in range(c["B"] * c["H"]):
        for g in range(nwg):
            if c["data"] == "planted_lattice":
                out.append(c["want"].get(g, FROZEN))
            else:
                out.append(c["want"].get((bh % c["H"], g), FROZEN))
    return out


def legacy_outlier_inputs(name, dt):
    """(q, k) of one case of test_h2o_scores_key_norm_outliers ([1, 2, 1200, 128], window 8), on the CPU."""
    from inputs import make_qkv
    # large logits on the lattice: every q.k is an exact multiple of 16 below 2^15 (no accumulation-order rounding of the
    # model-dtype logits, whose unit is up to 4 there - one flipped logit moves a probability by several per cent)
    q, k, _ = make_qkv(1, 2, 1200, 128, dt, "lattice" if name in ("large_logits", "wide_rows_tracked") else "gauss", 97)
    if name == "outlier_keys_no_row_looks_at":
        q[..., 0] = 0
        k[:, :, 5::300, :] = 0
        k[:, :, 5::300, 0] = 3000.0 if dt == "bf16" else 2000.0           # no row has a component along them: they score exactly 0
    elif name == "outlier_in_the_look_of_wg0":
        q[:, :, :256, :] *= 0.01                                          # first workgroup: queries along the outlier key 7,
        q[:, :, :256, 0] = 3.0                                            # inside the 16-key look: a span of ~400
        q[:, :, 256:, 0] = 0                                              # all other rows look away from it
        k[:, :, 7, :] = 0
        k[:, :, 7, 0] = 1500.0
    elif name == "large_logits":
        q *= 16
        k *= 16                                                           # logits ~ N(0, 106^2): row maxima ~ 350
    else:
        assert name == "wide_rows_tracked"
        q *= 8
        k *= 8                                                            # logits ~ N(0, 27^2): a 16-key sample spans ~90, row maxima ~ +70 above it
    return q, k


def make_inputs(c):
    """-> (q [B, H, S, D], k, v un-expanded [B, H / G, S, D]) on the CPU; the GQA case as token-major strided views."""
    from inputs import make_qkv
    S, D, dt = c["S"], c["D"], c["dt"]
    if c["data"] == "legacy":
        q, k = legacy_outlier_inputs(c["legacy"], dt)
        return q, k, make_qkv(1, 2, S, D, dt, "lattice", 98)[2]
    if c["data"] == "planted_lattice":
        q, k, v = make_qkv(1, 1, S, D, dt, "lattice", 5)
        if "q0_else" in c:
            q[..., 0] = c["q0_else"]
        k[0, 0, c["key"], :] = 0
        k[0, 0, c["key"], 0] = c["k0"]
        q[0, 0, c["rows"][0]:c["rows"][1], 0] = 4.0
        return q, k, v
    B, H, G = c["B"], c["H"], c["G"]
    g = torch.Generator().manual_seed(5)
    lat = lambda *shape: (torch.randint(-4, 5, shape, generator=g).float() / 4).to(DT[dt])      # noqa: E731
    q_tm, k_tm, v_tm = lat(B, S, H, D), lat(B, S, H // G, D + 64), lat(B, S, H // G, D)          # K: padded rows, 64-byte offset
    q, k, v = q_tm.permute(0, 2, 1, 3), k_tm[..., 32:32 + D].permute(0, 2, 1, 3), v_tm.permute(0, 2, 1, 3)
    k[:, :, c["key"], :] = 0
    k[:, :, c["key"], 0] = c["k0"]
    for h, (r0, r1) in c["rows"].items():
        q[:, h, r0:r1, 0] = 4.0
    return q, k, v


def case_plan(c, q=None, k=None):
    """-> (logits float64, plan) of a case."""
    if q is None:
        q, k, _ = make_inputs(c)
    x = h2o_logits(q.contiguous(), k.contiguous().repeat_interleave(c["G"], dim=1), c["w"])
    return x, plan_from_logits(x, c["w"])


# ---------------------------------------------------------------------------------------------- GPU
def check_scores(P, O, c, q, k, v, qd, kd, vd, got):
    """Part c: scores within score_bar's bar (lattice inputs: within 1 ulp), two calls bit-identical, the H2O selection at 32
    kept keys the canonical top-k of the kernel's own scores, K/V the oracle's gather."""
    from score_bar import check_h2o_scores
    w, G = c["w"], c["G"]
    ke, ve = k.contiguous().repeat_interleave(G, dim=1), v.contiguous().repeat_interleave(G, dim=1)
    gotc = got.cpu()
    again = P.ops.score_h2o(qd, kd, w, kv_group=G).cpu()
    assert torch.equal(gotc.view(torch.int16), again.view(torch.int16)), (case_id(c), "two calls differ")
    assert torch.isfinite(gotc.float()).all(), (case_id(c), "non-finite score")
    want = O.h2o_scores(q.contiguous(), ke, w)
    # probabilities below 2^-126 are +0 on the GPU (hardware exp2, MFMA operands): scores down there come out as 0
    tiny = want.float().abs() < 1e-35
    assert (gotc.float()[tiny].abs() < 1e-35).all(), (case_id(c), "a score below 1e-35 did not come out tiny")
    chk = gotc.clone()
    chk[tiny] = want[tiny]
    rep = check_h2o_scores(q.contiguous(), ke, w, chk, what=case_id(c))
    if c["data"] != "legacy" or c["legacy"] in ("large_logits", "wide_rows_tracked"):
        assert rep["max_ulp"] <= 1, (case_id(c), "lattice inputs: beyond 1 ulp", rep)
    kk = min(32, c["S"] - w)
    kc, vc, idx = P.ops.compress(qd, kd, vd, w, kk, None, 1, kv_group=G, h2o=True, return_indices=True)
    ic = idx.cpu().long()
    assert torch.equal(ic, O.topk_canonical(gotc, kk)), (case_id(c), "indices are not the canonical top-k of the kernel's scores")
    kr, vr = O.gather_compact(ke, ve, ic, w)
    assert torch.equal(kc.cpu(), kr) and torch.equal(vc.cpu(), vr), (case_id(c), "compacted K/V")
    return rep


def device_inputs(c, q, k, v):
    """The case's tensors on the device; the GQA case keeps its token-major strides (K: padded rows, 64-byte offset)."""
    if c["data"] != "gqa":
        return q.to("cuda"), k.to("cuda"), v.to("cuda")
    D = c["D"]
    tm = lambda t: t.permute(0, 2, 1, 3).contiguous().to("cuda")      # noqa: E731
    k_tm = torch.zeros(c["B"], c["S"], c["H"] // c["G"], D + 64, dtype=k.dtype, device="cuda")
    k_tm[..., 32:32 + D] = tm(k)
    qd, kd, vd = tm(q).permute(0, 2, 1, 3), k_tm[..., 32:32 + D].permute(0, 2, 1, 3), tm(v).permute(0, 2, 1, 3)
    assert qd.stride(2) == c["H"] * D and kd.stride(2) == (c["H"] // c["G"]) * (D + 64)
    return qd, kd, vd


def run_case(P, O, c):
    """One case on the loaded library -> dict(words, codes, digest, ok, why, crow_gpu, crow_cpu, rep).  On the debug library the
    record and c_row are read back and c_row is measured against the float64 reference (main() and the GPU test hold it to
    the bar, which needs the float32 restatement's worst ratio over ALL cases)."""
    import ctypes
    from inputs import checksum
    w, G, B, H, S = c["w"], c["G"], c["B"], c["H"], c["S"]
    res = dict(words=None, codes=None, digest=None, ok=True, why="", crow_gpu=None, crow_cpu=None, rep=None)
    q, k, v = make_inputs(c)
    qd, kd, vd = device_inputs(c, q, k, v)
    got = P.ops.score_h2o(qd, kd, w, kv_group=G)
    try:
        if P._native.lib.pkv_debug_build() == 1:
            lib = P._native.lib
            arr = (ctypes.c_int32 * len(WORDS))()
            P._native.check(lib.pkv_debug_h2o_route(arr, len(WORDS)), "pkv_debug_h2o_route")
            nwg, nrows = B * H * _cdiv(S, 256), B * H * S
            codes, crow = np.zeros(nwg, np.int32), np.zeros(nrows, np.float32)
            P._native.check(lib.pkv_debug_h2o_rows(codes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), nwg,
                                                   crow.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), nrows), "pkv_debug_h2o_rows")
            res["words"], res["codes"] = list(arr), codes.tolist()
            x, plan = case_plan(c, q, k)
            cref = crow_ref(x)
            unit = crow_unit(x, cref)
            res["crow_gpu"] = crow_ratio(crow.reshape(B * H, S), cref, unit)
            res["crow_cpu"] = crow_ratio(crow_f32(x, w, [r["route"] for r in plan]), cref, unit)
            assert np.isfinite(crow).all(), (case_id(c), "non-finite c_row")
        res["digest"] = checksum(got)
        res["rep"] = check_scores(P, O, c, q, k, v, qd, kd, vd, got)
    except AssertionError as e:
        res["ok"], res["why"] = False, repr(e)[:1500]
    return res


def crow_bar(cpu_ratios):
    """K = 4 x max(worst ratio of the float32 restatement over all cases, 1): numpy rounds exp2 and log2 correctly, the factor 4
    is for the two hardware approximations (v_exp_f32, v_log_f32)."""
    return 4.0 * max(max(cpu_ratios), 1.0)


def main():
    mode = sys.argv[1]
    assert mode == "matrix"
    import pyramidkv_amd as P
    from oracle import pkv_oracle as O
    res = {}
    for c in CASES:
        res[case_id(c)] = run_case(P, O, c)
    out = {"debug": P._native.lib.pkv_debug_build() == 1, "cases": res}
    if out["debug"]:
        out["crow_bar"] = crow_bar([r["crow_cpu"] for r in res.values() if r["crow_cpu"] is not None])
        for cid, r in res.items():
            if r["crow_gpu"] is None or not r["crow_gpu"] <= out["crow_bar"]:
                r["ok"], r["why"] = False, (r["why"] + " c_row beyond the bar: %r > %r" % (r["crow_gpu"], out["crow_bar"])).strip()
    if "--record" in sys.argv:
        rec = {cid: {"gpu": r["crow_gpu"], "f32_restatement": r["crow_cpu"]} for cid, r in res.items()}
        worst = {"gpu": max(r["gpu"] for r in rec.values()), "f32_restatement": max(r["f32_restatement"] for r in rec.values())}
        with open(sys.argv[sys.argv.index("--record") + 1], "w") as f:
            json.dump({"what": "worst |c_row - c_ref| / u_i per case (tests/h2o_routes.py: crow_ref, crow_unit); gpu = h2o_stats_kernel of "
                               "the debug library, f32_restatement = crow_f32 (numpy float32)", "worst": worst, "cases": rec}, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
