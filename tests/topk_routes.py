"""The route matrix of the top-k kernel (tests/test_gpu_topk_routes.py): cases whose row 0 is built for one selection route, run
in a child process - ``python tests/topk_routes.py`` prints one JSON object: per case and variant the routes the debug build
recorded (None on the release library), output digests and whether the outputs equal the oracle.

Route record (pkv_topk.hip, debug build): word 14 of the trace buffer, OR-ed over every launch on row 0 since it was cleared -
bit r + v of the route that wrote the row, bit 32 + g + v of each route that was tried and gave up; v = 8 for the ADA
instantiation (pkv_ada_select), 16 for a segment of a long row."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from inputs import SC_CROWD, SC_DISTINCT, SC_SINK, SC_TINY, SC_ZERO, checksum, make_qkv, plan_qkv  # noqa: E402

ROUTES = ["R1", "R2", "R3", "R4", "R5-rank", "R5-radix", "R5-bitonic"]
GAVE = ["R1", "R2", "R3/R4"]
W = 8


def decode(word):
    """-> (sorted list of "route/variant" exits, sorted list of "route/variant" give-ups)."""
    exits, gave = set(), set()
    for v, name in ((0, "plain"), (8, "ada"), (16, "seg"), (24, "seg-ada")):
        for r, rn in enumerate(ROUTES):
            if word >> (r + v) & 1:
                exits.add(rn + "/" + name)
        for g, gn in enumerate(GAVE):
            if word >> (32 + g + v) & 1:
                gave.add(gn + "/" + name)
    return sorted(exits), sorted(gave)


def race_plan(H, L, Cs, seed, crowd_chunks=None, n_tiny=0):
    """Per head: the sink, 63 distinct normals (list entries 0-63: wave 0's share of the ranking, each its own key bucket), a crowd
    of C - 64 equal normals, `n_tiny` subnormals, the rest zeros.  One positive per 8-key chunk, or the crowd packed 8 to a chunk
    into `crowd_chunks` chunks.  Positions stay clear of wave 0's first 1024 keys so that wave 0 finds every zero it needs there."""
    g = torch.Generator().manual_seed(seed)
    plan = torch.full((H, L), SC_ZERO, dtype=torch.long)
    plan[:, 0] = SC_SINK
    for h in range(H):
        C = Cs[h % len(Cs)]
        nch = L // 8
        free = torch.randperm(nch - 128, generator=g) + 128
        i = 0
        d = free[i:i + 63] * 8 + 1; i += 63
        plan[h, d] = SC_DISTINCT + torch.arange(63)
        if crowd_chunks:
            ch = free[i:i + crowd_chunks]; i += crowd_chunks
            pos = (ch[:, None] * 8 + torch.arange(8)[None]).reshape(-1)[:C - 64]
        else:
            pos = free[i:i + C - 64] * 8 + 2; i += C - 64
        plan[h, pos] = SC_CROWD
        if n_tiny:
            plan[h, free[i:i + n_tiny] * 8 + 3] = SC_TINY
    return plan


def ada_cases():
    """(name, dtype, make inputs -> (q, k, v, plan or None), H, S, base, M, short list?)"""
    def planned(H, S, Cs, dt, seed, **kw):
        return lambda: plan_qkv(race_plan(H, S - W, Cs, seed, **kw), dt)

    def gauss(H, S, dt, seed):
        return lambda: (*make_qkv(1, H, S, 128, dt, "gauss", seed), None)

    return [
        ("r1_gauss", "bf16", gauss(4, 32768, "bf16", 71), 4, 32768, 120, 480, False),
        ("r2_c200", "fp16", planned(4, 32768, (200,), "fp16", 72), 4, 32768, 120, 480, False),
        ("r2_c470_bf16", "bf16", planned(4, 32768, (470,), "bf16", 73), 4, 32768, 120, 480, False),
        # R2 attempted, then the full path: > 512 chunks hold a positive (most only a subnormal in zero's bin) / a crowd of > 512
        # equal normals packed into fewer than k chunks
        ("r2_gives_up_chunks", "fp16", planned(4, 32768, (164,), "fp16", 74, n_tiny=600), 4, 32768, 120, 480, False),
        ("r2_gives_up_crowd", "fp16", planned(4, 32768, (664,), "fp16", 75, crowd_chunks=75), 4, 32768, 120, 480, False),
        ("r3_not_dual", "bf16", gauss(4, 49160, "bf16", 76), 4, 49160, 60, 240, False),
        ("r5_rank", "fp16", gauss(4, 608, "fp16", 77), 4, 608, 30, 120, False),
        ("r5_radix", "bf16", gauss(8, 32768, "bf16", 78), 8, 32768, 125, 1000, False),
        ("r5_bitonic", "fp16", gauss(4, 49160, "fp16", 79), 4, 49160, 150, 600, False),
    ]


def plain_cases():
    """(name, scores [rows, L] on the CPU, k, row stride pad): row 0 is the crafted one."""
    g = torch.Generator().manual_seed(81)
    out = []
    s = torch.rand(2, 32760, generator=g).to(torch.bfloat16)
    out.append(("r1", s, 120, 0))
    out.append(("r3_unaligned", s, 120, 1))                                 # row stride 32761: no 16-byte loads, no algo-1 path
    s = torch.rand(2, 32760, generator=g) * 0.5
    s[:, 8::32] = 0.75                                                      # 1024 equal maxima: 448 < C <= 4096 candidates
    out.append(("r4_unaligned", s.to(torch.float16), 120, 1))
    out.append(("r5_radix", s.to(torch.float16), 1000, 0))
    out.append(("r5_bitonic", s.to(torch.bfloat16), 5000, 0))
    out.append(("r5_rank_short", s[:, :600].to(torch.float16), 120, 0))
    flat = torch.full((2, 32760), 0.25)
    out.append(("r1_gives_up", flat.to(torch.float16), 120, 0))            # every key tied: no prefilter helps
    out.append(("r34_gives_up", flat.to(torch.bfloat16), 120, 1))
    z = torch.zeros(2, 32760)
    z[:, 8 * torch.randperm(4095, generator=g)[:200] + 5] = torch.rand(2, 200, generator=g) + 0.01
    out.append(("r2_plain", z.to(torch.float16), 480, 0))
    out.append(("segmented", torch.rand(2, 70000, generator=g).to(torch.float16), 120, 0))
    return out


def mostly_zero_replay(dt):
    """The inputs of test_gpu_parity.test_topk_rows_that_are_mostly_zero, generated the same way, one row per launch (the route
    record covers row 0): (label, row [1, L], k)."""
    tdt = torch.bfloat16 if dt == "bf16" else torch.float16
    g = torch.Generator().manual_seed(6)
    tiny = 6e-8 if dt == "fp16" else 1e-40
    out = []
    for L in (32760, 8184, 600):
        for npos in (0, 1, 17, 119, 120, 121, 300, 900):
            if npos > L // 2:
                continue
            s = torch.zeros(3, L)
            for r in range(3):
                pos = torch.randperm(L, generator=g)[:npos]
                s[r, pos] = torch.rand(npos, generator=g) * 0.5 + 1e-4
            if npos >= 17:
                s[1, torch.randperm(L, generator=g)[:7]] = tiny
                s[2, :40] = 0.0
            s[0, torch.randperm(L, generator=g)[:50]] = -0.0
            for k in (1, 64, 120, 234, 512):
                if k <= L:
                    for r, tag in ((0, "negzero"), (1, "subnormal" if npos >= 17 else "plain"), (2, "lead40" if npos >= 17 else "plain")):
                        out.append(("L%d_npos%d_k%d_%s" % (L, npos, k, tag), s[r:r + 1].to(tdt), k))
        s = torch.zeros(2, L)
        s[:, 1000 % L: 1000 % L + 400] = torch.rand(2, 400, generator=g) + 0.01 if L > 1400 else 0.0
        out.append(("L%d_bunched_k120" % L, s[:1].to(tdt), 120))
        out.append(("L%d_bunched_k%d" % (L, 512 if L >= 512 else L), s[:1].to(tdt), 512 if L >= 512 else L))
        s = -torch.rand(2, L, generator=g)
        s[:, torch.randperm(L, generator=g)[:200]] = 0.0
        s[:, torch.randperm(L, generator=g)[:30]] = 0.3
        out.append(("L%d_negative_k120" % L, s[:1].to(tdt), 120))
        out.append(("L%d_negative_k%d" % (L, 400 if L >= 400 else L), s[:1].to(tdt), 400 if L >= 400 else L))
    from test_gpu_parity import _negative_zero_walk_rows
    enough, few = _negative_zero_walk_rows()
    out.append(("L32760_negative_zero_walk_k120", enough[:1].to(tdt), 120))
    out.append(("L32760_negative_too_few_zeros_k120", few[:1].to(tdt), 120))
    return out


def main():
    import pyramidkv_amd as P
    from oracle import pkv_oracle as O
    dev = "cuda"
    debug = P._native.lib.pkv_debug_build() == 1
    trace = torch.zeros(32, dtype=torch.int64, device=dev)                 # words 16-23: the budget kernel's stamps
    if debug:
        assert P._native.lib.pkv_debug_topk_trace(trace.data_ptr()) == 0

    def routed(fn):
        trace.zero_()
        torch.cuda.synchronize()
        out = fn()
        torch.cuda.synchronize()
        return out, (int(trace[14].item()) & 0xffffffffffffffff) if debug else None

    res = {}
    for name, s, k, pad in plain_cases():
        if pad:
            buf = torch.zeros(s.shape[0], s.shape[1] + pad, dtype=s.dtype)
            buf[:, :s.shape[1]] = s
            sd = buf.to(dev)[:, :s.shape[1]]
        else:
            sd = s.to(dev)
        idx, word = routed(lambda: P.ops.topk(sd, k))
        ok = torch.equal(idx.cpu().long(), O.topk_canonical(s, k))
        res["plain:" + name] = {"word": word, "digest": checksum(idx), "ok": ok}
    for name, dt, make, H, S, base, M, short in ada_cases():
        q, k, v, plan = make()
        qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
        sg = P.ops.score_window(qd, kd, W, "maxpool", 1, "mean")[0]
        sgc = sg.cpu()
        idx, word = routed(lambda: P.ops.topk(sg, M))
        res["plain:" + name] = {"word": word, "digest": checksum(idx), "ok": torch.equal(idx.cpu().long(), O.topk_canonical(sgc, M))}
        for norm in (True, False):
            mirror = torch.zeros(H, dtype=torch.int64).pin_memory()
            (top, cap, hl, cu, cuh), word = routed(lambda: P.ops.ada_select(qd, kd, W, "maxpool", 1, M, base, 0.2, norm,
                                                                            host_mirror=mirror, host_seq=3))
            ran_out = bool(mirror[0].item() & 0x80000000)
            sidx, caps = O.adakv_head_capacity(sgc[None], base, 0.2, norm)
            ok = torch.equal(top.cpu().long(), O.topk_canonical(sgc, M)) and not ran_out and cap.cpu().tolist() == caps[0].tolist()
            cl = P.AdaKVCluster(window_size=W, kernel_size=1, pooling="maxpool", max_capacity_prompt=base + W, floor=0.2, normalize=norm)
            kf, vf = cl.update_kv(kd, qd, vd)
            kr, vr, _ = O._flat_gather(k, v, [sidx[0, h, :int(caps[0, h])] for h in range(H)], W)
            ok = ok and torch.equal(kf.cpu(), kr) and torch.equal(vf.cpu(), vr)
            res["ada%s:%s" % ("_norm" if norm else "", name)] = {"word": word, "digest": checksum(top, cap, kf, vf), "ok": ok}
    if debug:
        for dt in ("fp16", "bf16"):
            for label, s, k in mostly_zero_replay(dt):
                sd = s.to(dev)
                idx, word = routed(lambda: P.ops.topk(sd, k))
                res["zero_%s:%s" % (dt, label)] = {"word": word, "digest": checksum(idx),
                                                   "ok": torch.equal(idx.cpu().long(), O.topk_canonical(s, k))}
        P._native.lib.pkv_debug_topk_trace(None)
    print(json.dumps({"debug": debug, "cases": res}))


if __name__ == "__main__":
    main()
