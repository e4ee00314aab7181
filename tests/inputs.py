"""Deterministic synthetic inputs shared by tests, golden generation, smoke and bench.

All generation happens on the CPU generator (bit-reproducible across machines with the same
torch build); tensors are moved to the device afterwards.
"""
import numpy as np
import torch

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def make_qkv(B, H, S, D, dtype, kind, seed, device="cpu"):
    """kind:
      gauss    N(0,1) fp32 -> cast (SURVEY section 8d 'tier B')
      lattice  values in {-4..4}/4: every q.k dot product is exact in fp32 in any order ('tier A')
      planted  gauss background + a few hundred 'heavy hitter' keys whose logits are
               well separated, so selection is robust to 1-ulp score noise
      sink     what a real prompt looks like to this path (round 6): logits with standard deviation 6 (q, k ~ N(0, 6^(1/2)))
               and an attention-sink key at position 0 that every one of the last 64 queries scores at exactly +40: next
               to it exp(x - 40) underflows for all but a handful of keys - in fp16 most pooled scores are exactly 0 and
               the k-th largest is tied thousands of times (bf16 keeps fp32's exponent range: a peaked row without ties)
    """
    g = torch.Generator().manual_seed(seed)
    dt = DTYPES[dtype] if isinstance(dtype, str) else dtype
    if kind == "gauss":
        q, k, v = (torch.randn(B, H, S, D, generator=g) for _ in range(3))
    elif kind == "lattice":
        q, k, v = (torch.randint(-4, 5, (B, H, S, D), generator=g).float() / 4 for _ in range(3))
    elif kind == "planted":
        # tiny background + 64 heavy-hitter keys aligned with a direction u shared by the window
        # queries; hitter logits are ~0.1 apart (>> 1 ulp of the score dtype after softmax)
        q = torch.randn(B, H, S, D, generator=g) * 0.02
        k = torch.randn(B, H, S, D, generator=g) * 0.02
        v = torch.randn(B, H, S, D, generator=g)
        n_hit = 64
        for b in range(B):
            for h in range(H):
                pos = (torch.randperm((S - 128) // 16, generator=g)[:n_hit] * 16 + 8) if S >= 2048 else torch.arange(0)
                u = torch.randn(D, generator=g)
                u = u / u.norm()
                q[b, h, -64:] += 6.0 * u
                strength = torch.linspace(2.0, 14.0, len(pos))
                k[b, h, pos] += strength[:, None] * u
    elif kind == "sink":
        a = 6.0 ** 0.5
        q = torch.randn(B, H, S, D, generator=g) * a
        k = torch.randn(B, H, S, D, generator=g) * a
        v = torch.randn(B, H, S, D, generator=g)
        u = torch.randn(B, H, 1, D, generator=g)
        u = u / u.norm(dim=-1, keepdim=True)
        nq = min(64, S)
        qw = q[:, :, -nq:]
        q[:, :, -nq:] = qw - (qw * u).sum(-1, keepdim=True) * u + 4.0 * u      # component along u: exactly 4
        k[:, :, 0:1] = (40.0 * D ** 0.5 / 4.0) * u                             # q . k0 / sqrt(D) = 40
    else:
        raise ValueError(kind)
    return q.to(dt).to(device), k.to(dt).to(device), v.to(dt).to(device)


def bits(t: torch.Tensor) -> np.ndarray:
    """Bit pattern of a tensor as a numpy integer array (bf16/fp16 -> uint16, fp32 -> uint32)."""
    t = t.detach().cpu().contiguous()
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16).numpy().view(np.uint16)
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.numpy()


def from_bits(a: np.ndarray, dtype) -> torch.Tensor:
    dt = DTYPES[dtype] if isinstance(dtype, str) else dtype
    if dt in (torch.bfloat16, torch.float16):
        return torch.from_numpy(a.view(np.int16).copy()).view(dt)
    return torch.from_numpy(a.view(np.int32).copy()).view(dt)


def checksum(*tensors) -> int:
    """Order-sensitive 63-bit checksum of bit patterns."""
    acc = 0
    for t in tensors:
        a = bits(t).astype(np.uint64).ravel()
        wts = (np.arange(a.size, dtype=np.uint64) % np.uint64(65521)) + np.uint64(1)
        acc = (acc * 1000003 + int((a * wts).sum() % np.uint64(2**61 - 1))) % (2**63 - 1)
    return acc


# ---- score-class plans: q/k/v whose window scores are known position by position (tests/test_gpu_topk_routes.py) ----
# The window queries are e0 and key j is c_j * e0 (its other coordinates only make the K/V rows distinct): every product q . k_j is
# c_j exactly, so every logit is a value chosen on the model dtype's grid, the sink key at position 0 holds the maximum m, and the
# fp32 softmax puts each position in one class, far from every rounding boundary of the model dtype:
SC_ZERO = 0        # exact zero: the probability underflows in the model dtype (logit 0, gap m to the sink)
SC_TINY = 1        # one shared subnormal: the smallest (code 1), the only positive value in zero's 8-key histogram bin of the top-k
                   # kernel (keys carry a bias: zero's key sits 6 above its bin's lower edge, pkv_common.hpp KeyBias)
SC_CROWD = 2       # one shared normal value below every distinct one (a crowded key bucket)
SC_SINK = 3        # position 0 only: the row maximum
SC_DISTINCT = 4    # SC_DISTINCT + n: the n-th largest of the distinct normals, each at least one 32-code key bucket from the next
# per dtype: sink logit m, gap of the first distinct normal, step between distinct ones, their count, gap of the crowd below the last
# one, and the bits of a 16-bit code (codes per octave, subnormal unit, smallest normal).  fp16 keeps the sink's share of the row
# above 3/4 so that the crowd stays normal; bf16 needs m >= ~93 for zero to underflow (logits there are 0.5 apart, and keys
# of that size 8: one logit step of the keys is 0.7).
_PLAN = {
    torch.float16: dict(m=30.0, d0=4.0, step=0.0625, nmax=64, crowd=0.625, codes=1024, sub=2.0 ** -24, nmin=2.0 ** -14),
    torch.bfloat16: dict(m=112.0, d0=4.0, step=1.0, nmax=64, crowd=1.0, codes=128, sub=2.0 ** -133, nmin=2.0 ** -126),
}


def _plan_logit(c: torch.Tensor, D: int) -> torch.Tensor:
    return c / np.sqrt(D)          # as the scoring does it (oracle window_logits, scale_mode "div"): one fp32 division, rounded


def _plan_keys(targets: torch.Tensor, dt, D: int) -> torch.Tensor:
    """c (model dtype dt) whose logit _plan_logit(c) lies nearest to each target logit: a fixed set of grid values."""
    uniq, inv = torch.unique(targets.double(), return_inverse=True)
    b0 = (uniq * np.sqrt(D)).to(dt).view(torch.int16).long()
    cand = (b0[:, None] + torch.arange(-3, 4)[None]).to(torch.int16).view(dt)          # neighbouring codes (positive values)
    err = (_plan_logit(cand, D).double() - uniq[:, None]).abs()
    best = cand.gather(1, err.argmin(1, keepdim=True))[:, 0]
    return best[inv]


def plan_pool(plan: torch.Tensor, kernel_size: int) -> torch.Tensor:
    """The classes after max pooling with ``kernel_size`` (1: the plan itself): a position takes the largest class of its window."""
    if kernel_size == 1:
        return plan.clone()
    rank = torch.where(plan >= SC_SINK, 1_000_000 - plan, plan).double()      # sink > distinct 0 > distinct 1 > ... > crowd > tiny > zero
    pooled = torch.nn.functional.max_pool1d(rank[None], kernel_size, 1, kernel_size // 2)[0].long()
    return torch.where(pooled >= SC_SINK, 1_000_000 - pooled, pooled)


def plan_qkv(plan: torch.Tensor, dtype, window: int = 8, D: int = 128, device="cpu"):
    """plan: int [H, L] of SC_* classes, position 0 of every head SC_SINK -> (q, k, v, plan) with q/k/v [1, H, L + window, D] in the
    model dtype.  ``window_scores(q, k, window, "mean")`` then holds the planned classes exactly (with maxpool of size ks: the
    classes ``plan_pool(plan, ks)``); ``check_plan`` states what that means."""
    dt = DTYPES[dtype] if isinstance(dtype, str) else dtype
    g = _PLAN[dt]
    plan = plan.long()
    H, L = plan.shape
    S = L + window
    if not bool((plan[:, 0] == SC_SINK).all()) or int((plan == SC_SINK).sum()) != H:
        raise ValueError("position 0 of every head, and only it, is the sink")
    if int(plan.max()) >= SC_DISTINCT + g["nmax"]:
        raise ValueError("at most %d distinct normals" % g["nmax"])
    last = g["d0"] + (g["nmax"] - 1) * g["step"]
    gap = torch.zeros(H, L, dtype=torch.float64)
    dist = plan >= SC_DISTINCT
    gap[dist] = g["d0"] + (plan[dist] - SC_DISTINCT).double() * g["step"]
    gap[plan == SC_CROWD] = last + g["crowd"]
    # the softmax normaliser of each head (float64; the tiny and zero positions add nothing that moves a class)
    Z = 1.0 + torch.where(dist | (plan == SC_CROWD), torch.exp(-gap), torch.zeros_like(gap)).sum(1)
    m0 = float(_plan_logit(_plan_keys(torch.tensor([g["m"]], dtype=torch.float64), dt, D), D))     # the sink's logit as it comes out
    tiny_gap = -torch.log(g["sub"] * Z)                                      # probability = 1 subnormal unit
    gap = torch.where(plan == SC_TINY, tiny_gap[:, None].expand(H, L), gap)
    c = _plan_keys((m0 - gap).reshape(-1), dt, D).reshape(H, L)
    c[plan == SC_ZERO] = 0
    # the margins, on the logits as they come out: every class far from a rounding boundary of its dtype
    logit = _plan_logit(c, D).double()
    m = logit[:, :1]
    Z = torch.exp(logit - m).sum(1) + window * float(np.exp(-g["m"]))
    p = torch.exp(logit - m) / Z[:, None]
    if bool((p[plan == SC_ZERO] > 0.25 * g["sub"]).any()):
        raise ValueError("zero class too close to the smallest subnormal")
    t = p[plan == SC_TINY] / g["sub"]
    if t.numel() and bool(((t - 1.0).abs() > 0.25).any()):
        raise ValueError("tiny class off its subnormal code")
    if bool((p[dist | (plan == SC_CROWD)] < 1.5 * g["nmin"]).any()):
        raise ValueError("a normal class too close to the subnormal range")
    q = torch.zeros(1, H, S, D, dtype=dt, device=device)
    q[0, :, -window:, 0] = 1.0
    hh = torch.arange(H, dtype=torch.int32, device=device).view(H, 1, 1)
    jj = torch.arange(S, dtype=torch.int32, device=device).view(1, S, 1)
    dd = torch.arange(D, dtype=torch.int32, device=device).view(1, 1, D)
    pat = ((hh * 7919 + jj * 131 + dd * 17) % 1021 - 510).to(torch.float32) / 64
    j = jj[..., 0]
    for d, part in ((1, j >> 14), (2, (j >> 7) & 127), (3, j & 127), (4, hh[..., 0].expand(H, S) & 255)):
        pat[:, :, d] = part.float()                                                       # distinct rows, exact in bf16
    v = pat.to(dt)[None]
    k = ((pat + 1.0) * 0.5).to(dt)[None]
    del pat
    k[0, :, :, 0] = 0
    k[0, :, :L, 0] = c.to(device)
    return q, k, v, plan


def check_plan(scores: torch.Tensor, plan: torch.Tensor, dtype) -> list:
    """Problems (empty list: none) of 16-bit score rows [H, L] against a class plan [H, L]: zeros exactly where planned; the tiny
    class the smallest subnormal; the crowd one normal value; the sink the row maximum; distinct normal n one value, below n - 1 and
    above the crowd by at least one 32-code key bucket."""
    dt = DTYPES[dtype] if isinstance(dtype, str) else dtype
    g = _PLAN[dt]
    s = scores.detach().cpu().to(dt)
    code = s.view(torch.int16).long() & 0xffff
    f = s.double()
    out = []
    for h in range(s.shape[0]):
        pl, fr, cr = plan[h], f[h], code[h]

        def one(mask, name):
            vals = torch.unique(cr[mask])
            if vals.numel() != 1:
                out.append("head %d: %s holds %d values" % (h, name, vals.numel()))
                return None
            return int(vals[0])

        if not torch.equal(fr == 0, pl == SC_ZERO):
            out.append("head %d: zeros at %d positions, planned %d" % (h, int((fr == 0).sum()), int((pl == SC_ZERO).sum())))
        if bool((fr < 0).any()):
            out.append("head %d: negative scores" % h)
        if bool((pl == SC_TINY).any()):
            ct = one(pl == SC_TINY, "tiny")
            if ct is not None and ct != 1:
                out.append("head %d: tiny class at code %#x" % (h, ct))
        prev = one(pl == SC_SINK, "sink")
        if prev is not None and int(cr.max()) != prev:
            out.append("head %d: the sink is not the maximum" % h)
        ladder = [SC_DISTINCT + n for n in range(g["nmax"]) if bool((pl == SC_DISTINCT + n).any())]
        if bool((pl == SC_CROWD).any()):
            ladder.append(SC_CROWD)
        for cl in ladder:
            cc = one(pl == cl, "class %d" % cl)
            if cc is None or prev is None:
                break
            if cc >= 0x8000 or cc < (0x0400 if dt == torch.float16 else 0x0080):      # smallest normal code
                out.append("head %d: class %d not a positive normal (%#x)" % (h, cl, cc))
            if prev - cc < 32:
                out.append("head %d: class %d only %d codes below the one above" % (h, cl, prev - cc))
            prev = cc
    return out
