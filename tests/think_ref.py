"""ThinK key-channel pruning (reference pyramidkv_utils.py:13-26, :349-391) restated for the tests: torch ops on CPU.

The contract (include/pkv.h pkv_think_prune):
  energy = every element squared and the square rounded to the model dtype -> fp32 sum over the rows -> ONE fp32 division by
           the row count -> ONE round-to-nearest-even to the model dtype (16-bit: bit for bit ``torch.pow(x, 2).mean(dim=2)``);
  score  = dtype(float(qe) * float(ke)), qe over the last min(32, S) query rows, ke over all rows of the compacted keys;
  pruned = the n_prune channels first in (score ascending, channel index ascending), NaN behind +inf by index
           (``torch.topk(largest=False)`` leaves equal scores to the backend);
  output = the kept channels, ascending, of rows 0 .. N - recent - 1 as [1, B*H, N - recent, D - n_prune]; the last
           ``recent`` rows keep all D channels; keep = the reference's ``~mask``.
``energy_bar`` states how far a device energy may sit from the exact one; ``compare_with_reference`` states what two results
must share when equal scores have no reference order."""
import json
import os

import numpy as np
import torch

from inputs import DTYPES, from_bits

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
QROWS = 32          # the reference's literal (:17); neither the window nor recent_size


# ------------------------------------------------------------------------------------------------ the restatement
def energy(x: torch.Tensor) -> torch.Tensor:
    """[..., n, D] -> [..., D] in x's dtype (the order of the fp32 sum is torch's here)."""
    sq = torch.pow(x, 2)                                                # rounded to the model dtype
    return (sq.float().sum(dim=-2) / float(x.shape[-2])).to(x.dtype)    # fp32 sum, one division, one rounding


def scores(q: torch.Tensor, kc: torch.Tensor):
    """-> (qe, ke, score), each [B,H,D] in the model dtype."""
    qe, ke = energy(q[..., -QROWS:, :]), energy(kc)
    return qe, ke, (qe.float() * ke.float()).to(kc.dtype)


def canonical_keep(score: torch.Tensor, n_prune: int):
    """score [..., D] -> (keep bool [..., D], keep_idx int64 [..., D - n_prune] ascending): the n_prune channels first in a
    stable ascending sort go (torch sorts NaN behind +inf)."""
    order = torch.argsort(score.float(), dim=-1, stable=True)
    keep = torch.ones(score.shape, dtype=torch.bool)
    keep.scatter_(-1, order[..., :n_prune], False)
    keep_idx = torch.sort(keep.to(torch.uint8), dim=-1, descending=True, stable=True).indices[..., :score.shape[-1] - n_prune]
    return keep, keep_idx


def compact(kc: torch.Tensor, keep_idx: torch.Tensor, recent: int) -> torch.Tensor:
    """kc [B,H,N,D], keep_idx [B,H,W] -> [1, B*H, N - recent, W]: bit copies."""
    B, H, N, D = kc.shape
    R, W = N - recent, keep_idx.shape[-1]
    bits = kc.view(torch.int16 if kc.element_size() == 2 else torch.int32)    # as integers: torch's 16-bit gather rewrites NaN payloads
    return bits[:, :, :R].gather(-1, keep_idx.long()[:, :, None, :].expand(B, H, R, W)).reshape(1, B * H, R, W).view(kc.dtype)


def think_prune(q, kc, recent: int, n_prune: int):
    """-> (k_pruned, k_recent, keep, keep_idx) in the reference's shapes (:26)."""
    N, D = kc.shape[-2], kc.shape[-1]
    if not (0 <= recent < N and 0 <= n_prune < D):
        raise ValueError("recent / n_prune out of range")
    keep, keep_idx = canonical_keep(scores(q, kc)[2], n_prune)
    return compact(kc, keep_idx, recent), kc[:, :, N - recent:, :], keep, keep_idx


def update_think(k, q, v, window, cap, kernel_size, pooling, recent, ratio, merge=None):
    """SnapKVCluster.update_think (:349-391) on expanded [B,H,S,D] tensors, on top of the SnapKV oracle."""
    from oracle import pkv_oracle as O
    out = O.snapkv_update_kv(k, q, v, window, cap, kernel_size, pooling, merge=merge)
    if q.shape[-2] < cap or merge is not None:                          # :357-358, :380-382: the 2-tuple
        return out
    kc, vc = out
    kp, kr, keep, _ = think_prune(q, kc, recent, int(k.shape[-1] * ratio))
    return kp, kr, keep, vc


# ------------------------------------------------------------------------------------------------ the energy bar
def energy_f64(x: torch.Tensor) -> torch.Tensor:
    """The exact mean of the ROUNDED squares (the rounding of a square is part of the contract, not an error)."""
    return torch.pow(x, 2).double().mean(dim=-2)


def _other_neighbour(r: torch.Tensor, e64: torch.Tensor) -> torch.Tensor:
    code = r.view(torch.int16).to(torch.int32)
    step = torch.where(r.double() > e64, -1, 1).to(torch.int32)
    return (code + step).clamp(0, 0x7fff).to(torch.int16).view(r.dtype)


def energy_bar(x: torch.Tensor, got: torch.Tensor, n: int, exact_grid: bool = False) -> dict:
    """Device energies ``got`` [..., D] (x's dtype) against the exact ones of the n rows ``x`` [..., n, D] (CPU tensors).

    16-bit: ``got`` equals the dtype rounding of the float64 mean of the rounded squares, except where that mean lies within
    relative n * 2^-24 of a rounding midpoint of the dtype - an fp32 sum of n non-negative terms is off by at most
    (n - 1) * 2^-24 relative in ANY order, the division adds 2^-24 - where either neighbour passes.  The exempt set is a
    function of the input alone and must stay at or below 5 % (derived share: n * 2^-12 for fp16, n * 2^-15 for bf16, hence
    n <= 160 wherever this bar is applied).  fp32: |got - exact| <= n * 2^-24 * exact.  ``exact_grid``: no exemption."""
    assert x.shape[-2] == n and n <= 160
    e64 = energy_f64(x)
    got = got.detach().cpu()
    assert got.shape == e64.shape and got.dtype == x.dtype
    if x.dtype == torch.float32:
        err = (got.double() - e64).abs()
        bound = n * 2.0 ** -24 * e64
        if exact_grid:                                       # an exact sum: the division's one rounding is all there is
            err, bound = (got - e64.float()).abs().double(), torch.zeros_like(e64)
        fig = dict(dtype="fp32", n=n, elements=e64.numel(), over_bound=int((err > bound).sum()), worst_excess=float((err - bound).max()))
        print("energy_bar", fig)
        assert fig["over_bound"] == 0, fig
        return fig
    want = e64.to(x.dtype)                                   # float64 -> 16 bit: one rounding
    same = got.view(torch.int16) == want.view(torch.int16)
    other = _other_neighbour(want, e64)
    mid = (want.double() + other.double()) / 2
    exempt = torch.isfinite(want) & (e64 > 0) & torch.isfinite(other) & ((e64 - mid).abs() <= n * 2.0 ** -24 * e64)
    if exact_grid:
        exempt = torch.zeros_like(exempt)
    ok = same | (exempt & (got.view(torch.int16) == other.view(torch.int16)))
    fig = dict(dtype=str(x.dtype), n=n, elements=e64.numel(), differ=int((~same).sum()), exempt=int(exempt.sum()),
               exempt_share=float(exempt.double().mean()), bad=int((~ok).sum()))
    print("energy_bar", fig)
    assert fig["bad"] == 0, fig
    assert fig["exempt_share"] <= 0.05, fig
    return fig


# ------------------------------------------------------------------------------------------------ comparing two results
def boundary_ambiguous(score: torch.Tensor, n_prune: int) -> torch.Tensor:
    """score [B,H,D] -> bool [B,H]: the n_prune-th and the (n_prune + 1)-th smallest score are equal (the kept set then
    depends on the order of equal scores)."""
    if n_prune == 0:
        return torch.zeros(score.shape[:-1], dtype=torch.bool)
    s = torch.sort(score.float(), dim=-1, stable=True).values
    return s[..., n_prune - 1] == s[..., n_prune]


def compare_with_reference(score, n_prune, kc, recent, got, ref) -> dict:
    """``got`` / ``ref`` = (k_pruned, keep) of two implementations on the same (kc [B,H,N,D], score [B,H,D]).
      * per head the kept set equals the reference's outside the boundary tie value (the n_prune-th smallest score);
      * inside it both keep the same number of channels;
      * heads without a boundary ambiguity: ``keep`` and ``k_pruned`` equal the reference's bit for bit;
      * either side's k_pruned is the bit copy of its own kept channels."""
    B, H, N, D = kc.shape
    R, W = N - recent, D - n_prune
    gk, gm = got[0].reshape(B, H, R, W), got[1].reshape(B, H, D)
    rk, rm = ref[0].reshape(B, H, R, W), ref[1].reshape(B, H, D)
    amb = boundary_ambiguous(score, n_prune)
    iv = torch.int16 if kc.element_size() == 2 else torch.int32          # rows are compared as integers: bit copies, NaN included
    s = score.float()
    edge = torch.sort(s, dim=-1, stable=True).values[..., max(n_prune - 1, 0)]
    for b in range(B):
        for h in range(H):
            assert int(gm[b, h].sum()) == int(rm[b, h].sum()) == W, "kept channel count"
            for m, kp in ((gm[b, h], gk[b, h]), (rm[b, h], rk[b, h])):
                assert torch.equal(kp.contiguous().view(torch.uint8), kc.view(iv)[b, h, :R][:, m].contiguous().view(torch.uint8)), "not a bit copy"
            if not bool(amb[b, h]):
                assert torch.equal(gm[b, h], rm[b, h]), f"head ({b},{h}): kept sets differ without a boundary tie"
                assert torch.equal(gk[b, h].contiguous().view(torch.uint8), rk[b, h].contiguous().view(torch.uint8))
                continue
            tie = s[b, h] == edge[b, h]
            assert torch.equal(gm[b, h][~tie], rm[b, h][~tie]), f"head ({b},{h}): kept sets differ outside the tie value"
            assert int(gm[b, h][tie].sum()) == int(rm[b, h][tie].sum())
    return dict(heads=B * H, ambiguous=int(amb.sum()))


# ------------------------------------------------------------------------------------------------ inputs and fixtures
def scaled_grid(B, H, S, D, dtype, seed):
    """-> (q, k): multiples of 1/8 in [-1, 1); channel c of k is scaled by 2^-(c % 4), channel c of q by 2^-((c // 4) % 4).
    Every rounded square and every column sum of up to 160 of them is exact in fp32 in any order, and the scores spread over
    enough binades that equal ones are rare."""
    g = torch.Generator().manual_seed(seed)
    dt = DTYPES[dtype] if isinstance(dtype, str) else dtype
    c = torch.arange(D)
    k = torch.randint(-8, 8, (B, H, S, D), generator=g).float() / 8 * (2.0 ** -(c % 4).float())
    q = torch.randint(-8, 8, (B, H, S, D), generator=g).float() / 8 * (2.0 ** -((c // 4) % 4).float())
    return q.to(dt), k.to(dt)


def fixture_files():
    return sorted(f for f in os.listdir(GOLD) if f.startswith("think_") and f.endswith(".npz"))


def load_fixture(name):
    """-> (meta, tensors) of tests/golden/think_*.npz (written by tests/golden/make_golden_think.py): the inputs q, k, v, the
    reference's outputs of SnapKVCluster.update_think (out0 .. out3, or out0, out1 for the 2-tuple) and, in the pruner-only
    files, kc with the three outputs of key_pruner_query_driven."""
    z = np.load(os.path.join(GOLD, name))
    meta = json.loads(str(z["meta"]))
    t = {}
    for n in z.files:
        if n == "meta":
            continue
        t[n] = torch.from_numpy(z[n].copy()) if z[n].dtype == np.bool_ else from_bits(z[n], meta["dtype"])
    return meta, t
