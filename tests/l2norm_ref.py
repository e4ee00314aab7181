"""L2Norm (reference pyramidkv_utils.py:394-429) restated for the tests: torch ops on CPU, no float64 in the policy itself.

The contract:
  norm   = fp32 sum of squares -> correctly rounded fp32 sqrt -> ONE round-to-nearest-even to the model dtype;
  order  = norm ascending, index ascending (the reference's ``argsort`` without ``stable=True`` leaves equal norms to the backend);
  output = the first ``cap`` rows of that order, K and V, no window rows appended.
``norm_f64`` / ``norm_bar`` state how far a device norm may sit from the exact one; ``compare_outputs`` states what two
results of the policy must share when ties have no reference order."""
import os

import numpy as np
import torch

from inputs import DTYPES, from_bits

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def norms_model(k: torch.Tensor) -> torch.Tensor:
    """[..., S, D] -> [..., S] in k's dtype: the target arithmetic (the order of the fp32 sum is torch's here; on inputs whose
    squares sum exactly in fp32 every order gives the same bits).  torch.norm and not ``.pow(2).sum(-1).sqrt()``: the
    element-wise fp32 ``sqrt`` of the CPU backend is a vectorised routine that is not correctly rounded (6 of 1000 random
    inputs differ from the float64 root), the reduction's final root is."""
    return torch.norm(k.float(), p=2, dim=-1).to(k.dtype)


def canonical_order(norms: torch.Tensor) -> torch.Tensor:
    """Stable ascending argsort: norm ascending, index ascending; +inf last by index, NaN behind it."""
    return torch.argsort(norms.float(), dim=-1, stable=True)


def l2norm_update_kv(k, q, v, cap, layer_idx=0, skip_layers=(), return_indices=False):
    """The canonical restatement of L2NormCluster.update_kv on expanded [B,H,S,D] tensors."""
    assert k.shape[-2] == q.shape[-2]                                   # :408
    if q.shape[-2] < cap or layer_idx in skip_layers:                   # :413, :415 (in this order)
        return (k, v, None) if return_indices else (k, v)
    idx = canonical_order(norms_model(k))[..., :cap]                    # :419-420
    ix = idx[..., None].expand(-1, -1, -1, k.shape[-1])
    ko, vo = k.gather(2, ix), v.gather(2, ix)                           # :423-427
    return (ko, vo, idx) if return_indices else (ko, vo)


# ------------------------------------------------------------------------------------------------ the norm bar
def norm_f64(k: torch.Tensor) -> torch.Tensor:
    return k.double().pow(2).sum(-1).sqrt()


def round_dtype(n64: torch.Tensor, dtype) -> torch.Tensor:
    """float64 -> fp32 (of an exact sum of squares: the correctly rounded fp32 sqrt) -> the model dtype, both nearest-even."""
    return n64.float().to(dtype)


def _other_neighbour(r: torch.Tensor, n64: torch.Tensor) -> torch.Tensor:
    """16-bit r = the dtype value nearest to n64 (> 0, finite) -> the dtype value on the OTHER side of n64."""
    code = r.view(torch.int16).to(torch.int32)
    step = torch.where(r.double() > n64, -1, 1).to(torch.int32)
    return (code + step).clamp(0, 0x7fff).to(torch.int16).view(r.dtype)


def norm_bar(k: torch.Tensor, got: torch.Tensor, exact_grid: bool = False) -> dict:
    """Device norms ``got`` [..., S] (k's dtype) against the exact norms of ``k`` [..., S, D] (CPU tensors).

    16-bit: ``got == round_dtype(norm_f64)`` exactly, except where the exact norm lies within relative D * 2^-25 of a
    rounding midpoint of the dtype - an fp32 sum of D squares is off by at most (D - 1) * 2^-24 relative in ANY order, the
    square root halves that - where either neighbour passes.  The exempt set is a function of the input alone and must stay
    below 5 % of the elements (derived share: D * 2^-13 for fp16, D * 2^-16 for bf16).  ``exact_grid``: no exemption.
    fp32: |got - n64| <= D * 2^-24 * n64.
    Returns the figures; raises AssertionError with them when the bar is missed."""
    D = k.shape[-1]
    n64 = norm_f64(k)
    got = got.detach().cpu()
    assert got.shape == n64.shape and got.dtype == k.dtype
    if k.dtype == torch.float32:
        err = (got.double() - n64).abs()
        bound = D * 2.0 ** -24 * n64
        if exact_grid:
            bound = torch.zeros_like(bound)
            err = (got - round_dtype(n64, torch.float32)).abs().double()
        worst = float((err - bound).max())
        fig = dict(dtype="fp32", D=D, elements=n64.numel(), over_bound=int((err > bound).sum()), worst_excess=worst)
        print("norm_bar", fig)
        assert fig["over_bound"] == 0, fig
        return fig
    want = round_dtype(n64, k.dtype)
    same = got.view(torch.int16) == want.view(torch.int16)
    finite = torch.isfinite(want) & (n64 > 0)
    other = _other_neighbour(want, n64)
    mid = (want.double() + other.double()) / 2
    exempt = finite & torch.isfinite(other) & ((n64 - mid).abs() <= D * 2.0 ** -25 * n64)
    if exact_grid:
        exempt = torch.zeros_like(exempt)
    ok = same | (exempt & (got.view(torch.int16) == other.view(torch.int16)))
    fig = dict(dtype=str(k.dtype), D=D, elements=n64.numel(), differ=int((~same).sum()), exempt=int(exempt.sum()),
               exempt_share=float(exempt.double().mean()), bad=int((~ok).sum()))
    print("norm_bar", fig)
    assert fig["bad"] == 0, fig
    assert fig["exempt_share"] <= 0.05, fig
    return fig


# ------------------------------------------------------------------------------------------------ comparing two results
def recover_indices(k, v, ko, vo) -> torch.Tensor:
    """Every (K_out[i], V_out[i]) must be ONE source row pair (K[s], V[s]); -> int64 [B,H,n] of the s found (the lowest)."""
    B, H, S, D = k.shape
    n = ko.shape[2]
    kb, vb, kob, vob = (t.contiguous().view(torch.uint8).reshape(t.shape[0], t.shape[1], t.shape[2], -1).numpy() for t in (k, v, ko, vo))
    out = torch.zeros(B, H, n, dtype=torch.int64)
    for b in range(B):
        for h in range(H):
            table = {}
            for s in range(S):
                table.setdefault(kb[b, h, s].tobytes() + vb[b, h, s].tobytes(), s)
            for i in range(n):
                key = kob[b, h, i].tobytes() + vob[b, h, i].tobytes()
                assert key in table, f"output row ({b},{h},{i}) is not a source row pair"
                out[b, h, i] = table[key]
    return out


def compare_outputs(k, v, got, ref, cap, canonical_got=True, norms=None):
    """``got`` / ``ref`` = (K_out, V_out) of two implementations of the policy on (k, v) (CPU tensors, [B,H,S,D]).
      * the norm VALUES of the output rows form the same sequence (unique whatever the tie order);
      * outside the boundary tie value (the norm of the last kept row) both kept the same set;
      * every output row pair is one source row pair, no source row twice;
      * ``canonical_got``: inside every tie value ``got`` holds ascending indices, and of the boundary value the lowest ones.
    ``norms`` [B,H,S]: the norms the order was built on (default: norms_model(k))."""
    nk = norms_model(k) if norms is None else norms
    assert got[0].shape == ref[0].shape == (k.shape[0], k.shape[1], cap, k.shape[3])
    gi, ri = recover_indices(k, v, *got), recover_indices(k, v, *ref)
    gn, rn = nk.gather(2, gi).float(), nk.gather(2, ri).float()
    assert torch.equal(gn, rn), "norm sequences of the output rows differ"
    assert bool((gn[..., 1:] >= gn[..., :-1]).all()), "output rows are not in ascending-norm order"
    for b in range(k.shape[0]):
        for h in range(k.shape[1]):
            a, r, row = gi[b, h], ri[b, h], nk[b, h].float()
            assert a.unique().numel() == cap and r.unique().numel() == cap, "a source row was kept twice"
            edge = gn[b, h, -1]
            assert set(a[gn[b, h] < edge].tolist()) == set(r[rn[b, h] < edge].tolist()), "kept sets differ below the boundary value"
            if canonical_got:
                want = canonical_order(row)[:cap]
                assert torch.equal(a, want), "not the (norm ascending, index ascending) order"
    return gi, ri


# ------------------------------------------------------------------------------------------------ fixtures
def grid_kv(B, H, S, D, dtype, seed, scale=8):
    """Multiples of 1/8 in [-1, 1]: squares are multiples of 1/64 <= 1 and D <= 256 of them sum exactly in fp32 in any order."""
    g = torch.Generator().manual_seed(seed)
    dt = DTYPES[dtype] if isinstance(dtype, str) else dtype
    k = (torch.randint(-scale, scale + 1, (B, H, S, D), generator=g).float() / scale).to(dt)
    v = (torch.randint(-scale, scale + 1, (B, H, S, D), generator=g).float() / scale).to(dt)
    return k, v


def fixture_files():
    return sorted(f for f in os.listdir(GOLD) if f.startswith("l2norm_") and f.endswith(".npz"))


def load_fixture(name):
    """-> (meta dict, k, v, k_out, v_out) of tests/golden/l2norm_*.npz (written by tests/golden/make_golden_l2norm.py)."""
    import json
    z = np.load(os.path.join(GOLD, name))
    meta = json.loads(str(z["meta"]))
    ts = [from_bits(z[n], meta["dtype"]) for n in ("k", "v", "k_out", "v_out")]
    return (meta, *ts)
