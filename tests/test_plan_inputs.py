"""CPU: the score-class plans of tests/inputs.py (plan_qkv) hold through the oracle's scoring - every planned class, tie group and
zero count comes out exactly, in fp16 and bf16, un-pooled and max-pooled - so the GPU route tests can put a row on a chosen route
of the top-k kernel through q and k alone."""
import pytest
import torch

from inputs import SC_CROWD, SC_DISTINCT, SC_SINK, SC_TINY, SC_ZERO, check_plan, plan_pool, plan_qkv
from oracle import pkv_oracle as O


def _plan(H, L, n_distinct, n_crowd, n_tiny, seed, spacing=8):
    """Sink at 0; the other classes on positions at least `spacing` apart (one per 8-key chunk at 8), the rest zero."""
    g = torch.Generator().manual_seed(seed)
    plan = torch.full((H, L), SC_ZERO, dtype=torch.long)
    plan[:, 0] = SC_SINK
    n = n_distinct + n_crowd + n_tiny
    for h in range(H):
        slots = torch.randperm(L // spacing - 1, generator=g)[:n] + 1
        pos = slots * spacing + torch.randint(0, spacing - 6, (n,), generator=g)
        plan[h, pos[:n_distinct]] = SC_DISTINCT + torch.arange(n_distinct)
        plan[h, pos[n_distinct:n_distinct + n_crowd]] = SC_CROWD
        plan[h, pos[n_distinct + n_crowd:]] = SC_TINY
    return plan


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("ks", [1, 7])
def test_planned_classes_come_out_of_the_oracle_exactly(dt, ks):
    w = 8
    cases = [(2, 8000, 63, 200, 150, 8), (3, 2400, 63, 1, 0, 16), (1, 12000, 10, 400, 300, 8), (2, 1200, 0, 0, 0, 8)]
    for ci, (H, L, nd, nc, nt, sp) in enumerate(cases):
        plan = _plan(H, L, nd, nc, nt, 40 + ci, sp if ks == 1 else 16)
        q, k, v, pl = plan_qkv(plan, dt, window=w)
        assert torch.equal(pl, plan) and q.shape == k.shape == v.shape == (1, H, L + w, 128)
        s = O.pool_scores(O.window_scores(q, k, w, "mean"), "maxpool" if ks > 1 else None, ks)[0]
        want = plan_pool(plan, ks)
        assert check_plan(s, want, dt) == [], (ci, check_plan(s, want, dt)[:4])
        for h in range(H):                      # the counts a route test relies on, stated directly
            pos = s[h] > 0
            assert int((s[h] == 0).sum()) == int((want[h] == SC_ZERO).sum())
            assert int(pos.sum()) == int((want[h] != SC_ZERO).sum())
            if nc:
                crowd = s[h][want[h] == SC_CROWD]
                assert int((s[h] == crowd[0]).sum()) == int((want[h] == SC_CROWD).sum()) == (nc if ks == 1 else 7 * nc)
            if nt:
                assert int((s[h][pos] < torch.finfo(s.dtype).tiny).sum()) == int((want[h] == SC_TINY).sum())
        # the v / k rows the gather copies are all distinct (a wrong index cannot pass unnoticed)
        assert torch.unique(v[0, 0].float(), dim=0).shape[0] == L + w
        assert torch.unique(k[0, 0, :, 1:].float(), dim=0).shape[0] == L + w


def test_plan_rejects_what_it_cannot_pin():
    plan = torch.zeros(1, 100, dtype=torch.long)
    with pytest.raises(ValueError):
        plan_qkv(plan, "fp16")                              # no sink
    plan[0, 0] = SC_SINK
    plan[0, 5] = SC_DISTINCT + 64
    with pytest.raises(ValueError):
        plan_qkv(plan, "bf16")                              # more distinct normals than the grid holds
    plan[0, 5] = SC_DISTINCT
    s = O.window_scores(*plan_qkv(plan, "fp16")[:2], 8, "mean")[0].clone()
    assert check_plan(s, plan, "fp16") == []
    s[0, 7] = 1e-3                                         # one zero that is not: found
    assert check_plan(s, plan, "fp16")
