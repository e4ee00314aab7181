"""Single-query attention over the ThinK cache (pruned keys next to full-width keys): the float64 restatement, the masks, the
exact fixtures and the error bar that tests/test_think_decode_cpu.py, tests/test_gpu_think_decode.py and
tools/think_decode_bench.py share.  The fp32 orders, `ulp`, `out_bar` and `lse_bar` are those of tests/decode_attn_ref.py.
Nothing here launches a kernel or imports the package.

Layout, one layer of a ThinKCache without its batch dimension: q [H, D]; keep bool [H, D]; k_pruned [H, R, Dk] - the kept
channels of R keys, ascending; k_full [H, T, D]; v [H, R + T, D]."""
import math

import numpy as np
import torch

from decode_attn_ref import DTYPES, _merge_f32, _online_f32, _v_rows, chunk_rows, lse_bar, out_bar, ulp  # noqa: F401


def kept_widths(D):
    """Dk of the GPU test: one channel, the reference's ratio 0.4 (39 / 77 / 154), all but one, all (an unpruned layer)."""
    return [1, D - int(0.4 * D), D - 1, D]


def masks(H, D, Dk, seed=0):
    """bool [H, D] with exactly Dk ones per head, a different mask per head: head 0 drops channel 0 (where anything is dropped),
    head 1 keeps only the last Dk channels, the others are drawn."""
    g = torch.Generator().manual_seed(1000 * D + 7 * Dk + seed)
    keep = torch.zeros(H, D, dtype=torch.bool)
    for h in range(H):
        if h == 1:
            idx = torch.arange(D - Dk, D)
        elif h == 0 and Dk < D:
            idx = 1 + torch.randperm(D - 1, generator=g)[:Dk]
        else:
            idx = torch.randperm(D, generator=g)[:Dk]
        keep[h, idx] = True
    assert bool((keep.sum(1) == Dk).all())
    return keep


def keep_index(keep):
    """int64 [H, Dk], ascending - what ThinKCache derives from its mask."""
    Dk = int(keep[0].sum())
    return torch.sort(keep.to(torch.uint8), dim=-1, descending=True, stable=True).indices[..., :Dk]


def prune(k, keep):
    """[H, R, D] -> [H, R, Dk]: the kept channels of every row."""
    idx = keep_index(keep)
    return k.gather(-1, idx[:, None, :].expand(-1, k.shape[1], -1)).contiguous()


def widen(k_pruned, keep):
    """The inverse with zeros in the dropped channels: [H, R, Dk] -> [H, R, D]."""
    H, R, _ = k_pruned.shape
    idx = keep_index(keep)
    return torch.zeros(H, R, keep.shape[1], dtype=k_pruned.dtype).scatter_(-1, idx[:, None, :].expand(-1, R, -1), k_pruned)


def ref_f64(q, keep, k_pruned, k_full, v, scale):
    """float64, one head at a time: gather q through the mask, score the pruned rows then the full rows, softmax, weighted V.
    -> (out [H, D] float64, lse [H] float64); no rows: zeros, -inf."""
    H, D = q.shape
    out, lse = torch.zeros(H, D, dtype=torch.float64), torch.full((H,), -math.inf, dtype=torch.float64)
    if k_pruned.shape[1] + k_full.shape[1] == 0:
        return out, lse
    for h in range(H):
        qp = q[h].double()[keep[h]]
        s = torch.cat([k_pruned[h].double() @ qp, k_full[h].double() @ q[h].double()]) * float(scale)
        m = s.max()
        e = torch.exp(s - m)
        out[h] = (e[:, None] * v[h].double()).sum(0) / e.sum()
        lse[h] = m + torch.log(e.sum())
    return out, lse


def gauss(H, R, T, D, Dk, dtype, seed):
    """N(0, 1) inputs rounded to dtype.  -> q, keep, k_pruned, k_full, v."""
    g = torch.Generator().manual_seed(seed)
    keep = masks(H, D, Dk, seed)
    return (torch.randn(H, D, generator=g).to(dtype), keep, torch.randn(H, R, Dk, generator=g).to(dtype),
            torch.randn(H, T, D, generator=g).to(dtype), torch.randn(H, R + T, D, generator=g).to(dtype))


def eager_fp32_deviation(eager, q, keep, k_pruned, k_full, v, scale, ref, ref_lse):
    """E per head: the largest deviation from `ref` of `eager` (think_decode_attention) run on the inputs upcast to fp32, on the
    tensors' device - fp32 accumulation, no final rounding; and the same for lse, which the eager function does not return:
    torch.logsumexp over fp32 scores (an fp32 matrix-vector product per part and head, times `scale`), the form of
    decode_attn_ref.eager_fp32_lse_deviation.  -> (E [H], E_lse [H]) float64."""
    idx = keep_index(keep.cpu()).to(q.device)
    qf, kpf, kff = q.float(), k_pruned.float(), k_full.float()
    got = eager(qf[None, :, None, :], idx[None], kpf[None], kff[None], v.float()[None], scale)[0, 0].double().cpu()
    E_lse = torch.zeros(q.shape[0], dtype=torch.float64)
    for h in range(q.shape[0]):                                            # head by head, as decode_attn_ref.eager_fp32_lse_deviation
        s = torch.cat([kpf[h] @ qf[h][idx[h]], kff[h] @ qf[h]]) * scale
        E_lse[h] = abs(float(torch.logsumexp(s, 0).double().cpu()) - float(ref_lse[h]))
    return (got - ref).abs().amax(dim=1), E_lse


# ---- the exact fixtures: every fp32 evaluation order gives the same bits ------------------------------------------------------
def shapes(C):
    """(R, T) of the GPU test: no pruned rows, one of each, a misaligned head base (R * Dk * e no multiple of 16), both sides of
    a chunk boundary in either part, several chunks."""
    return [(0, 1), (1, 1), (3, 2), (C - 1, 1), (C, C + 1), (C + 1, 2), (3 * C + 5, C)]


def plant_rows(R, T, C):
    """Score rows to plant: rows 0, C-1, C, C+1 and R-1 of the pruned part, row R (the first full-width row), the last row
    (the appended token) - those that exist, each once."""
    rows = [r for r in (0, C - 1, C, C + 1, R - 1) if 0 <= r < R] + [R, R + T - 1]
    return list(dict.fromkeys(rows))


def onehot_fixture(H, R, T, D, keep, dtype, row):
    """All keys zero except score row `row` of every head, which holds 64 at the head's LAST kept channel c - at stored column
    Dk - 1 of a pruned row (different from c wherever a channel below c was dropped), at channel c of a full-width row; q = 64 e_c.
    With scale = D ** -0.5 the planted score is 4096 / sqrt(D) >= 256 above every other one: every other exp is exactly 0 in
    fp32, the planted weight exactly 1.  -> q, k_pruned, k_full, v, want_out (the planted V rows), want_lse (float32)."""
    Dk = int(keep[0].sum())
    last = keep_index(keep)[:, -1]
    q = torch.zeros(H, D, dtype=dtype)
    kp, kf = torch.zeros(H, R, Dk, dtype=dtype), torch.zeros(H, T, D, dtype=dtype)
    v = _v_rows([R + T] * H, D).to(dtype).view(H, R + T, D)
    for h in range(H):
        q[h, last[h]] = 64.0
        if row < R:
            kp[h, row, Dk - 1] = 64.0
        else:
            kf[h, row - R, last[h]] = 64.0
    lse = torch.full((H,), float(np.float32(4096.0) * np.float32(float(D) ** -0.5)), dtype=torch.float32)
    return q, kp, kf, v, v[:, row].clone(), lse


def uniform_fixture(H, R, T, D, Dk, dtype):
    """q = 0: every weight is exactly 1 / n.  n = R + T a power of two and V small integers: out is the exact mean, lse = log(n).
    -> q, keep, k_pruned, k_full, v, want_out, want_lse (float64)."""
    n = R + T
    assert n > 0 and n & (n - 1) == 0
    g = torch.Generator().manual_seed(7)
    keep = masks(H, D, Dk)
    kp, kf = torch.randn(H, R, Dk, generator=g).to(dtype), torch.randn(H, T, D, generator=g).to(dtype)
    h, j, d = torch.arange(H)[:, None, None], torch.arange(n)[None, :, None], torch.arange(D)[None, None, :]
    v64 = ((j * 5 + d * 3 + h) % 16 - 8).double()
    want = v64.sum(1) / n
    assert torch.equal(want.float().double(), want), "the mean is an fp32 number"
    return torch.zeros(H, D, dtype=dtype), keep, kp, kf, v64.to(dtype), want.to(dtype), torch.full((H,), math.log(n), dtype=torch.float64)


# ---- fp32 evaluation on the CPU in three orders (numpy float32, one rounding per operation) ------------------------------------
def attend_f32(q, keep, k_pruned, k_full, v, scale, order, chunk=None, splits=1):
    """fp32 online softmax per head on the CPU over the score rows of both parts laid end to end (a pruned row = a full-width row
    with zeros in the dropped channels).  order: "forward", "reversed", or "chunked": ceil(R / chunk) chunks of pruned rows, then
    ceil(T / chunk) chunks of full-width rows - none straddles the two parts - dealt to `splits` partials round-robin, each
    evaluated on its own, then merged.  -> (out [H, D] float32 before the rounding to the model dtype, lse [H] float32)."""
    H, D = q.shape
    R, T = k_pruned.shape[1], k_full.shape[1]
    k_all = torch.cat([widen(k_pruned, keep), k_full], dim=1)
    qn, kn, vn = (t.float().numpy() for t in (q, k_all, v))
    out, lse = np.zeros((H, D), dtype=np.float32), np.full(H, -np.inf, dtype=np.float32)
    if R + T == 0:
        return torch.from_numpy(out), torch.from_numpy(lse)
    chunks = []
    if order == "chunked":
        chunks = [list(range(a, min(R, a + chunk))) for a in range(0, R, chunk)] + [list(range(R + a, R + min(T, a + chunk))) for a in range(0, T, chunk)]
    for h in range(H):
        if order == "forward":
            m, l, acc = _online_f32(qn[h], kn[h], vn[h], scale, range(R + T))
        elif order == "reversed":
            m, l, acc = _online_f32(qn[h], kn[h], vn[h], scale, range(R + T - 1, -1, -1))
        else:
            parts = [_online_f32(qn[h], kn[h], vn[h], scale, [j for c in chunks[sp::splits] for j in c]) for sp in range(min(splits, len(chunks)))]
            m, l, acc = _merge_f32(parts)
        out[h] = acc / l
        lse[h] = np.float32(np.float64(m) + np.log(np.float64(l)))
    return torch.from_numpy(out), torch.from_numpy(lse)
