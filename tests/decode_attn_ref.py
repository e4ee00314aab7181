"""Single-query attention over the flat var-len cache: the float64 restatement, the exact fixtures and the error bar that
tests/test_decode_attn_cpu.py, tests/test_gpu_decode_attn.py and tools/decode_attn_bench.py share.  Nothing here launches a
kernel or imports the package."""
import math
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
# significand bits behind the leading one, smallest normal exponent
_FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}


def chunk_rows() -> int:
    """PKV_DECODE_CHUNK as include/pkv.h states it."""
    hdr = open(os.path.join(ROOT, "include", "pkv.h")).read()
    return int(re.search(r"#define PKV_DECODE_CHUNK (\d+)", hdr).group(1))


def cu_of(lens) -> torch.Tensor:
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)


def ref_f64(q, k_flat, v_flat, cu_klen, scale):
    """float64, one head at a time.  -> (out [H, D] float64, lse [H] float64); a head without rows: zeros, -inf."""
    H, D = q.shape
    out, lse = torch.zeros(H, D, dtype=torch.float64), torch.full((H,), -math.inf, dtype=torch.float64)
    cu = [int(x) for x in cu_klen]
    for h in range(H):
        a, b = cu[h], cu[h + 1]
        if b <= a:
            continue
        s = (k_flat[a:b].double() @ q[h].double()) * float(scale)
        m = s.max()
        e = torch.exp(s - m)
        out[h] = (e[:, None] * v_flat[a:b].double()).sum(0) / e.sum()
        lse[h] = m + torch.log(e.sum())
    return out, lse


def ulp(dtype, x: torch.Tensor) -> torch.Tensor:
    """Spacing of `dtype` at |x| (float64 in and out); the subnormal spacing below the smallest normal."""
    bits, emin = _FMT[dtype]
    ex = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), ex - bits)


def eager_fp32_deviation(eager, q, k_flat, v_flat, cu_klen, max_seqlen_k, scale, ref):
    """E per head: the largest deviation from `ref` of `eager` (varlen_decode_attention) run on the inputs upcast to fp32 -
    fp32 accumulation, no final rounding.  -> [H] float64."""
    got = eager(q.float(), k_flat.float(), v_flat.float(), cu_klen, max_seqlen_k, scale).double()
    return (got - ref).abs().amax(dim=1)


def eager_fp32_lse_deviation(q, k_flat, cu_klen, scale, ref_lse):
    """The same for lse, which the eager function does not return: torch.logsumexp over its fp32 scores (the inputs upcast to
    fp32, an fp32 matrix-vector product times `scale`), head by head, on the tensors' device.  -> [H] float64."""
    cu = [int(x) for x in cu_klen]
    E = torch.zeros(len(cu) - 1, dtype=torch.float64)
    for h in range(len(cu) - 1):
        if cu[h + 1] > cu[h]:
            s = (k_flat[cu[h]:cu[h + 1]].float() @ q[h].float()) * scale
            E[h] = abs(float(torch.logsumexp(s, 0).double().cpu()) - float(ref_lse[h]))
    return E


def lse_bar(ref_lse, E_lse):
    """lse is an fp32 number: its one rounding, given twice its half-ulp, + 4 E of the head."""
    return ulp(torch.float32, ref_lse) + 4.0 * E_lse


def out_bar(dtype, ref, E):
    """Per element: the one rounding to the model dtype, given twice its half-ulp, + 4 E of the head (a different fp32
    summation order and nothing else)."""
    return ulp(dtype, ref) + 4.0 * E[:, None]


# ---- the exact fixtures: every fp32 evaluation order gives the same bits ------------------------------------------------------
def _v_rows(lens, D):
    """V rows that spell (head, row) in small integers (exact in bf16): element 0 = head + 1, 1 = row % 128, 2 = row // 128,
    the rest a pattern of both in [-32, 32)."""
    rows = []
    for h, n in enumerate(lens):
        j = torch.arange(n)[:, None]
        d = torch.arange(D)[None, :]
        v = ((j * 7 + d * 3 + h * 11) % 64 - 32).double()
        v[:, 0], v[:, 1], v[:, 2] = h + 1, (j[:, 0] % 128).double(), (j[:, 0] // 128).double()
        rows.append(v)
    return torch.cat(rows) if rows else torch.zeros(0, D, dtype=torch.float64)


def onehot_fixture(lens, D, dtype, plant):
    """All keys zero except row plant[h] of head h, whose element 0 is 64; q = 64 e_0.  With scale = D ** -0.5 the planted score
    is 4096 / sqrt(D) >= 256 above every other one: every other exp is exactly 0 in fp32, the planted weight exactly 1.
    -> q, k_flat, v_flat, cu_klen, want_out (the planted V rows), want_lse (the planted score, float32)."""
    H, total = len(lens), int(sum(lens))
    cu = cu_of(lens)
    q = torch.zeros(H, D, dtype=dtype)
    q[:, 0] = 64.0
    k = torch.zeros(total, D, dtype=dtype)
    v = _v_rows(lens, D).to(dtype)
    want = torch.zeros(H, D, dtype=dtype)
    for h, n in enumerate(lens):
        assert 0 <= plant[h] < n
        k[int(cu[h]) + plant[h], 0] = 64.0
        want[h] = v[int(cu[h]) + plant[h]]
    lse = torch.full((H,), float(np.float32(4096.0) * np.float32(float(D) ** -0.5)), dtype=torch.float32)
    return q, k, v, cu, want, lse


def plants(lens, C):
    """Row 0, C-1, C, C+1 and n-1 (the appended token's row) of each head, where the head has them."""
    out = []
    for r in (0, C - 1, C, C + 1, None):
        out.append([min(n - 1, r) if r is not None else n - 1 for n in lens])
    return [list(p) for p in dict.fromkeys(tuple(p) for p in out)]


def uniform_fixture(lens, D, dtype):
    """q = 0: every weight is exactly 1 / n.  n a power of two and V small integers: out is the exact mean, lse = log(n).
    -> q, k_flat, v_flat, cu_klen, want_out, want_lse (float64)."""
    H, total = len(lens), int(sum(lens))
    assert all(n & (n - 1) == 0 and n > 0 for n in lens)
    cu = cu_of(lens)
    q = torch.zeros(H, D, dtype=dtype)
    g = torch.Generator().manual_seed(7)
    k = torch.randn(total, D, generator=g).to(dtype)
    vs = []
    for h, n in enumerate(lens):
        j, d = torch.arange(n)[:, None], torch.arange(D)[None, :]
        vs.append(((j * 5 + d * 3 + h) % 16 - 8).double())
    v64 = torch.cat(vs)
    want = torch.stack([v64[int(cu[h]):int(cu[h + 1])].sum(0) / n for h, n in enumerate(lens)])
    assert torch.equal(want.float().double(), want), "the mean is an fp32 number"
    return q, k, v64.to(dtype), cu, want.to(dtype), torch.tensor([math.log(n) for n in lens], dtype=torch.float64)


# ---- fp32 evaluation on the CPU in three orders (numpy float32, one rounding per operation) ------------------------------------
def _online_f32(q, k, v, scale, rows):
    f = np.float32
    m, l, acc = f(-np.inf), f(0), np.zeros(v.shape[1], dtype=f)
    for j in rows:
        s = f(np.dot(q, k[j]).astype(f) * f(scale))
        mn = max(m, s)
        sc = f(0) if m == -np.inf else np.exp(f(m - mn), dtype=f)
        p = np.exp(f(s - mn), dtype=f)
        l = f(l * sc + p)
        acc = (acc * sc + p * v[j]).astype(f)
        m = mn
    return m, l, acc


def _merge_f32(parts):
    f = np.float32
    M = max(p[0] for p in parts)
    L, A = f(0), np.zeros_like(parts[0][2])
    for m, l, acc in parts:
        w = f(0) if m == -np.inf else np.exp(f(m - M), dtype=f)
        L = f(L + l * w)
        A = (A + acc * w).astype(f)
    return M, L, A


def attend_f32(q, k_flat, v_flat, cu_klen, scale, order, chunk=None, splits=1):
    """fp32 online softmax per head on the CPU.  order: "forward", "reversed", or "chunked" (chunks of `chunk` rows dealt
    to `splits` partials round-robin, each evaluated on its own, then merged).  -> (out [H, D] float32 before the rounding
    to the model dtype, lse [H] float32)."""
    H, D = q.shape
    qn, kn, vn = (t.float().numpy() for t in (q, k_flat, v_flat))
    out, lse = np.zeros((H, D), dtype=np.float32), np.full(H, -np.inf, dtype=np.float32)
    cu = [int(x) for x in cu_klen]
    for h in range(H):
        a, n = cu[h], cu[h + 1] - cu[h]
        if n <= 0:
            continue
        kh, vh = kn[a:a + n], vn[a:a + n]
        if order == "forward":
            m, l, acc = _online_f32(qn[h], kh, vh, scale, range(n))
        elif order == "reversed":
            m, l, acc = _online_f32(qn[h], kh, vh, scale, range(n - 1, -1, -1))
        else:
            nck = (n + chunk - 1) // chunk
            parts = []
            for sp in range(min(splits, nck)):
                rows = [j for c in range(sp, nck, splits) for j in range(c * chunk, min(n, (c + 1) * chunk))]
                parts.append(_online_f32(qn[h], kh, vh, scale, rows))
            m, l, acc = _merge_f32(parts)
        out[h] = acc / l
        lse[h] = np.float32(np.float64(m) + np.log(np.float64(l)))
    return torch.from_numpy(out), torch.from_numpy(lse)
