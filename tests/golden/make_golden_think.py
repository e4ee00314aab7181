"""Generate the ThinK fixtures by running the REAL reference on CPU: SnapKVCluster.update_think (pyramidkv_utils.py:349-391)
and key_pruner_query_driven (:13-26) alone.

    python tests/golden/make_golden_think.py            # writes tests/golden/think_*.npz

The reference checkout is looked for in $PKV_REFERENCE_ROOT, else next to this repository (../reference).  It cannot travel
to the GPU box, so its outputs are committed here: every file holds the inputs (bit patterns), the reference's outputs and
the configuration.

Two kinds of file.

``think_pruner_*``: key_pruner_query_driven on given (Kc, Q), "scaled grid" inputs (tests/think_ref.py scaled_grid): every
rounded square and every column sum is exact in fp32 in any order, so a channel score has ONE value whoever computes it.

``think_e2e_*``: the whole update_think.  The first half of it is SnapKV's selection, whose `topk` leaves equal scores to the
backend, and V_c is compared bit for bit; so these inputs are grid values with a PLANTED selection: the queries are positive,
a few past keys ("hitters") carry mostly positive signs in different proportions, the rest mostly negative ones.  Every value
is still (an integer in -8..8) / 8 times the channel's power of two, so the channel energies stay exact.  A head is redrawn
until its k + 1 largest window scores are at least 4 codes of the model dtype apart from each other (fp32: 2^-16 relative):
the selection and its order then have one answer, and a last-bit difference in a softmax cannot change it.  The generator
asserts that the reference and the canonical oracle agree bit for bit on K_c and V_c, and, in every file, that at most half
of the heads have the n_prune-th and the (n_prune + 1)-th smallest channel score equal.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("PKV_REFERENCE_ROOT") or os.path.join(os.path.dirname(ROOT), "reference"))

import think_ref as T  # noqa: E402
from inputs import DTYPES, bits  # noqa: E402
from oracle import pkv_oracle as O  # noqa: E402
from pyramidkv import pyramidkv_utils as ref  # noqa: E402  (the real reference)

LIMIT = 267150          # bytes: the largest fixture this directory held before these


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):            # :355 prints on every call
        return fn(*a, **k)


def planted_head(S, D, w, k, dtype, seed):
    """One head (q, kk, v) [S, D] of the planted grid described above, redrawn until its window scores are separated."""
    dt = DTYPES[dtype]
    c = torch.arange(D)
    sk, sq = 2.0 ** -(c % 4).float(), 2.0 ** -((c // 4) % 4).float()
    L = S - w
    nh = min(k + 1, L)                                          # scores that must be apart from each other and from the rest
    for attempt in range(20000):
        g = torch.Generator().manual_seed(seed * 100003 + attempt)
        q = (torch.randint(1, 9, (S, D), generator=g).float() / 8 * sq).to(dt)
        frac = torch.full((S,), 0.5)
        frac[:L] = 0.12                                         # the crowd: far below every hitter
        hit = torch.randperm(L, generator=g)[:nh]
        frac[hit] = torch.linspace(0.45, 0.97, nh)[torch.randperm(nh, generator=g)]
        sign = torch.where(torch.rand(S, D, generator=g) < frac[:, None], 1.0, -1.0)
        kk = (sign * torch.randint(1, 9, (S, D), generator=g).float() / 8 * sk).to(dt)
        v = (torch.randint(-8, 8, (S, D), generator=g).float() / 8).to(dt)
        s = O.pool_scores(O.window_scores(q[None, None], kk[None, None], w), "avgpool", 1)[0, 0]
        top = torch.sort(s.float(), descending=True).values
        if dt == torch.float32:
            ok = bool(((top[:nh - 1] - top[1:nh]) > top[:nh - 1] * 2.0 ** -16).all())
            ok = ok and (nh == L or bool(top[nh - 1] - top[nh] > top[nh - 1] * 2.0 ** -16))
        else:
            code = torch.sort(s.view(torch.int16).int(), descending=True).values        # positive values: codes are monotone
            ok = bool(((code[:nh - 1] - code[1:nh]) >= 4).all()) and (nh == L or int(code[nh - 1] - code[nh]) >= 4)
        if ok:
            return q, kk, v, attempt
    raise RuntimeError("no separated head found")


def planted_qkv(B, H, S, D, w, k, dtype, seed):
    heads = [planted_head(S, D, w, k, dtype, seed * 64 + i) for i in range(B * H)]
    q, kk, v = (torch.stack([h[j] for h in heads]).reshape(B, H, S, D) for j in range(3))
    return q, kk, v, max(h[3] for h in heads)


E2E = []
#                 name                dtype   B  H   S   D  window cap recent ratio
for row in [("bf16_D64",   "bf16", 1, 4, 128,  64,  64,  72, 32, 0.4),
            ("bf16_D128",  "bf16", 1, 4, 160, 128,  88, 100, 32, 0.4),
            ("bf16_D256",  "bf16", 1, 2, 144, 256,  64,  72, 32, 0.3),
            ("fp16_D64",   "fp16", 1, 4, 160,  64,  88, 100, 32, 0.4),
            ("fp16_D128",  "fp16", 1, 4, 128, 128,  64,  72, 32, 0.3),
            ("fp16_D256",  "fp16", 1, 2, 150, 256,  88, 100, 32, 0.4),
            ("fp32_D64",   "fp32", 1, 4, 160,  64,  32, 160, 32, 0.4),      # S == cap is not a pass-through: all 128 past keys, in score order
            ("fp32_D128",  "fp32", 1, 2, 160, 128,  32, 160, 17, 0.3),
            ("fp32_D256",  "fp32", 1, 1, 160, 256, 128, 160, 32, 0.4),
            ("batch2_bf16", "bf16", 2, 2, 120, 128,  64,  72, 32, 0.4),     # pruned shape [1, 2H, R, D - k]
            ("s20_fp16",   "fp16", 1, 4,  20,  64,   8,  20,  5, 0.4),      # S = N = 20: fewer than 32 query rows
            ("short_bf16", "bf16", 1, 4,  50, 128,  32,  64, 32, 0.4),      # S < cap: the 2-tuple, same objects
            ("merge_fp16", "fp16", 1, 4, 120, 128,  64,  72, 32, 0.4)]:     # merge="pivot": the 2-tuple of merge_kv
    E2E.append(dict(zip(("name", "dtype", "B", "H", "S", "D", "window", "cap", "recent", "ratio"), row)))
E2E[-1]["merge"] = "pivot"

PRUNER = []
for dt in ("bf16", "fp16", "fp32"):
    for D, N in ((64, 72), (128, 100), (256, 160)):
        PRUNER.append(dict(name=f"{dt}_D{D}", dtype=dt, B=1, H=8 if D < 256 else 2, S=40, D=D, N=N, recent=32, ratio=0.4 if D != 256 else 0.3))
for p in PRUNER:
    if p["dtype"] == "fp32" and p["D"] < 256:
        p["H"] //= 2


def tie_share(score, n_prune):
    amb = T.boundary_ambiguous(score, n_prune)
    return int(amb.sum()), amb.numel()


def save(name, meta, **tensors):
    path = os.path.join(HERE, f"think_{name}.npz")
    arrays = {n: (t.numpy() if t.dtype == torch.bool else bits(t)) for n, t in tensors.items()}
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    size = os.path.getsize(path)
    print(f"{os.path.basename(path)}: {size} bytes {meta}")
    assert size <= LIMIT, "fixture larger than the largest one the directory held"


def main():
    seed = 7000
    for c in E2E:
        while True:
            seed += 1
            k_sel = c["cap"] - c["window"]
            q, k, v, tries = planted_qkv(c["B"], c["H"], c["S"], c["D"], c["window"], k_sel, c["dtype"], seed)
            cl = ref.SnapKVCluster(window_size=c["window"], max_capacity_prompt=c["cap"], kernel_size=1, pooling="avgpool",
                                   merge=c.get("merge"), recent_size=c["recent"], ratio=c["ratio"])
            out = quiet(cl.update_think, k, q, v, None, 1)
            meta = dict(c, seed=seed, kernel_size=1, pooling="avgpool", n_out=len(out), n_prune=int(c["D"] * c["ratio"]))
            if c["S"] < c["cap"]:
                assert len(out) == 2 and out[0] is k and out[1] is v
                meta["passthrough"] = True
                break
            kc, vc = O.snapkv_update_kv(k, q, v, c["window"], c["cap"], 1, "avgpool", merge=c.get("merge"))
            if c.get("merge"):
                assert len(out) == 2
                meta["oracle_bit_equal"] = bool(torch.equal(out[0], kc) and torch.equal(out[1], vc))
                break
            assert len(out) == 4
            assert torch.equal(out[3], vc), "the reference's selection is not the canonical one"
            qe, ke, score = T.scores(q, kc)
            assert torch.equal(score.double(), (T.energy_f64(q[..., -32:, :]).to(q.dtype).double() * T.energy_f64(kc).to(q.dtype).double()).to(q.dtype).double())
            amb, heads = tie_share(score, meta["n_prune"])
            if 2 * amb <= heads:
                meta["ambiguous_heads"] = amb
                break
        save("e2e_" + c["name"], meta, q=q, k=k, v=v, **{f"out{i}": t for i, t in enumerate(out)})
    for c in PRUNER:
        while True:
            seed += 1
            q, kc = T.scaled_grid(c["B"], c["H"], c["N"], c["D"], c["dtype"], seed)
            q = q[:, :, :c["S"]].contiguous()
            n_prune = int(c["D"] * c["ratio"])
            score = T.scores(q, kc)[2]
            exact = (T.energy_f64(q[..., -32:, :]).to(q.dtype).double() * T.energy_f64(kc).to(q.dtype).double()).to(q.dtype)
            assert torch.equal(score, exact), "torch's score is not the float64-exact one on a scaled grid"
            amb, heads = tie_share(score, n_prune)
            if 2 * amb <= heads:
                break
        kp, kr, keep = ref.key_pruner_query_driven(kc, q, c["recent"], c["ratio"])
        save("pruner_" + c["name"], dict(c, seed=seed, n_prune=n_prune, ambiguous_heads=amb), q=q, kc=kc, k_pruned=kp, k_recent=kr, keep=keep)


if __name__ == "__main__":
    main()
