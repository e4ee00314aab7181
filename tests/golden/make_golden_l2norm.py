"""Generate the L2Norm fixtures by running the REAL reference's L2NormCluster (pyramidkv_utils.py:394-429) on CPU.

    python tests/golden/make_golden_l2norm.py            # writes tests/golden/l2norm_*.npz

The reference checkout is looked for in $PKV_REFERENCE_ROOT, else next to this repository (../reference).  It cannot travel
to the GPU box, so its outputs are committed here: every file holds the inputs K, V (bit patterns), the reference's K_out,
V_out and the configuration.  Inputs are multiples of 1/8 in [-1, 1] (squares sum exactly in fp32 in any order, so the norm
of a row has ONE value whoever computes it); equal norms are the normal case there, and the reference's `argsort` leaves
their order to the backend - tests compare what does not depend on it (tests/l2norm_ref.py compare_outputs).  One case is
tie-free (integer-valued fp32 rows with pairwise distinct sums of squares per head): there the index sequence itself is pinned.
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

from inputs import DTYPES, bits  # noqa: E402
from l2norm_ref import grid_kv  # noqa: E402
from pyramidkv import pyramidkv_utils as ref  # noqa: E402  (the real reference)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):            # :411 prints on every call
        return fn(*a, **k)


def tie_free_kv(B, H, S, D, seed):
    """Integer-valued fp32 rows whose sums of squares are pairwise distinct inside every head (seed retried otherwise)."""
    while True:
        g = torch.Generator().manual_seed(seed)
        k = torch.randint(-8, 9, (B, H, S, D), generator=g).float()
        v = torch.randint(-8, 9, (B, H, S, D), generator=g).float()
        ss = k.double().pow(2).sum(-1)
        if all(ss[b, h].unique().numel() == S for b in range(B) for h in range(H)):
            return k, v, seed
        seed += 1


CASES = []
for dt in ("bf16", "fp16", "fp32"):
    for D in (64, 128, 256):
        CASES.append(dict(name=f"grid_{dt}_D{D}", dtype=dt, B=2, H=2, S=96, D=D, cap=40, layer_idx=2, skip_layers=[0, 1], seed=500 + D))
CASES.append(dict(name="full_permutation_bf16", dtype="bf16", B=2, H=2, S=80, D=128, cap=80, layer_idx=3, skip_layers=[0, 1], seed=601))
CASES.append(dict(name="skip_layer_fp16", dtype="fp16", B=2, H=2, S=96, D=128, cap=40, layer_idx=1, skip_layers=[0, 1], seed=602))
CASES.append(dict(name="short_prompt_bf16", dtype="bf16", B=2, H=2, S=50, D=128, cap=64, layer_idx=5, skip_layers=[0, 1], seed=603))
CASES.append(dict(name="short_prompt_skip_layer_bf16", dtype="bf16", B=2, H=2, S=50, D=64, cap=64, layer_idx=0, skip_layers=[0, 1], seed=604))
CASES.append(dict(name="tie_free_fp32", dtype="fp32", B=2, H=2, S=40, D=64, cap=16, layer_idx=2, skip_layers=[0, 1], seed=605, tie_free=True))


def main():
    for c in CASES:
        if c.get("tie_free"):
            k, v, c["seed"] = tie_free_kv(c["B"], c["H"], c["S"], c["D"], c["seed"])
        else:
            k, v = grid_kv(c["B"], c["H"], c["S"], c["D"], c["dtype"], c["seed"])
        assert k.dtype == DTYPES[c["dtype"]]
        q = torch.zeros_like(k)                                   # the policy reads the query's shape only (:409)
        cl = ref.L2NormCluster(max_capacity_prompt=c["cap"], layer_idx=c["layer_idx"], skip_layers=list(c["skip_layers"]))
        ko, vo = quiet(cl.update_kv, k, q, v, None, 1)
        meta = dict(c, passthrough=bool(ko is k and vo is v))
        path = os.path.join(HERE, f"l2norm_{c['name']}.npz")
        np.savez_compressed(path, meta=np.array(json.dumps(meta)), k=bits(k), v=bits(v), k_out=bits(ko), v_out=bits(vo))
        print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, out {tuple(ko.shape)}, passthrough={meta['passthrough']}")


if __name__ == "__main__":
    main()
