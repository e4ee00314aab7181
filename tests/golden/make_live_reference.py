"""Record what the REAL reference returns on the seeded random configurations of tests/test_oracle_live_reference.py.

    PKV_REFERENCE_ROOT=<checkout of PyramidKV> python tests/golden/make_live_reference.py
        -> tests/golden/live_reference.json, tests/golden/live_reference_indices.npz

Per configuration: the checksum of the inputs (re-derived from the seed by tests/inputs.py), then what the reference's
update_kv did with them - the exception type it raised, pass-through (it returned the caller's tensors), or the bit digest
of K and V it returned plus, for Ada-SnapKV / HeadKV, the flat layout's metadata.  For the tie-rule test: the indices the
reference selected, recovered by matching its gathered K rows to the source rows (absent where a head holds duplicate rows).
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("PKV_REFERENCE_ROOT")
if not REF or not os.path.exists(os.path.join(REF, "pyramidkv", "pyramidkv_utils.py")):
    raise SystemExit("set PKV_REFERENCE_ROOT to a checkout of the reference (pyramidkv/pyramidkv_utils.py)")
sys.path.insert(0, REF)

from inputs import make_qkv, checksum  # noqa: E402
from pyramidkv import pyramidkv_utils as ref  # noqa: E402  (the real reference)
import test_oracle_live_reference as T  # noqa: E402


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def run_reference(c, q, k, v):
    w, cap, pol, mg = c["w"], c["cap"], c["policy"], c.get("merge")
    if pol == "snapkv":
        cl = ref.SnapKVCluster(window_size=w, max_capacity_prompt=cap, kernel_size=c["ks"], pooling=c["pool"], merge=mg)
    elif pol == "pyramidkv":
        cl = ref.PyramidKVCluster(num_hidden_layers=c["layers"], layer_idx=c["layer"], window_size=w, max_capacity_prompt=cap,
                                  kernel_size=c["ks"], pooling=c["pool"], merge=mg)
    elif pol == "h2o":
        cl = ref.H2OKVCluster(window_size=w, max_capacity_prompt=cap, merge=mg)
    elif pol == "streamingllm":
        cl = ref.StreamingLLMKVCluster(window_size=w, max_capacity_prompt=cap, merge=mg)
    elif pol == "adakv":
        cl = ref.AdaKVCluster(window_size=w, kernel_size=c["ks"], pooling=c["pool"], max_capacity_prompt=cap, floor=c["floor"],
                              normalize=c["normalize"], layer_idx=0, num_hidden_layers=32)
    else:
        cl = ref.HeadKVCluster(window_size=w, kernel_size=c["ks"], pooling=c["pool"], max_capacity_prompt=cap, layer_idx=0,
                               num_hidden_layers=32, head_capacity=c["head_capacity"])
    if pol in ("adakv", "headkv"):
        kc, vc = quiet(cl.update_kv, k, q, v)
        return kc, vc, cl
    kc, vc = quiet(cl.update_kv, k, q, v, None, 1)
    return kc, vc, cl


def inputs(c):
    q, k, v = make_qkv(c["B"], c["H"], c["S"], 128, c["dtype"], c["kind"], c["seed"])
    return q, k, v, {"config": c, "input_checksum": checksum(q, k, v)}


def main():
    cases, tie_cases, indices = {}, {}, {}
    for policy in T.POLICIES:
        rows = []
        for c in T.configurations_case(policy):
            q, k, v, r = inputs(c)
            try:
                kr, vr, cl = run_reference(c, q, k, v)
            except Exception as e:                                # noqa: BLE001 - recorded: the oracle must refuse it too
                r["raises"] = type(e).__name__
                rows.append(r)
                continue
            r["passthrough"] = kr is k
            if not r["passthrough"]:
                r["k"], r["v"] = T.bits_digest(kr), T.bits_digest(vr)
                if policy in ("adakv", "headkv"):
                    r["meta"] = {name: getattr(cl, name).numpy().tolist() for name in T.META_FIELDS}
                    r["meta"].update(max_seqlen_k=int(cl.max_seqlen_k), klen_sum=int(cl.klen_sum))
            rows.append(r)
        cases[policy] = rows
    for policy in ("snapkv", "pyramidkv", "h2o"):
        rows = []
        for j, c in enumerate(T.configurations_tie(policy)):
            q, k, v, r = inputs(c)
            kr, _, _ = run_reference(c, q, k, v)
            r["passthrough"] = kr is k
            if not r["passthrough"]:
                w = c["w"]
                ri = T._recover_indices(k[:, :, :-w], kr[:, :, :kr.shape[2] - w])
                if ri is not None:
                    indices["%s_%02d" % (policy, j)] = ri.numpy().astype(np.int16)
            rows.append(r)
        tie_cases[policy] = rows
    with open(os.path.join(HERE, "live_reference.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_live_reference.py", "cases": cases, "tie_cases": tie_cases}, f, indent=0)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "live_reference_indices.npz"), **indices)


if __name__ == "__main__":
    main()
