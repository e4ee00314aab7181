"""The oracle against the REAL reference on random configurations (CPU).  The committed fixtures (tests/golden,
test_oracle_golden.py) pin fixed cases; this walks seeded random ones through the same statement: oracle/pkv_oracle.py with
the reference's own topk / sort calls == pyramidkv/pyramidkv_utils.py, bit for bit - K/V, the flat layout's metadata,
pass-through identity, the LOOK-M merge.  What the reference returned on every one of these configurations is recorded in
tests/golden/live_reference.json (bit digests of K / V, metadata, the exception it raised) and
tests/golden/live_reference_indices.npz (the indices it selected), written by tests/golden/make_live_reference.py next to a
checkout of the reference; the inputs are re-derived from their seeds and checked against the recorded checksums."""
import contextlib
import hashlib
import io
import json
import os

import numpy as np
import pytest
import torch

from inputs import make_qkv, bits, checksum                  # noqa: E402
from oracle import pkv_oracle as O                           # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def random_case(rng, policy):
    dt = ("bf16", "fp16", "fp32")[int(rng.integers(0, 3))]
    kind = ("gauss", "lattice", "planted")[int(rng.integers(0, 3))]
    w = int(rng.choice([1, 4, 8, 16, 32]))
    S = int(rng.integers(w + 1, 420))
    c = dict(policy=policy, dtype=dt, kind=kind, B=int(rng.integers(1, 3)), H=int(rng.choice([1, 2, 4, 8])), S=S, w=w,
             cap=w + int(rng.integers(1, 120)), ks=int(rng.choice([1, 3, 5, 7])), pool=("maxpool", "avgpool")[int(rng.integers(0, 2))],
             seed=int(rng.integers(1, 1 << 30)))
    if policy == "pyramidkv":
        c["layers"] = int(rng.choice([2, 8, 32]))
        c["layer"] = int(rng.integers(0, c["layers"]))
    if policy in ("snapkv", "pyramidkv", "h2o", "streamingllm") and rng.random() < 0.3:
        c["merge"] = "pivot"
    if policy in ("adakv", "headkv"):
        c["B"] = 1                                            # the flat layout is single-sequence (:738 asserts)
    if policy == "adakv":
        c["floor"] = float(rng.choice([0.0, 0.2, 0.5, 1.0]))
        c["normalize"] = bool(rng.integers(0, 2))
    if policy == "headkv":
        c["head_capacity"] = [[int(x) for x in rng.integers(1, 140, size=c["H"])]]
    return c


def run_oracle(c, q, k, v):
    w, cap, pol, mg = c["w"], c["cap"], c["policy"], c.get("merge")
    if pol == "snapkv":
        return O.snapkv_update_kv(k, q, v, w, cap, c["ks"], c["pool"], topk_mode="reference", merge=mg)
    if pol == "pyramidkv":
        return O.pyramidkv_update_kv(k, q, v, w, cap, c["ks"], c["pool"], c["layers"], c["layer"], topk_mode="reference", merge=mg)
    if pol == "h2o":
        return O.h2o_update_kv(k, q, v, w, cap, topk_mode="reference", merge=mg)
    if pol == "streamingllm":
        return O.streamingllm_update_kv(k, q, v, w, cap, merge=mg)
    if pol == "adakv":
        return O.adakv_update_kv(k, q, v, w, cap, c["ks"], c["pool"], c["floor"], c["normalize"], sort_mode="reference")
    return O.headkv_update_kv(k, q, v, w, cap, c["ks"], c["pool"], c["head_capacity"], 0, sort_mode="reference")


POLICIES = ("snapkv", "pyramidkv", "h2o", "streamingllm", "adakv", "headkv")
META_FIELDS = ("head_lens", "cu_klen", "cu_qlen", "cu_offset", "cu_head_offset")
N_CASES, N_TIE_CASES = 40, 30


def bits_digest(t):
    """shape + dtype + sha256 of the bit pattern: equal digests <=> the same shape and the same bits."""
    a = bits(t)
    return "%s:%s:%s" % ("x".join(map(str, t.shape)), str(t.dtype).replace("torch.", ""), hashlib.sha256(a.tobytes()).hexdigest())


def configurations_case(policy):
    """The seeded configurations of the equality test, in order."""
    rng = np.random.default_rng(20260925 + POLICIES.index(policy))
    return [random_case(rng, policy) for _ in range(N_CASES)]


def configurations_tie(policy):
    """The seeded configurations of the tie-rule test, in order (no merge: the selection is what is compared)."""
    rng = np.random.default_rng(777 + POLICIES.index(policy))
    out = []
    for _ in range(N_TIE_CASES):
        c = random_case(rng, policy)
        c.pop("merge", None)
        out.append(c)
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLD, "live_reference.json")) as f:
        rec = json.load(f)
    with np.load(os.path.join(GOLD, "live_reference_indices.npz")) as z:
        idx = {name: z[name] for name in z.files}
    return rec, idx


def _inputs(c, rec_case):
    q, k, v = make_qkv(c["B"], c["H"], c["S"], 128, c["dtype"], c["kind"], c["seed"])
    assert checksum(q, k, v) == rec_case["input_checksum"], ("inputs drifted from the recorded ones", c)
    return q, k, v


@pytest.mark.parametrize("policy", POLICIES)
def test_oracle_equals_the_live_reference_on_random_configurations(policy, recorded):
    rec = recorded[0]["cases"][policy]
    cases = configurations_case(policy)
    assert len(rec) == len(cases)
    ran = compressed = 0
    for c, r in zip(cases, rec):
        assert r["config"] == c, "the recorded configurations are not this test's"
        q, k, v = _inputs(c, r)
        if "raises" in r:                                     # the oracle must refuse what the reference refuses
            with pytest.raises(Exception) as ei:
                run_oracle(c, q, k, v)
            assert r["raises"] in [t.__name__ for t in type(ei.value).__mro__], (r["raises"], ei.value, c)
            continue
        out = run_oracle(c, q, k, v)
        ko, vo = out[0], out[1]
        ran += 1
        if r["passthrough"]:                                  # pass-through returns the caller's objects (:219, :315)
            assert ko is k and vo is v, c
            continue
        compressed += 1
        assert bits_digest(ko) == r["k"], c
        assert bits_digest(vo) == r["v"], c
        if policy in ("adakv", "headkv"):
            meta = out[2]
            for name in META_FIELDS:
                assert getattr(meta, name).numpy().tolist() == r["meta"][name], (name, c)
            assert meta.max_seqlen_k == r["meta"]["max_seqlen_k"] and meta.klen_sum == r["meta"]["klen_sum"], c
    assert ran >= 30 and compressed >= 20, (ran, compressed)


def _recover_indices(K, Kc_past):
    """K [B,H,L,D] source rows, Kc_past [B,H,k,D] gathered rows -> int64 [B,H,k]; None when a head holds duplicate rows."""
    B, H, L, _ = K.shape
    k = Kc_past.shape[2]
    out = np.zeros((B, H, k), dtype=np.int64)
    Kb, Cb = bits(K), bits(Kc_past)
    for b in range(B):
        for h in range(H):
            table = {Kb[b, h, s].tobytes(): s for s in range(L)}
            if len(table) != L:
                return None
            for j in range(k):
                out[b, h, j] = table[Cb[b, h, j].tobytes()]
    return torch.from_numpy(out)


@pytest.mark.parametrize("policy", ("snapkv", "pyramidkv", "h2o"))
def test_canonical_tie_rule_selects_what_the_live_reference_selected(policy, recorded):
    """What the HIP path implements is the oracle's CANONICAL tie rule (descending score, ascending index among equals); the
    reference's CPU topk orders equal scores its own way.  On random configurations the two select the same score-value
    sequence per head (O.equivalent_selection), and the same indices wherever the selected scores are distinct."""
    rec, rec_idx = recorded[0]["tie_cases"][policy], recorded[1]
    cases = configurations_tie(policy)
    assert len(rec) == len(cases)
    checked = identical_rows = 0
    for j, (c, r) in enumerate(zip(cases, rec)):
        assert r["config"] == c, "the recorded configurations are not this test's"
        q, k, v = _inputs(c, r)
        if r["passthrough"]:
            continue
        key = "%s_%02d" % (policy, j)
        if key not in rec_idx:                                # duplicate source rows: the reference's choice is not recoverable
            continue
        ref_idx = torch.from_numpy(rec_idx[key].astype(np.int64))
        if ref_idx.shape[2] == 0:
            continue
        w = c["w"]
        if policy == "snapkv":
            out = O.snapkv_update_kv(k, q, v, w, c["cap"], c["ks"], c["pool"], topk_mode="canonical", return_indices=True)
        elif policy == "pyramidkv":
            out = O.pyramidkv_update_kv(k, q, v, w, c["cap"], c["ks"], c["pool"], c["layers"], c["layer"], topk_mode="canonical",
                                        return_indices=True)
        else:
            out = O.h2o_update_kv(k, q, v, w, c["cap"], topk_mode="canonical", return_indices=True)
        idx = out[2]
        s = O.h2o_scores(q, k, w) if policy == "h2o" else O.pool_scores(O.window_scores(q, k, w, "sum"), c["pool"], c["ks"])
        assert idx.shape == ref_idx.shape, c
        assert O.equivalent_selection(idx, ref_idx, s), c
        checked += 1
        for b in range(idx.shape[0]):
            for h in range(idx.shape[1]):
                row = s[b, h].float()
                sel = row[idx[b, h]]
                if sel.unique().numel() == sel.numel() and int((row == sel[-1]).sum()) == 1:
                    assert torch.equal(idx[b, h], ref_idx[b, h]), c
                    identical_rows += 1
    assert checked >= 10 and identical_rows >= 3, (checked, identical_rows)
