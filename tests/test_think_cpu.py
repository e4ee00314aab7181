"""ThinK on CPU: the restatement (tests/think_ref.py) against the reference's recorded results (tests/golden/think_*.npz) and,
where a checkout of the reference is at hand, against the live reference; the tie rule; the host side of
SnapKVCluster.update_think, init_think_native and ThinKCache; the "think" forward of replace_llama / replace_mistral on a tiny
model; the argument checks of pkv_think_prune.  No kernel is launched here."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import think_ref as T
from inputs import DTYPES
from oracle import pkv_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LARGEST_BEFORE = 267150          # bytes of the largest fixture tests/golden held before the think_* files


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pyramidkv_amd", "libpkv.so")):
        g.build()
    import pyramidkv_amd
    return pyramidkv_amd


# ------------------------------------------------------------------------------------------------ fixtures
def test_fixture_set_is_complete():
    names = T.fixture_files()
    for dt in ("bf16", "fp16", "fp32"):
        for D in (64, 128, 256):
            assert f"think_e2e_{dt}_D{D}.npz" in names and f"think_pruner_{dt}_D{D}.npz" in names
    for n in ("batch2_bf16", "s20_fp16", "short_bf16", "merge_fp16"):
        assert f"think_e2e_{n}.npz" in names
    caps = set()
    for n in names:
        assert os.path.getsize(os.path.join(T.GOLD, n)) <= LARGEST_BEFORE
        meta, _ = T.load_fixture(n)
        assert meta["H"] <= 8 and meta["S"] <= 160
        caps.add(meta.get("cap", meta.get("N")))
    assert {72, 100, 160} <= caps


def _exact_score(q, kc):
    """The score from float64-exact energies: on the fixtures' grids torch's own is this one."""
    qe = T.energy_f64(q[..., -T.QROWS:, :]).to(q.dtype)
    ke = T.energy_f64(kc).to(q.dtype)
    return (qe.double() * ke.double()).to(q.dtype)


@pytest.mark.parametrize("name", [n for n in T.fixture_files() if "_pruner_" in n])
def test_restatement_reproduces_the_recorded_pruner(name):
    meta, t = T.load_fixture(name)
    q, kc = t["q"], t["kc"]
    assert kc.shape == (meta["B"], meta["H"], meta["N"], meta["D"]) and kc.dtype == DTYPES[meta["dtype"]]
    qe, ke, score = T.scores(q, kc)
    assert torch.equal(score, _exact_score(q, kc)), "scaled grid: the score has one value whoever computes it"
    kp, kr, keep, keep_idx = T.think_prune(q, kc, meta["recent"], meta["n_prune"])
    assert kp.shape == t["k_pruned"].shape == (1, meta["B"] * meta["H"], meta["N"] - meta["recent"], meta["D"] - meta["n_prune"])
    assert torch.equal(kr, t["k_recent"]) and keep.shape == t["keep"].shape
    fig = T.compare_with_reference(score, meta["n_prune"], kc, meta["recent"], (kp, keep), (t["k_pruned"], t["keep"]))
    assert 2 * fig["ambiguous"] <= fig["heads"] and fig["ambiguous"] == meta["ambiguous_heads"]
    assert bool((keep_idx[..., 1:] > keep_idx[..., :-1]).all())


@pytest.mark.parametrize("name", [n for n in T.fixture_files() if "_e2e_" in n])
def test_restatement_reproduces_the_recorded_update_think(name):
    meta, t = T.load_fixture(name)
    q, k, v = t["q"], t["k"], t["v"]
    out = T.update_think(k, q, v, meta["window"], meta["cap"], meta["kernel_size"], meta["pooling"], meta["recent"], meta["ratio"],
                         merge=meta.get("merge"))
    assert len(out) == meta["n_out"]
    if meta.get("passthrough"):
        assert out[0] is k and out[1] is v and torch.equal(t["out0"], k) and torch.equal(t["out1"], v)
        return
    if meta.get("merge"):
        assert out[0].shape == t["out0"].shape == (meta["B"], meta["H"], meta["cap"], meta["D"])
        assert torch.equal(out[0], t["out0"]) and torch.equal(out[1], t["out1"])
        return
    kp, kr, keep, vc = out
    assert torch.equal(vc, t["out3"]), "V_c: the planted selection has one answer"
    assert torch.equal(kr, t["out1"])
    kc = O.snapkv_update_kv(k, q, v, meta["window"], meta["cap"], meta["kernel_size"], meta["pooling"])[0]
    score = T.scores(q, kc)[2]
    assert torch.equal(score, _exact_score(q, kc))
    fig = T.compare_with_reference(score, meta["n_prune"], kc, meta["recent"], (kp, keep), (t["out0"], t["out2"]))
    assert 2 * fig["ambiguous"] <= fig["heads"]
    B, H = meta["B"], meta["H"]
    assert kp.shape == (1, B * H, meta["cap"] - meta["recent"], meta["D"] - meta["n_prune"])


# ------------------------------------------------------------------------------------------------ the live reference
def _reference():
    root = os.environ.get("PKV_REFERENCE_ROOT") or os.path.join(os.path.dirname(ROOT), "reference")
    if not os.path.exists(os.path.join(root, "pyramidkv", "pyramidkv_utils.py")):
        pytest.skip("no checkout of the reference next to this repository (PKV_REFERENCE_ROOT)")
    sys.path.insert(0, root)
    try:                                                    # a reference that is present but does not import FAILS the test
        from pyramidkv import pyramidkv_utils as ref
    finally:
        sys.path.remove(root)
    return ref


def test_restatement_against_the_live_reference_on_gaussian_inputs():
    """The CPU sum order is the same on both sides, so the scores are bit-equal and only equal scores can differ."""
    ref = _reference()
    rng = np.random.default_rng(20241018)
    for _ in range(18):
        dt = DTYPES[("bf16", "fp16", "fp32")[int(rng.integers(0, 3))]]
        D = int(rng.choice([64, 128, 256]))
        B, H, N, S = int(rng.integers(1, 3)), int(rng.choice([1, 2, 4])), int(rng.integers(2, 200)), int(rng.integers(1, 120))
        recent, ratio = int(rng.integers(0, N)), float(rng.choice([0.0, 0.1, 0.3, 0.4, 0.9]))
        g = torch.Generator().manual_seed(int(rng.integers(1, 1 << 30)))
        kc, q = torch.randn(B, H, N, D, generator=g).to(dt), torch.randn(B, H, S, D, generator=g).to(dt)
        n_prune = int(D * ratio)
        if recent == 0:
            continue                                        # the reference's `[:, :, N - 0:]` slice is empty; ours is too, nothing to compare
        rp, rr, rk = ref.key_pruner_query_driven(kc, q, recent, ratio)
        ref_score = torch.pow(q[..., -32:, :], 2).mean(dim=2) * torch.pow(kc, 2).mean(dim=2)          # :17-19
        qe, ke, score = T.scores(q, kc)
        assert torch.equal(score.view(torch.uint8), ref_score.view(torch.uint8))
        kp, kr, keep, _ = T.think_prune(q, kc, recent, n_prune)
        assert torch.equal(kr, rr)
        T.compare_with_reference(score, n_prune, kc, recent, (kp, keep), (rp, rk))


# ------------------------------------------------------------------------------------------------ the tie rule
def test_tie_rule_on_planted_scores():
    inf, nan = float("inf"), float("nan")
    s = torch.tensor([[3.0, 0.0, 1.0, 0.0, 1.0, 0.0, 2.0, 0.0]])
    keep, idx = T.canonical_keep(s, 2)
    assert keep.tolist() == [[True, False, True, False, True, True, True, True]]            # of four tied zeros the first two go
    assert idx.tolist() == [[0, 2, 4, 5, 6, 7]]
    keep, _ = T.canonical_keep(s, 5)
    assert keep.tolist() == [[True, False, False, False, True, False, True, False]]         # four zeros, then the first 1.0
    keep, _ = T.canonical_keep(torch.full((1, 6), 0.5), 4)
    assert keep.tolist() == [[False] * 4 + [True] * 2]                                      # all equal: prune 0 .. k-1
    s = torch.tensor([[nan, 1.0, inf, nan, inf, 0.5]])
    assert T.canonical_keep(s, 2)[0].tolist() == [[True, False, True, True, True, False]]
    assert T.canonical_keep(s, 3)[0].tolist() == [[True, False, False, True, True, False]]   # +inf by index ...
    assert T.canonical_keep(s, 5)[0].tolist() == [[False, False, False, True, False, False]]  # ... NaN behind it, by index
    assert T.canonical_keep(s, 0)[0].all() and T.canonical_keep(s, 0)[1].tolist() == [list(range(6))]
    assert T.boundary_ambiguous(torch.tensor([[[0.0, 1.0, 1.0, 2.0]]]), 2).tolist() == [[True]]
    assert T.boundary_ambiguous(torch.tensor([[[0.0, 1.0, 1.0, 2.0]]]), 1).tolist() == [[False]]


def test_energy_bar_accepts_the_restatement_and_rejects_a_wrong_rounding():
    g = torch.Generator().manual_seed(5)
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        x = torch.randn(2, 3, 72, 64, generator=g).to(dt)
        T.energy_bar(x, T.energy(x), 72)
        wrong = T.energy(x).clone()
        if dt == torch.float32:
            wrong[0, 0, 0] *= 1.001
        else:
            wrong.view(torch.int16)[0, 0, :8] += 2            # two codes off: beyond either neighbour
        with pytest.raises(AssertionError):
            T.energy_bar(x, wrong, 72)


# ------------------------------------------------------------------------------------------------ host side of the cluster
class _RefOps:
    """Restatement-backed stand-in for pyramidkv_amd.ops (the product ops need a GPU): what SnapKVCluster reaches."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def prepare_compress(*a, **kw):
        return None

    def compress(self, q, k, v, window, topk_k, pooling, kernel_size, scale_mode="div", kv_group=1, h2o=False, return_indices=False,
                 idx_out=None):
        self.calls.append("compress")
        k, v = (t.repeat_interleave(kv_group, dim=1) for t in (k, v))
        return O.snapkv_update_kv(k, q, v, window, topk_k + window, kernel_size, pooling)

    def select(self, q, k, window, topk_k, pooling, kernel_size, scale_mode="div", kv_group=1, h2o=False):
        k = k.repeat_interleave(kv_group, dim=1)
        return O.topk_canonical(O.pool_scores(O.window_scores(q, k, window), pooling, kernel_size), topk_k).to(torch.int32)

    def merge_compact(self, k, v, idx, window, kv_group=1):
        self.calls.append("merge")
        k, v = (t.repeat_interleave(kv_group, dim=1) for t in (k, v))
        return O.merge_kv(k, v, idx.long(), window, "pivot")

    def think_prune(self, q, kc, recent, n_prune, **kw):
        self.calls.append(("think_prune", recent, n_prune))
        kp, _, keep, _ = T.think_prune(q, kc, recent, n_prune)
        return kp, keep


@pytest.fixture
def ref_ops(P, monkeypatch):
    ops = _RefOps()
    monkeypatch.setattr(P.pyramidkv_utils, "ops", ops)
    return ops


def test_update_think_tuple_forms_and_errors(P, ref_ops):
    meta, t = T.load_fixture("think_e2e_bf16_D64.npz")
    q, k, v = t["q"], t["k"], t["v"]
    kw = dict(window_size=meta["window"], max_capacity_prompt=meta["cap"], kernel_size=1, pooling="avgpool")
    cl = P.SnapKVCluster(recent_size=meta["recent"], ratio=meta["ratio"], **kw)
    out = cl.update_think(k, q, v, None, 1)
    assert len(out) == 4 and ref_ops.calls == ["compress", ("think_prune", 32, 25)]
    kp, kr, keep, vc = out
    want = T.update_think(k, q, v, meta["window"], meta["cap"], 1, "avgpool", meta["recent"], meta["ratio"])
    for a, b in zip(out, want):
        assert torch.equal(a, b)
    assert kr.shape == (1, 4, 32, 64) and kr._base is not None, "k_recent is a view of K_c"
    assert torch.equal(vc, t["out3"]) and keep.dtype == torch.bool
    # un-expanded K/V go in exactly where update_kv takes them
    out_g = cl.update_think(k[:, ::2], q, v[:, ::2], None, 2)
    assert len(out_g) == 4 and out_g[0].shape == kp.shape
    # a short prompt: what update_kv returns, the input objects
    short = P.SnapKVCluster(recent_size=32, ratio=0.4, window_size=32, max_capacity_prompt=4096)
    o2 = short.update_think(k, q, v, None, 1)
    assert len(o2) == 2 and o2[0] is k and o2[1] is v
    # merge set: the merge result, a 2-tuple (reference :380-382)
    ref_ops.calls.clear()
    mg = P.SnapKVCluster(merge="pivot", recent_size=32, ratio=0.4, **kw)
    o3 = mg.update_think(k, q, v, None, 1)
    assert len(o3) == 2 and ref_ops.calls == ["merge"] and o3[0].shape == (1, 4, meta["cap"], 64)
    # out-of-range settings raise before anything is launched
    ref_ops.calls.clear()
    for bad in (dict(recent_size=meta["cap"]), dict(recent_size=meta["cap"] + 5), dict(recent_size=-1), dict(ratio=1.0), dict(ratio=1.5),
                dict(ratio=-0.1)):
        with pytest.raises(ValueError):
            P.SnapKVCluster(**{**dict(recent_size=32, ratio=0.4), **bad, **kw}).update_think(k, q, v, None, 1)
    assert ref_ops.calls == []
    # ... but not on the paths that never prune (the reference does not look at them there either)
    assert len(P.SnapKVCluster(recent_size=10 ** 6, ratio=7.0, window_size=32, max_capacity_prompt=4096).update_think(k, q, v, None, 1)) == 2
    assert len(P.SnapKVCluster(recent_size=meta["cap"] - 1, ratio=0.0, **kw).update_think(k, q, v, None, 1)) == 4
    with pytest.raises(AssertionError):                     # :352
        cl.update_think(k, q[:, :, :-1], v, None, 1)
    cl.reset()                                              # reset stays as it is: recent_size and ratio survive it
    assert (cl.recent_size, cl.ratio, cl.max_capacity_prompt) == (32, 0.4, 320)


def test_think_prune_needs_a_gpu(P):
    q = torch.zeros(1, 2, 40, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        P.ops.think_prune(q, q, 8, 25)


def test_factory_defaults_and_the_pinned_placeholder(P):
    U = P.pyramidkv_utils
    with pytest.raises(NotImplementedError):
        U.init_think(object())
    mod = types.SimpleNamespace(config=types.SimpleNamespace(), layer_idx=3)
    U.init_think_native(mod)
    cl = mod.kv_cluster
    assert isinstance(cl, P.SnapKVCluster)
    assert (cl.window_size, cl.max_capacity_prompt, cl.kernel_size, cl.pooling, cl.merge, cl.recent_size, cl.ratio) == \
        (32, 4096, 5, "avgpool", None, 32, 0.4)                                             # reference :926-952
    mod.config.ratio, mod.config.recent_size = 0.3, 16
    U.init_think_native(mod)                                # rebuilt on every call, reading the config again
    assert mod.kv_cluster is not cl and (mod.kv_cluster.ratio, mod.kv_cluster.recent_size) == (0.3, 16)
    from pyramidkv_amd import monkeypatch as mp
    assert mp._THINK_METHODS == {"think": "init_think_native"} and "think" not in mp._METHODS
    assert mp._METHODS == {"pyramidkv": ("init_pyramidkv", True), "snapkv": ("init_snapkv", False), "h2o": ("init_H2O", False),
                           "streamingllm": ("init_StreamingLLM", False), "l2norm": ("init_l2norm_native", False)}
    assert P.init_think_native is U.init_think_native and P.ThinKCache is U.ThinKCache


# ------------------------------------------------------------------------------------------------ ThinKCache
def test_thinkcache_bookkeeping(P):
    c = P.ThinKCache()
    assert len(c) == 0 and c.get_seq_length() == 0 and c.get_seq_length(3) == 0 and c.get_mask_sizes(7, 0) == (7, 0)
    H, R, rec, D, W = 2, 5, 3, 8, 6
    keep = torch.tensor([[[1, 1, 0, 1, 1, 0, 1, 1], [0, 1, 1, 1, 0, 1, 1, 1]]], dtype=torch.bool)
    kp, kr, v = torch.randn(1, H, R, W), torch.randn(1, H, rec, D), torch.randn(1, H, R + rec, D)
    with pytest.raises(IndexError):
        c.update_think(kp, kr, keep, v, 1)
    c.update_think(kp, kr, keep, v, 0)
    c.update_think(kp * 2, kr, keep, v, 0)                  # once per layer (cache_utils_think.py:419)
    assert len(c) == 1 and torch.equal(c.key_cache_pruned[0], kp) and c.mask[0] is keep
    assert c.keep_idx[0].tolist() == [[[0, 1, 3, 4, 6, 7], [1, 2, 3, 5, 6, 7]]]
    assert c.get_seq_length(0) == R + rec and c.get_seq_length(1) == 0                       # :431
    k1, v1 = torch.randn(1, H, 1, D), torch.randn(1, H, 1, D)
    ko, vo = c.update(k1, v1, 0)
    assert ko.shape == (1, H, rec + 1, D) and vo.shape == (1, H, R + rec + 1, D) and torch.equal(ko[:, :, -1:], k1)
    assert c.get_seq_length(0) == R + rec + 1 and torch.equal(c.key_cache_pruned[0], kp)
    c._seen_tokens = 40
    assert c.get_query_offset(0) == 40 and c.get_mask_sizes(1, 0) == (41, 0) and c.get_query_offset(1) == 0
    # the reference's layout [1, B*H, R, W] is taken as it comes
    c.update_think(kp.reshape(1, H, R, W), kr, keep, v, 1)
    assert c.key_cache_pruned[1].shape == (1, H, R, W)


# ------------------------------------------------------------------------------------------------ replace_llama / replace_mistral
class _RefThinkCluster:
    accepts_unexpanded_kv = True

    def __init__(self, cfg):
        self.cfg = cfg

    def update_think(self, k, q, v, mask, groups):
        g = q.shape[1] // k.shape[1]
        k, v = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)
        c = self.cfg
        return T.update_think(k, q, v, c.window_size, c.max_capacity_prompt, c.kernel_size, c.pooling, c.recent_size, c.ratio,
                              merge=getattr(c, "merge", None))


@pytest.fixture
def patched():
    pytest.importorskip("transformers")
    from pyramidkv_amd import monkeypatch as mp
    saved = mp._cluster_module
    m = types.SimpleNamespace()
    m.init_think_native = lambda self: setattr(self, "kv_cluster", _RefThinkCluster(self.config))
    mp._cluster_module = m
    yield mp
    mp._cluster_module = saved
    mp.restore()


def _tiny(family, layers=2):
    torch.manual_seed(0)
    kw = dict(vocab_size=97, hidden_size=256, intermediate_size=512, num_hidden_layers=layers, num_attention_heads=4,
              num_key_value_heads=2, head_dim=64, max_position_embeddings=4096)
    if family == "llama":
        from transformers import LlamaConfig, LlamaForCausalLM
        return LlamaForCausalLM(LlamaConfig(**kw)).eval()
    from transformers import MistralConfig, MistralForCausalLM
    return MistralForCausalLM(MistralConfig(sliding_window=None, **kw)).eval()


@pytest.mark.parametrize("family,cap", [("llama", 48), ("mistral", 48), ("llama", 4096)])
def test_think_forward_decode_equals_full_width_keys_with_pruned_channels_zeroed(P, patched, family, cap):
    """Prefill: the prompt attends to the full K/V.  Decode: the logits are those of a plain cache whose first R keys carry
    zeros in the pruned channels (dropping a channel from q and k = a zero in k).  cap 4096: a short prompt, an unpruned layer."""
    from transformers import DynamicCache
    model = _tiny(family)
    S, recent, window = 90, 8, 16
    ids = torch.randint(0, 97, (1, S), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        base = model(ids).logits
    replace = patched.replace_llama if family == "llama" else patched.replace_mistral
    replace("think")
    for layer in model.model.layers:
        c = layer.self_attn.config
        c.window_size, c.max_capacity_prompt, c.kernel_size, c.pooling, c.recent_size, c.ratio = window, cap, 5, "avgpool", recent, 0.4
    with pytest.raises(TypeError):
        model(ids, past_key_values=DynamicCache(config=model.config), use_cache=True)
    cache = P.ThinKCache()
    with torch.no_grad():
        out = model(ids, past_key_values=cache, use_cache=True)
    assert torch.allclose(out.logits, base, atol=1e-4, rtol=1e-4)
    H, D = 4, 64
    n = min(cap, S)
    pruned = cap <= S
    W = D - int(D * 0.4) if pruned else D
    for l in range(2):
        assert cache.key_cache_pruned[l].shape == (1, H, n - recent if pruned else 0, W)
        assert cache.key_cache[l].shape == (1, H, recent if pruned else S, D) and cache.value_cache[l].shape == (1, H, n, D)
        assert int(cache.mask[l].sum()) == H * W
    assert cache.get_seq_length() == S and cache._seen_tokens == S        # the instance reports the tokens seen (positions)
    # the twin: a plain cache with full-width keys, zeros in the pruned channels of the first R rows
    twin = DynamicCache(config=model.config)
    for l in range(2):
        kp, idx = cache.key_cache_pruned[l], cache.keep_idx[l]
        full = torch.zeros(1, H, kp.shape[2], D).scatter_(-1, idx[:, :, None, :].expand(-1, -1, kp.shape[2], -1), kp)
        twin.update(torch.cat([full, cache.key_cache[l]], dim=2), cache.value_cache[l], l)
        patched._track_tokens(twin, l, S, True)
    nxt = out.logits[:, -1:].argmax(-1)
    steps = []
    with torch.no_grad():
        for _ in range(3):
            o = model(nxt, past_key_values=cache, use_cache=True)
            steps.append((nxt, o.logits))
            nxt = o.logits[:, -1:].argmax(-1)
    assert cache.key_cache[0].shape[2] == (recent if pruned else S) + 3 and cache._seen_tokens == S + 3
    replace("snapkv")                                       # its decode step: append, attend over the cache
    with torch.no_grad():
        for tok, want in steps:
            o = model(tok, past_key_values=twin, use_cache=True)
            assert torch.allclose(o.logits, want, atol=1e-4, rtol=1e-4)
    patched.restore()
    with torch.no_grad():
        assert torch.equal(model(ids).logits, base)


# ------------------------------------------------------------------------------------------------ ABI (no launch)
def _desc(N, dtype=0, B=1, H=4, S=256, D=128, g=1):
    d = N.PkvDesc()
    d.dtype, d.B, d.H, d.S, d.D, d.kv_group = dtype, B, H, S, D, g
    for i, st in enumerate((H * S * D, S * D, D)):
        d.q_stride[i] = st
    return d


def test_think_abi_declared_exported_and_checked_before_any_launch(P):
    N = P._native
    hdr = open(os.path.join(ROOT, "include", "pkv.h")).read()
    for name in ("pkv_think_workspace_bytes", "pkv_think_prune"):
        assert re.search(r"PKV_API \w+ " + name + r"\(", hdr) and name in N.EXPORTED and hasattr(N.lib, name)
    assert N.lib.pkv_version() == N.PKV_VERSION == 204 and int(re.search(r"#define PKV_VERSION (\d+)", hdr).group(1)) == 204
    assert "PKV_K_COUNT = 9" in hdr and len(N.KERNEL_NAMES) == 9
    assert ctypes.sizeof(N.PkvDesc) == 136                                  # the descriptor did not grow
    good = _desc(N)
    call = lambda d, q=16, kc=16, n=100, rec=32, k=51, out=16, keep=16, idx=None, st=None, ws=16, nb=1 << 30: \
        N.lib.pkv_think_prune(d, q, kc, n, rec, k, out, keep, idx, st, ws, nb, None)   # noqa: E731
    # the workspace: one fp32 row of D per started chunk of THINK_SCAN_ROWS key rows, one for the queries, one index row
    nb = N.lib.pkv_think_workspace_bytes(good, 100)
    assert nb > 0 and nb % 256 == 0
    R0 = N.THINK_SCAN_ROWS
    sizes = [N.lib.pkv_think_workspace_bytes(good, n) for n in (1, R0, R0 + 1, 2 * R0, 2 * R0 + 1, 4096)]
    assert sizes[0] == sizes[1] < sizes[2] == sizes[3] < sizes[4] < sizes[5]
    assert sizes[2] - sizes[1] == 4 * 128 * 4                                # B*H rows of D floats more
    assert N.lib.pkv_think_workspace_bytes(good, 0) == 0
    assert call(good, nb=nb - 1) == -4                                      # PKV_ERR_WORKSPACE
    for bad in (dict(n=0), dict(rec=-1), dict(rec=100), dict(rec=101), dict(k=-1), dict(k=128), dict(k=200)):
        assert call(good, **bad) == -2, bad                                 # PKV_ERR_SHAPE
    assert call(good, rec=99, k=127, nb=0) == -4 and call(good, rec=0, k=0, nb=0) == -4     # in range: only the workspace is left to object
    assert call(_desc(N, D=96)) == -2 and call(_desc(N, dtype=3)) == -1 and call(_desc(N, H=6, g=4)) == -2 and call(_desc(N, S=0)) == -2
    assert call(_desc(N, dtype=2), nb=0) == -4                              # fp32 is taken
    odd = _desc(N)
    odd.q_stride[2] = 132
    assert call(odd) == -3                                                  # q rows off 16 bytes
    assert call(good, q=None) == -7 and call(good, kc=None) == -7 and call(good, out=None) == -7 and call(good, keep=None) == -7
    assert call(good, ws=None) == -7
    assert call(good, q=8) == -3 and call(good, kc=24) == -3 and call(good, out=2) == -3 and call(good, st=8) == -3 and call(good, ws=4) == -3
    assert call(good, idx=6) == -3 and call(good, idx=4, nb=0) == -4 and call(good, keep=3, nb=0) == -4
    short = _desc(N)
    short.struct_size = 132
    assert call(short) == -9 and N.lib.pkv_think_workspace_bytes(short, 100) == 0
    # the descriptor's window / topk / pooling fields and k, v strides are not this entry point's business
    loose = _desc(N)
    loose.window, loose.topk, loose.pool_kind, loose.pool_kernel = 0, 0, 7, 4
    assert N.lib.pkv_think_workspace_bytes(loose, 100) == nb
    # ... and every other entry point keeps its own checks
    assert N.lib.pkv_workspace_bytes(_desc(N)) == 0 and N.lib.pkv_l2norm_workspace_bytes(loose) == 0
    assert (N.THINK_SCAN_ROWS, N.THINK_TILE_BYTES, N.THINK_QROWS) == (128, 16384, 32)
    src = open(os.path.join(ROOT, "pyramidkv_amd", "csrc", "pkv_kernels.hpp")).read()
    for name in ("THINK_SCAN_ROWS", "THINK_TILE_BYTES", "THINK_QROWS"):
        assert int(re.search(r"constexpr int " + name + r" = (\d+);", src).group(1)) == getattr(N, name)
