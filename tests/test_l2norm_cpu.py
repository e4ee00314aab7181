"""L2Norm on CPU: the canonical restatement (tests/l2norm_ref.py) against the reference's recorded results
(tests/golden/l2norm_*.npz) and, where a checkout of the reference is at hand, against the live reference; the host side of
L2NormCluster (pass-throughs, reset, factory), the plumbing of replace_llama / replace_mistral("l2norm") and the argument
checks of pkv_compress_l2norm.  No kernel is launched here."""
import contextlib
import ctypes
import io
import os
import sys
import types

import numpy as np
import pytest
import torch

import l2norm_ref as R
from inputs import DTYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pyramidkv_amd", "libpkv.so")):
        g.build()
    import pyramidkv_amd
    return pyramidkv_amd


# ------------------------------------------------------------------------------------------------ fixtures
def test_fixture_set_is_complete():
    names = R.fixture_files()
    for dt in ("bf16", "fp16", "fp32"):
        for D in (64, 128, 256):
            assert f"l2norm_grid_{dt}_D{D}.npz" in names
    for n in ("full_permutation_bf16", "skip_layer_fp16", "short_prompt_bf16", "short_prompt_skip_layer_bf16", "tie_free_fp32"):
        assert f"l2norm_{n}.npz" in names
    for n in names:
        assert os.path.getsize(os.path.join(R.GOLD, n)) < 512 * 1024


@pytest.mark.parametrize("name", R.fixture_files())
def test_restatement_reproduces_the_reference_fixture(name):
    meta, k, v, ko_ref, vo_ref = R.load_fixture(name)
    assert k.shape == (meta["B"], meta["H"], meta["S"], meta["D"]) and k.dtype == DTYPES[meta["dtype"]] and meta["B"] == 2
    # the fixture inputs are what they claim to be: squares that sum exactly in fp32 (any order gives the same norm bits)
    assert torch.equal(R.norms_model(k), R.round_dtype(R.norm_f64(k), k.dtype))
    q = torch.zeros_like(k)
    ko, vo, idx = R.l2norm_update_kv(k, q, v, meta["cap"], meta["layer_idx"], meta["skip_layers"], return_indices=True)
    if meta["passthrough"]:
        assert ko is k and vo is v and torch.equal(ko_ref, k) and torch.equal(vo_ref, v)
        return
    gi, ri = R.compare_outputs(k, v, (ko, vo), (ko_ref, vo_ref), meta["cap"])
    assert torch.equal(gi, idx)
    if meta.get("tie_free"):
        assert torch.equal(gi, ri), "tie-free rows: the index sequence itself is the reference's"
        assert torch.equal(ko, ko_ref) and torch.equal(vo, vo_ref)
    if meta["cap"] == meta["S"]:                       # q_len == cap is not a pass-through: a full permutation
        assert torch.equal(gi.sort(-1).values, torch.arange(meta["S"]).expand_as(gi))


def test_fixtures_hold_ties_where_the_contract_says_so():
    """Equal norms are the normal case on these inputs (and the boundary value is tied in some head): the comparison above is
    not vacuously an exact one."""
    meta, k, v, ko_ref, vo_ref = R.load_fixture("l2norm_grid_bf16_D64.npz")
    n = R.norms_model(k)
    assert all(n[b, h].unique().numel() < meta["S"] for b in range(2) for h in range(2))
    meta, k, *_ = R.load_fixture("l2norm_tie_free_fp32.npz")
    n = R.norms_model(k)
    assert all(n[b, h].unique().numel() == meta["S"] for b in range(2) for h in range(2))


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


def test_restatement_against_the_live_reference_on_random_grids():
    ref = _reference()
    rng = np.random.default_rng(20240607)
    ran = 0
    for _ in range(24):
        dt = ("bf16", "fp16", "fp32")[int(rng.integers(0, 3))]
        D = int(rng.choice([64, 128, 256]))
        B, H, S = int(rng.integers(1, 3)), int(rng.choice([1, 2, 4])), int(rng.integers(2, 200))
        cap = int(rng.integers(1, S + 20))
        layer, skip = int(rng.integers(0, 4)), [0, 1][:int(rng.integers(0, 3))]
        k, v = R.grid_kv(B, H, S, D, dt, int(rng.integers(1, 1 << 30)))
        q = torch.zeros_like(k)
        cl = ref.L2NormCluster(max_capacity_prompt=cap, layer_idx=layer, skip_layers=list(skip))
        with contextlib.redirect_stdout(io.StringIO()):
            kr, vr = cl.update_kv(k, q, v, None, 1)
        ko, vo = R.l2norm_update_kv(k, q, v, cap, layer, skip)
        if S < cap or layer in skip:
            assert kr is k and vr is v and ko is k and vo is v
            continue
        R.compare_outputs(k, v, (ko, vo), (kr, vr), cap)
        ran += 1
    assert ran >= 8


# ------------------------------------------------------------------------------------------------ host side of the cluster
def test_passthroughs_in_the_reference_order_and_reset(P):
    k, v = R.grid_kv(1, 4, 30, 64, "bf16", 1)
    q = torch.zeros_like(k)
    cl = P.L2NormCluster(max_capacity_prompt=64, layer_idx=0, skip_layers=[0, 1])
    ko, vo = cl.update_kv(k, q, v, None, 1)                 # short prompt first (:413), then the skip list (:415): same objects
    assert ko is k and vo is v
    cl = P.L2NormCluster(max_capacity_prompt=16, layer_idx=1, skip_layers=[0, 1])
    ko, vo = cl.update_kv(k, q, v, None, 1)
    assert ko is k and vo is v
    # un-expanded K/V come back as the repeat_kv tensors the reference would have been handed
    ku, vu = k[:, :2], v[:, :2]
    ko, vo = cl.update_kv(ku, q, vu, None, 2)
    assert ko.shape == k.shape and torch.equal(ko[:, 0], ku[:, 0]) and torch.equal(ko[:, 1], ku[:, 0]) and torch.equal(vo[:, 3], vu[:, 1])
    # a layer that is not skipped selects: CPU tensors have no path (no eager fallback)
    cl.reset(max_capacity_prompt=16, layer_idx=2, skip_layers=[0, 1])
    assert (cl.max_capacity_prompt, cl.layer_idx, cl.skip_layers) == (16, 2, [0, 1])
    with pytest.raises(RuntimeError):
        cl.update_kv(k, q, v, None, 1)
    with pytest.raises(AssertionError):                     # :408
        cl.update_kv(k, q[:, :, :-1], v, None, 1)
    cl.reset()
    assert (cl.max_capacity_prompt, cl.layer_idx, cl.skip_layers) == (256 + 64, 0, [])
    a, b = P.L2NormCluster(), P.L2NormCluster()             # the reference's signature shares ONE default list (:395)
    a.skip_layers.append(7)
    assert b.skip_layers == [] and P.L2NormCluster().skip_layers == []
    assert P.L2NormCluster.accepts_unexpanded_kv is True and P.L2NormCluster.index_out is None


def test_factory_defaults_and_the_pinned_placeholder(P):
    U = P.pyramidkv_utils
    with pytest.raises(NotImplementedError, match="init_l2norm_native"):
        U.init_l2norm(object())
    mod = types.SimpleNamespace(config=types.SimpleNamespace(), layer_idx=3)
    U.init_l2norm_native(mod)
    cl = mod.kv_cluster
    assert isinstance(cl, P.L2NormCluster)
    assert (cl.max_capacity_prompt, cl.layer_idx, cl.skip_layers) == (4096, 3, [0, 1])        # reference :954-968
    assert (mod.config.max_capacity_prompt, mod.config.layer_idx, mod.config.skip_layers) == (4096, 0, [0, 1])
    mod.config.max_capacity_prompt = 77
    U.init_l2norm_native(mod)                               # rebuilt on every call, reading the config again
    assert mod.kv_cluster is not cl and mod.kv_cluster.max_capacity_prompt == 77
    from pyramidkv_amd import monkeypatch as mp
    assert mp._METHODS["l2norm"] == ("init_l2norm_native", False)
    assert P.init_l2norm_native is U.init_l2norm_native


# ------------------------------------------------------------------------------------------------ replace_llama / replace_mistral
class _RefCluster:
    """Restatement-backed stand-in for L2NormCluster on CPU (the product cluster needs a GPU)."""
    accepts_unexpanded_kv = True

    def __init__(self, cfg, layer_idx):
        self.cfg, self.layer_idx = cfg, layer_idx

    def update_kv(self, k, q, v, mask, groups):
        g = q.shape[1] // k.shape[1]
        if g > 1:
            b, h, s, d = k.shape
            k = k[:, :, None].expand(b, h, g, s, d).reshape(b, h * g, s, d)
            v = v[:, :, None].expand(b, h, g, s, d).reshape(b, h * g, s, d)
        return R.l2norm_update_kv(k, q, v, self.cfg.max_capacity_prompt, self.layer_idx, self.cfg.skip_layers)


@pytest.fixture
def patched():
    pytest.importorskip("transformers")
    from pyramidkv_amd import monkeypatch as mp
    saved = mp._cluster_module
    m = types.SimpleNamespace()
    m.init_l2norm_native = lambda self: setattr(self, "kv_cluster", _RefCluster(self.config, self.layer_idx))
    mp._cluster_module = m
    yield mp
    mp._cluster_module = saved
    mp.restore()


def _tiny(family, layers=4):
    torch.manual_seed(0)
    kw = dict(vocab_size=97, hidden_size=256, intermediate_size=512, num_hidden_layers=layers, num_attention_heads=2,
              num_key_value_heads=1, head_dim=128, max_position_embeddings=4096)
    if family == "llama":
        from transformers import LlamaConfig, LlamaForCausalLM
        return LlamaForCausalLM(LlamaConfig(**kw)).eval()
    from transformers import MistralConfig, MistralForCausalLM
    return MistralForCausalLM(MistralConfig(sliding_window=None, **kw)).eval()


@pytest.mark.parametrize("family", ["llama", "mistral"])
def test_replace_l2norm_plumbing(patched, family):
    from transformers import DynamicCache
    model = _tiny(family)
    S, new, cap = 120, 4, 48
    ids = torch.randint(0, 97, (1, S), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        base = model(ids).logits
    (patched.replace_llama if family == "llama" else patched.replace_mistral)("l2norm")
    for layer in model.model.layers:
        c = layer.self_attn.config
        c.max_capacity_prompt, c.skip_layers = cap, [0, 1]
    cache = DynamicCache(config=model.config)
    with torch.no_grad():
        out = model(ids, past_key_values=cache, use_cache=True)
    assert torch.allclose(out.logits, base, atol=1e-4, rtol=1e-4)          # the prompt attends to the full K/V
    H = model.config.num_attention_heads
    want = [S, S, cap, cap]                                                 # layers 0 and 1 are skipped: the full cache
    assert [tuple(l.keys.shape[1:3]) for l in cache.layers] == [(H, n) for n in want]
    for l in cache.layers[2:]:                                              # ascending-norm rows
        n = R.norms_model(l.keys).float()
        assert bool((n[..., 1:] >= n[..., :-1]).all())
    nxt = out.logits[:, -1:].argmax(-1)
    with torch.no_grad():
        for t in range(new):
            o = model(nxt, past_key_values=cache, use_cache=True)
            nxt = o.logits[:, -1:].argmax(-1)
            assert torch.isfinite(o.logits).all()
    assert [l.keys.shape[2] for l in cache.layers] == [n + new for n in want]
    assert cache.get_seq_length() == S + new


# ------------------------------------------------------------------------------------------------ argument checks (no launch)
def _desc(N, dtype=0, B=1, H=4, S=256, D=128, g=1, cap=64, window=0):
    d = N.PkvDesc()
    d.dtype, d.B, d.H, d.S, d.D, d.kv_group, d.window, d.topk = dtype, B, H, S, D, g, window, cap
    for i, st in enumerate((H // g * S * D, S * D, D)):
        d.k_stride[i] = d.v_stride[i] = d.q_stride[i] = st
    return d


def test_compress_l2norm_argument_checks(P):
    N = P._native
    call = lambda d, ws=1 << 30: N.lib.pkv_compress_l2norm(d, 16, 16, 16, 16, None, None, 16, ws, None)   # noqa: E731
    good = _desc(N)
    nb = N.lib.pkv_l2norm_workspace_bytes(good)
    assert nb > 0 and nb % 256 == 0
    assert call(good, nb - 1) == -4                                         # PKV_ERR_WORKSPACE (checked before any launch)
    assert call(_desc(N, window=8)) == -2 and N.lib.pkv_l2norm_workspace_bytes(_desc(N, window=8)) == 0     # PKV_ERR_SHAPE
    assert call(_desc(N, cap=257)) == -2 and call(_desc(N, cap=0)) == -2
    assert call(_desc(N, D=96)) == -2
    assert call(_desc(N, dtype=3)) == -1
    assert call(_desc(N, H=6, g=4)) == -2
    assert call(_desc(N, dtype=2, S=8192, cap=4097)) == -5                  # PKV_ERR_UNSUPPORTED: fp32 selection holds 4096 winners
    assert call(_desc(N, S=65536, cap=16385)) == -5                    # beyond the segmented route (k <= 4096): never a fallback
    assert N.lib.pkv_compress_l2norm(good, None, 16, 16, 16, None, None, 16, nb, None) == -7
    assert N.lib.pkv_compress_l2norm(good, 16, 16, 16, 16, None, 8, 16, nb, None) == -3       # norm_out off a 16-byte boundary
    bad = _desc(N)
    bad.struct_size = 132
    assert call(bad) == -9 and N.lib.pkv_l2norm_workspace_bytes(bad) == 0
    # every other entry point keeps rejecting window < 1
    assert N.lib.pkv_workspace_bytes(_desc(N)) == 0
    assert N.lib.pkv_compress(_desc(N), 16, 16, 16, 16, 16, None, 16, 1 << 30, None) == -2
    assert N.lib.pkv_gather_streaming(_desc(N), 16, 16, 16, 16, None) == -2
    # one selection row per KV head: a GQA group of 4 needs about a quarter of the score / selection scratch
    assert N.lib.pkv_l2norm_workspace_bytes(_desc(N, H=32, S=32768, g=4, cap=4096)) < N.lib.pkv_l2norm_workspace_bytes(_desc(N, H=32, S=32768, cap=4096))
    assert N.lib.pkv_version() == N.PKV_VERSION == 204 and "l2norm" in N.KERNEL_NAMES
    assert isinstance(ctypes.sizeof(N.PkvDesc), int) and ctypes.sizeof(N.PkvDesc) == 136      # the descriptor did not grow
