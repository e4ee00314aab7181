"""L2Norm on the GPU: key-norm scan -> lowest-norm selection -> gather (pkv_compress_l2norm, ops.compress_l2norm,
L2NormCluster, replace_llama / replace_mistral("l2norm")).  Nothing here reads the reference tree: its results enter as
tests/golden/l2norm_*.npz; bars and restatement live in tests/l2norm_ref.py."""
import ctypes

import pytest
import torch

import l2norm_ref as R
from inputs import DTYPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def P():
    import pyramidkv_amd
    return pyramidkv_amd


def _gauss(B, H, S, D, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    k = (torch.randn(B, H, S, D, generator=g) * scale).to(DTYPES[dtype])
    v = torch.randn(B, H, S, D, generator=g).to(DTYPES[dtype])
    return k, v


def _want_order(norms: torch.Tensor, cap: int) -> torch.Tensor:
    """Stable ascending argsort of the kernel's own norms; a NaN norm counts as +inf (ordered with it, by index)."""
    n = norms.detach().cpu().float()
    n = torch.where(torch.isnan(n), torch.full_like(n, float("inf")), n)
    return torch.argsort(n, dim=-1, stable=True)[..., :cap].to(torch.int32)


def _run(P, k, v, cap, g=1):
    ko, vo, idx, norms = P.ops.compress_l2norm(k.to(DEV), v.to(DEV), cap, kv_group=g, return_indices=True, return_norms=True)
    torch.cuda.synchronize()
    return ko.cpu(), vo.cpu(), idx.cpu(), norms.cpu()


def _check_selection_and_movement(k, v, ko, vo, idx, norms, cap, g=1):
    B, Hk, S, D = k.shape
    assert norms.shape == (B, Hk, S) and idx.shape == (B, Hk * g, cap) and ko.shape == vo.shape == (B, Hk * g, cap, D)
    want = _want_order(norms, cap)                                            # [B, Hk, cap]
    want = want[:, :, None].expand(B, Hk, g, cap).reshape(B, Hk * g, cap)
    assert int(idx.min()) >= 0 and int(idx.max()) < S
    assert torch.equal(idx, want), "indices are not the stable ascending argsort of the kernel's norms"
    ke = k[:, :, None].expand(B, Hk, g, S, D).reshape(B, Hk * g, S, D)
    ve = v[:, :, None].expand(B, Hk, g, S, D).reshape(B, Hk * g, S, D)
    ix = idx.long()[..., None].expand(-1, -1, -1, D)
    assert torch.equal(ko.view(torch.uint8), ke.gather(2, ix).contiguous().view(torch.uint8)), "K rows are not bit copies"
    assert torch.equal(vo.view(torch.uint8), ve.gather(2, ix).contiguous().view(torch.uint8)), "V rows are not bit copies"


# ------------------------------------------------------------------------------------------------ 0. the square root
def test_kernel_sqrt_is_correctly_rounded(P):
    """The build keeps hipcc's correctly rounded fp32 sqrt: pkv_debug_sqrt runs the device function the norm scan inlines."""
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.rand(1 << 18, generator=g) * 300.0,                                   # sums of squares of real rows
                   torch.exp(torch.rand(1 << 18, generator=g) * 170.0 - 85.0),                 # the whole normal range
                   torch.rand(1 << 12, generator=g) * 1e-39,                                   # subnormals
                   torch.tensor([0.0, 1.0, 2.0, 4.0, float("inf"), 3.4028234e38, 1.17549435e-38, 1e-45])])
    xd = x.to(DEV)
    out = torch.empty_like(xd)
    N = P._native
    N.check(N.lib.pkv_debug_sqrt(xd.data_ptr(), out.data_ptr(), xd.numel(), N.stream_ptr()), "pkv_debug_sqrt")
    torch.cuda.synchronize()
    want = x.double().sqrt().float()               # float64 root, rounded once more: the correctly rounded fp32 root (53 >= 2 * 24 + 2)
    bad = out.cpu().view(torch.int32) != want.view(torch.int32)
    print("sqrt: differing", int(bad.sum()), "of", x.numel())
    assert not bool(bad.any())


# ------------------------------------------------------------------------------------------------ 1. norms
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_norms_gaussian_rows(P, dtype, D):
    """norm_out against round_dtype(norm_f64): exact outside the input-defined exempt set (tests/l2norm_ref.py norm_bar)."""
    S = 32768 if D == 128 else 8192
    k, v = _gauss(1, 8, S, D, dtype, 100 + D)
    _, _, _, norms = _run(P, k, v, 64)
    R.norm_bar(k, norms)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_norms_exact_grid_rows_have_no_exemption(P, dtype, D):
    for S in (4096, 1003):                         # 1003: rows that do not end on an 8-row boundary (element-wise norm stores)
        k, v = R.grid_kv(2, 3, S, D, dtype, 7 * D + S)
        _, _, _, norms = _run(P, k, v, 64)
        fig = R.norm_bar(k, norms, exact_grid=True)
        assert fig.get("differ", 0) == 0
        assert torch.equal(norms, R.norms_model(k))


# ------------------------------------------------------------------------------------------------ 2. + 3. selection, movement
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("cap", [64, 2048, 4096])
def test_selection_and_movement_all_dtypes_and_head_sizes(P, dtype, D, cap):
    k, v = _gauss(2, 2, 8192, D, dtype, 11 * D + cap)
    _check_selection_and_movement(k, v, *_run(P, k, v, cap), cap)


@pytest.mark.parametrize("dtype,S,cap", [("bf16", 32768, 4096), ("fp16", 32768, 2048), ("fp32", 32768, 4096),
                                         ("bf16", 32768, 16384),          # one workgroup's largest budget
                                         ("bf16", 32768, 20000),          # beyond it: the complete sort of the row
                                         ("fp16", 32768, 32768),          # ... as a full permutation
                                         ("bf16", 57344, 4096),           # the longest single-workgroup row
                                         ("bf16", 131072, 4096),          # segmented long row
                                         ("fp16", 300, 300), ("fp32", 257, 257), ("bf16", 2, 2), ("bf16", 1, 1),   # cap == S
                                         ("bf16", 333, 100), ("fp32", 1001, 64)])
def test_selection_routes(P, dtype, S, cap):
    H = 2 if S > 40000 else 4
    k, v = _gauss(1, H, S, 128, dtype, S + cap)
    ko, vo, idx, norms = _run(P, k, v, cap)
    _check_selection_and_movement(k, v, ko, vo, idx, norms, cap)
    if cap == S:
        assert torch.equal(idx.sort(-1).values, torch.arange(S, dtype=torch.int32).expand_as(idx))


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_selection_degenerate_rows(P, dtype):
    S, D, cap = 4096, 128, 512
    k, v = _gauss(1, 4, S, D, dtype, 5)
    k[0, 0] = k[0, 0, 0].clone()                                                   # all rows equal: the first cap indices
    k[0, 1, ::3] = 0                                                           # zero-norm keys come first, by index
    k[0, 2, 5::7] = 0
    k[0, 2, 100:200] = k[0, 2, 100].clone()
    ko, vo, idx, norms = _run(P, k, v, cap)
    _check_selection_and_movement(k, v, ko, vo, idx, norms, cap)
    assert torch.equal(idx[0, 0], torch.arange(cap, dtype=torch.int32))
    assert torch.equal(idx[0, 1], torch.arange(0, 3 * cap, 3, dtype=torch.int32))
    assert bool((norms[0, 1, ::3] == 0).all()) and not bool(torch.signbit(norms[0, 1, ::3]).any())


def test_selection_fp16_rows_overflowing_to_inf(P):
    S, D, cap = 2048, 128, 1536
    k, v = _gauss(1, 2, S, D, "fp16", 9)
    k[0, 0, 1::2] = 30000.0                                                    # norm 30000 * sqrt(128) > 65504: +inf in fp16
    k[0, 1, :1000, 0] = float("inf")
    ko, vo, idx, norms = _run(P, k, v, cap)
    assert bool(torch.isinf(norms[0, 0, 1::2]).all()) and bool(torch.isinf(norms[0, 1, :1000]).all())
    _check_selection_and_movement(k, v, ko, vo, idx, norms, cap)
    assert torch.equal(idx[0, 0, 1024:], torch.arange(1, 1024, 2, dtype=torch.int32))          # +inf last, by index
    assert torch.equal(idx[0, 1, 1048:], torch.arange(0, cap - 1048, dtype=torch.int32))


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_nan_norms_are_safe_and_ordered_with_inf(P, dtype):
    """Outside the parity contract (the reference sorts NaN behind +inf): never an out-of-range index, ordered with +inf by index."""
    S, D, cap = 1024, 64, 1024
    k, v = _gauss(1, 2, S, D, dtype, 13)
    k[0, 0, 10, 3] = float("nan")
    k[0, 0, 500, 0] = float("inf")
    k[0, 0, 700, 1] = float("nan")
    ko, vo, idx, norms = _run(P, k, v, cap)
    assert bool(torch.isnan(norms[0, 0, 10])) and bool(torch.isinf(norms[0, 0, 500])) and bool(torch.isnan(norms[0, 0, 700]))
    assert idx[0, 0, -3:].tolist() == [10, 500, 700]
    assert torch.equal(idx, _want_order(norms, cap))
    assert torch.equal(idx.sort(-1).values, torch.arange(S, dtype=torch.int32).expand_as(idx))


def test_strided_views_and_batch(P):
    """Non-contiguous K/V (a sequence slice of a longer buffer, every second head of a wider one), B = 2."""
    g = torch.Generator().manual_seed(21)
    big_k = torch.randn(2, 8, 3000, 128, generator=g).to(torch.bfloat16).to(DEV)
    big_v = torch.randn(2, 8, 3000, 128, generator=g).to(torch.bfloat16).to(DEV)
    kview, vview = big_k[:, ::2, 200:2248], big_v[:, 1::2, 8:2056]
    assert not kview.is_contiguous()
    ko, vo, idx, norms = P.ops.compress_l2norm(kview, vview, 777, return_indices=True, return_norms=True)
    torch.cuda.synchronize()
    _check_selection_and_movement(kview.cpu().contiguous(), vview.cpu().contiguous(), ko.cpu(), vo.cpu(), idx.cpu(), norms.cpu(), 777)
    R.norm_bar(kview.cpu().contiguous(), norms.cpu())
    tr_k = torch.randn(2, 2048, 4, 64, generator=g).to(torch.float16).to(DEV).transpose(1, 2)   # [B,H,S,D] view of [B,S,H,D]
    tr_v = torch.randn(2, 2048, 4, 64, generator=g).to(torch.float16).to(DEV).transpose(1, 2)
    ko, vo, idx, norms = P.ops.compress_l2norm(tr_k, tr_v, 100, return_indices=True, return_norms=True)
    torch.cuda.synchronize()
    _check_selection_and_movement(tr_k.cpu().contiguous(), tr_v.cpu().contiguous(), ko.cpu(), vo.cpu(), idx.cpu(), norms.cpu(), 100)


# ------------------------------------------------------------------------------------------------ 4. GQA
@pytest.mark.parametrize("g", [4, 8])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_gqa_unexpanded_and_materialised_equal_the_expanded_call(P, g, dtype):
    from pyramidkv_amd import config as cfg
    B, Hk, S, D, cap = 2, 2, 4096, 128, 1000
    ku, vu = _gauss(B, Hk, S, D, dtype, 31 + g)
    ke = ku[:, :, None].expand(B, Hk, g, S, D).reshape(B, Hk * g, S, D).contiguous()
    ve = vu[:, :, None].expand(B, Hk, g, S, D).reshape(B, Hk * g, S, D).contiguous()
    q = torch.empty(B, Hk * g, S, D, dtype=ku.dtype, device=DEV)
    ko, vo, idx, norms = _run(P, ke, ve, cap)                                               # the expanded call
    _check_selection_and_movement(ke, ve, ko, vo, idx, norms, cap)
    ko_u, vo_u, idx_u, norms_u = _run(P, ku, vu, cap, g)                                    # un-expanded: one selection row per KV head
    _check_selection_and_movement(ku, vu, ko_u, vo_u, idx_u, norms_u, cap, g)
    assert torch.equal(idx_u, idx) and torch.equal(ko_u, ko) and torch.equal(vo_u, vo)
    cl = P.L2NormCluster(max_capacity_prompt=cap, layer_idx=2, skip_layers=[0, 1])
    buf = torch.full((B, Hk * g, cap), -1, dtype=torch.int32, device=DEV)
    cl.index_out = buf
    a = cl.update_kv(ku.to(DEV), q, vu.to(DEV), None, g)                                    # un-expanded through the cluster
    assert torch.equal(a[0].cpu(), ko) and torch.equal(a[1].cpu(), vo) and torch.equal(buf.cpu(), idx)
    saved = cfg.gqa_dedup
    try:
        for dedup in (False, True):                                                         # materialised repeat_kv tensors
            cfg.gqa_dedup = dedup
            b = cl.update_kv(ke.to(DEV), q, ve.to(DEV), None, g)
            assert torch.equal(b[0].cpu(), ko) and torch.equal(b[1].cpu(), vo)
    finally:
        cfg.gqa_dedup = saved


# ------------------------------------------------------------------------------------------------ 5. fixtures
@pytest.mark.parametrize("name", R.fixture_files())
def test_fixtures_through_the_cluster(P, name):
    meta, k, v, ko_ref, vo_ref = R.load_fixture(name)
    cl = P.L2NormCluster(max_capacity_prompt=meta["cap"], layer_idx=meta["layer_idx"], skip_layers=list(meta["skip_layers"]))
    kd, vd = k.to(DEV), v.to(DEV)
    q = torch.empty_like(kd)
    ko, vo = cl.update_kv(kd, q, vd, None, 1)
    if meta["passthrough"]:
        assert ko is kd and vo is vd
        return
    torch.cuda.synchronize()
    ko, vo = ko.cpu(), vo.cpu()
    gi, ri = R.compare_outputs(k, v, (ko, vo), (ko_ref, vo_ref), meta["cap"])
    if meta.get("tie_free"):
        assert torch.equal(gi, ri) and torch.equal(ko, ko_ref) and torch.equal(vo, vo_ref)
    ks, vs, _ = R.l2norm_update_kv(k, torch.zeros_like(k), v, meta["cap"], meta["layer_idx"], meta["skip_layers"], return_indices=True)
    assert torch.equal(ko, ks) and torch.equal(vo, vs)             # bit-identical to the canonical restatement


# ------------------------------------------------------------------------------------------------ 6. ABI errors
def test_abi_errors_on_device_buffers(P):
    N = P._native
    k, v = _gauss(1, 2, 512, 128, "bf16", 1)
    kd, vd = k.to(DEV), v.to(DEV)
    ko, vo = torch.empty(1, 2, 512, 128, dtype=kd.dtype, device=DEV), torch.empty(1, 2, 512, 128, dtype=kd.dtype, device=DEV)
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=DEV)

    def call(ws_bytes=ws.numel(), **kw):
        d = P.ops.make_desc(None, kd, vd, kw.pop("window", 0), topk=kw.pop("cap", 64), num_heads=2)
        for name, val in kw.items():
            setattr(d, name, val)
        return N.lib.pkv_compress_l2norm(d, kd.data_ptr(), vd.data_ptr(), ko.data_ptr(), vo.data_ptr(), None, None, ws.data_ptr(),
                                         ws_bytes, N.stream_ptr())
    assert call() == 0
    assert call(window=8) == -2                      # PKV_ERR_SHAPE
    assert call(cap=513) == -2
    assert call(D=96) == -2
    assert call(dtype=2, S=8192, cap=4097) == -5     # PKV_ERR_UNSUPPORTED (validated before anything is read)
    d = P.ops.make_desc(None, kd, vd, 0, topk=64, num_heads=2)
    need = N.lib.pkv_l2norm_workspace_bytes(d)
    assert 0 < need <= ws.numel() and call(ws_bytes=need - 1) == -4 and call(ws_bytes=need) == 0      # PKV_ERR_WORKSPACE
    torch.cuda.synchronize()
    with pytest.raises(ValueError):                  # the Python layer turns the status into an exception, never a fallback
        P.ops.compress_l2norm(kd, vd, 513)
    big = torch.zeros(1, 1, 65536, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="outside the limits"):
        P.ops.compress_l2norm(big, big, 16385)       # beyond the segmented route
    with pytest.raises(ValueError):
        P.ops.compress_l2norm(kd, vd, 64, idx_out=torch.empty(5, dtype=torch.int32, device=DEV))
    assert ctypes.sizeof(N.PkvDesc) == 136


# ------------------------------------------------------------------------------------------------ 7. end to end
@pytest.mark.parametrize("family", ["llama", "mistral"])
def test_end_to_end_tiny_model(P, family):
    pytest.importorskip("transformers")
    from transformers import DynamicCache
    from pyramidkv_amd import monkeypatch as mp
    torch.manual_seed(0)
    kw = dict(vocab_size=97, hidden_size=256, intermediate_size=512, num_hidden_layers=4, num_attention_heads=2,
              num_key_value_heads=1, head_dim=128, max_position_embeddings=4096)
    if family == "llama":
        from transformers import LlamaConfig, LlamaForCausalLM
        model = LlamaForCausalLM(LlamaConfig(**kw))
    else:
        from transformers import MistralConfig, MistralForCausalLM
        model = MistralForCausalLM(MistralConfig(sliding_window=None, **kw))
    model = model.eval().to(DEV)
    S, new, cap, D = 200, 3, 64, 128
    ids = torch.randint(0, 97, (1, S), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        base = model(ids).logits
    try:
        (mp.replace_llama if family == "llama" else mp.replace_mistral)("l2norm")
        # the patched forward itself, with a budget above the prompt length: every layer passes through, the cache holds the
        # full K of every layer exactly as the compressing run below computes it
        for layer in model.model.layers:
            c = layer.self_attn.config
            c.max_capacity_prompt, c.skip_layers = S + 1, [0, 1]
        full = DynamicCache(config=model.config)
        with torch.no_grad():
            model(ids, past_key_values=full, use_cache=True)
        full_k = [l.keys.cpu() for l in full.layers]                    # [1, H, S, D] per layer, after RoPE and repeat_kv
        assert all(t.shape == (1, 2, S, D) for t in full_k)
        for layer in model.model.layers:
            layer.self_attn.config.max_capacity_prompt = cap
        cache = DynamicCache(config=model.config)
        with torch.no_grad():
            out = model(ids, past_key_values=cache, use_cache=True)
        assert torch.allclose(out.logits, base, atol=1e-3, rtol=1e-3)   # the prompt attends to the full K/V
        assert isinstance(model.model.layers[2].self_attn.kv_cluster, P.L2NormCluster)
        H = model.config.num_attention_heads
        assert [tuple(l.keys.shape[1:3]) for l in cache.layers] == [(H, S), (H, S), (H, cap), (H, cap)]
        for li in (2, 3):
            # the kernel's own norms of the layer's full K decide: the cached keys are exactly the rows the stable ascending
            # argsort of those norms names, in that order (so their norms are non-decreasing, exactly)
            src = full_k[li].to(DEV)
            _, _, idx, nrm = P.ops.compress_l2norm(src, src, cap, return_indices=True, return_norms=True)
            want = torch.argsort(nrm.cpu().float(), dim=-1, stable=True)[..., :cap]
            assert torch.equal(idx.cpu().long(), want)
            picked = nrm.cpu().float().gather(2, want)
            assert bool((picked[..., 1:] >= picked[..., :-1]).all())
            rows = full_k[li].gather(2, want[..., None].expand(-1, -1, -1, D))
            assert torch.equal(cache.layers[li].keys.cpu(), rows)        # every cached key is that row of the layer's full K
        nxt = out.logits[:, -1:].argmax(-1)
        with torch.no_grad():
            for t in range(new):
                o = model(nxt, past_key_values=cache, use_cache=True)
                nxt = o.logits[:, -1:].argmax(-1)
                assert bool(torch.isfinite(o.logits).all())
        assert [l.keys.shape[2] for l in cache.layers] == [S + new, S + new, cap + new, cap + new]
    finally:
        mp.restore()
        for layer in model.model.layers:
            if hasattr(layer.self_attn, "kv_cluster"):
                del layer.self_attn.kv_cluster
