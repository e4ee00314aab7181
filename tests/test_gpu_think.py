"""ThinK on the GPU: channel-energy scan -> select -> channel compaction (pkv_think_prune, ops.think_prune,
SnapKVCluster.update_think, replace_llama("think")).  Nothing here reads the reference tree: its results enter as
tests/golden/think_*.npz; bars and restatement live in tests/think_ref.py."""
import types

import pytest
import torch

import think_ref as T
from inputs import DTYPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def P():
    import pyramidkv_amd
    return pyramidkv_amd


def _gauss(B, H, S, N, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    dt = DTYPES[dtype] if isinstance(dtype, str) else dtype
    return torch.randn(B, H, S, D, generator=g).to(dt), torch.randn(B, H, N, D, generator=g).to(dt)


def _run(P, q, kc, recent, n_prune, **kw):
    out = P.ops.think_prune(q.to(DEV), kc.to(DEV), recent, n_prune, return_keep_idx=True, return_stats=True, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)                       # k_pruned, keep, keep_idx, stats


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _check_selection_and_movement(kc, recent, n_prune, kp, keep, kidx, stats):
    """3. + 4.: keep / keep_idx are the canonical answer to the kernel's OWN scores; k_pruned is a bit copy through keep_idx."""
    B, H, N, D = kc.shape
    R, W = N - recent, D - n_prune
    assert kp.shape == (1, B * H, R, W) and keep.shape == (B, H, D) and keep.dtype == torch.bool
    assert kidx.shape == (B, H, W) and kidx.dtype == torch.int32 and stats.shape == (B, H, 3, D)
    want_keep, want_idx = T.canonical_keep(stats[:, :, 2], n_prune)
    assert set(_bytes(keep).unique().tolist()) <= {0, 1}, "keep bytes are 0 or 1"
    assert torch.equal(keep, want_keep), "keep is not the canonical selection on the kernel's scores"
    assert torch.equal(kidx.long(), want_idx), "keep_idx is not the ascending list of the kept channels"
    assert torch.equal(_bytes(kp), _bytes(T.compact(kc, kidx, recent))), "k_pruned is not a bit copy through keep_idx"


# ------------------------------------------------------------------------------------------------ 1. + 2. energies, score
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_energies_and_score(P, dtype, D):
    """n in {20, 72, 160} rows: qe over min(32, S) query rows (S = 20: all of them), ke over N key rows."""
    for S, N in ((20, 72), (50, 160), (300, 20)):
        q, kc = _gauss(2, 3, S, N, D, dtype, 31 * D + S)
        kp, keep, kidx, st = _run(P, q, kc, 3, int(D * 0.4))
        nq = min(32, S)
        T.energy_bar(q[:, :, S - nq:], st[:, :, 0], nq)
        T.energy_bar(kc, st[:, :, 1], N)
        want = (st[:, :, 0].float() * st[:, :, 1].float()).to(kc.dtype)           # from the kernel's own energies: one rounding
        assert torch.equal(_bytes(st[:, :, 2]), _bytes(want))
        _check_selection_and_movement(kc, 3, int(D * 0.4), kp, keep, kidx, st)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_energies_are_exact_on_scaled_grids(P, dtype, D):
    for S, N in ((20, 72), (160, 160)):
        q, kc = T.scaled_grid(2, 2, max(S, N), D, dtype, 17 * D + N)
        q, kc = q[:, :, :S].contiguous(), kc[:, :, :N].contiguous()
        _, _, _, st = _run(P, q, kc, 1, int(D * 0.3))
        qe, ke, sc = T.scores(q, kc)
        assert torch.equal(_bytes(st[:, :, 0]), _bytes(qe)) and torch.equal(_bytes(st[:, :, 1]), _bytes(ke))
        assert torch.equal(_bytes(st[:, :, 2]), _bytes(sc))
        T.energy_bar(kc, st[:, :, 1], N, exact_grid=True)


# ------------------------------------------------------------------------------------------------ 3. selection
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_selection_counts(P, dtype, D):
    q, kc = _gauss(1, 4, 40, 72, D, dtype, 5 * D)
    for k in (0, 1, int(0.3 * D), int(0.4 * D), D - 1):
        _check_selection_and_movement(kc, 32, k, *_run(P, q, kc, 32, k))


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_selection_on_planted_rows(P, dtype):
    D, N, S = 128, 40, 40
    dt = DTYPES[dtype]
    k = 51
    # all channels equal: prune 0 .. k-1
    q, kc = torch.full((1, 1, S, D), 0.5).to(dt), torch.full((1, 1, N, D), 0.25).to(dt)
    kp, keep, kidx, st = _run(P, q, kc, 8, k)
    assert keep[0, 0].tolist() == [False] * k + [True] * (D - k) and kidx[0, 0].tolist() == list(range(k, D))
    _check_selection_and_movement(kc, 8, k, kp, keep, kidx, st)
    # two values: the low one on the even channels - all 64 of them go first, lowest index first
    kc2 = kc.clone()
    kc2[..., 1::2] = 1.0
    for kk in (10, 64, 70):
        kp, keep, kidx, st = _run(P, q, kc2, 8, kk)
        gone = list(range(0, 2 * min(kk, 64), 2)) + list(range(1, 2 * max(kk - 64, 0), 2))     # even channels first, then odd ones
        want = [c not in gone for c in range(D)]
        assert keep[0, 0].tolist() == want
        _check_selection_and_movement(kc2, 8, kk, kp, keep, kidx, st)
    # a zero query channel is pruned first, whatever its keys hold
    q3, kc3 = _gauss(1, 2, S, N, D, dtype, 9)
    q3[..., 77] = 0
    kc3[..., 77] = 50.0
    kp, keep, kidx, st = _run(P, q3, kc3, 8, 1)
    assert not keep[:, :, 77].any() and int(keep.sum()) == 2 * (D - 1) and bool((st[:, :, 2, 77] == 0).all())
    _check_selection_and_movement(kc3, 8, 1, kp, keep, kidx, st)
    # a NaN channel and a +inf channel in K: kept unless k reaches them, +inf before NaN
    q4, kc4 = _gauss(1, 1, S, N, D, dtype, 10)
    kc4[0, 0, 3, 20] = float("nan")
    kc4[0, 0, 5, 90] = float("inf")
    for kk, nan_kept, inf_kept in ((51, True, True), (D - 2, True, True), (D - 1, True, False)):
        kp, keep, kidx, st = _run(P, q4, kc4, 8, kk)
        assert torch.isnan(st[0, 0, 2, 20]) and torch.isinf(st[0, 0, 2, 90])
        assert bool(keep[0, 0, 20]) == nan_kept and bool(keep[0, 0, 90]) == inf_kept
        _check_selection_and_movement(kc4, 8, kk, kp, keep, kidx, st)


# ------------------------------------------------------------------------------------------------ 4. movement
def _tile_rows(P, D, dtype):
    return P._native.THINK_TILE_BYTES // (D * DTYPES[dtype].itemsize)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_movement_widths_and_row_counts(P, dtype, D):
    """Kept widths 39/45, 77/90, 154/180, D and 1; R = 1; rows around the scan's chunk and around the compaction's tile."""
    SR, TR = P._native.THINK_SCAN_ROWS, _tile_rows(P, D, dtype)
    cases = [(72, 32, int(D * 0.4)), (72, 32, int(D * 0.3)), (72, 32, 0), (72, 32, D - 1), (33, 32, int(D * 0.4)), (1, 0, int(D * 0.3))]
    cases += [(n, 0, int(D * 0.4)) for n in (SR - 1, SR, SR + 1, 2 * SR + 37)]             # scan chunks: below, at, above, three with a ragged last
    cases += [(r + 5, 5, int(D * 0.4)) for r in sorted({TR - 1, TR, TR + 1, 2 * TR + 3})]  # compaction tiles likewise (R = N - 5)
    for N, recent, k in cases:
        q, kc = _gauss(1, 3, 40, N, D, dtype, N * 7 + k)
        _check_selection_and_movement(kc, recent, k, *_run(P, q, kc, recent, k))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_movement_misaligned_head_bases(P, dtype):
    """R * (D - k) * e is no multiple of 16 and B*H > 1: every later head starts off a 16-byte boundary."""
    D, k, R = 128, 51, 7
    e = DTYPES[dtype].itemsize
    assert (R * (D - k) * e) % 16 != 0
    q, kc = _gauss(2, 5, 40, R + 4, D, dtype, 99)
    _check_selection_and_movement(kc, 4, k, *_run(P, q, kc, 4, k))


# ------------------------------------------------------------------------------------------------ 5. canaries
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("D,k", [(64, 25), (128, 51), (256, 77)])
def test_canaries_around_out(P, dtype, D, k):
    dt = DTYPES[dtype]
    e = dt.itemsize
    B, H, N, recent = 1, 3, 45, 4
    R, W = N - recent, D - k
    n = B * H * R * W
    assert n % 2 == 1 and (n * e) % 16 != 0                 # an odd element count: the span ends off a 16-byte boundary
    q, kc = _gauss(B, H, 40, N, D, dtype, 3 * D)
    pad = 64                                                 # elements: 128 / 256 bytes, a 16-byte multiple
    buf = torch.full((pad + n + pad,), -7.0, dtype=dt, device=DEV)
    assert buf.data_ptr() % 16 == 0 and (pad * e) % 16 == 0
    sentinel = _bytes(buf.cpu().clone())
    out = buf[pad:pad + n]
    kp, keep, kidx, st = _run(P, q, kc, recent, k, out=out)
    got = _bytes(buf.cpu())
    assert torch.equal(got[:pad * e], sentinel[:pad * e]), "bytes before the span changed"
    assert torch.equal(got[(pad + n) * e:], sentinel[(pad + n) * e:]), "bytes behind the span changed"
    assert kp.shape == (1, B * H, R, W)
    _check_selection_and_movement(kc, recent, k, kp, keep, kidx, st)


# ------------------------------------------------------------------------------------------------ 6. Q layouts
@pytest.mark.parametrize("S", [20, 32, 33, 300])
def test_q_layouts(P, S):
    """Q as the model's [B,S,H,D].transpose(1,2) view and contiguous: the same bytes out; only the last min(32, S) rows count."""
    B, H, N, D = 2, 4, 48, 128
    q, kc = _gauss(B, H, S, N, D, "bf16", S)
    qd, kd = q.to(DEV), kc.to(DEV)
    q_view = qd.transpose(1, 2).contiguous().transpose(1, 2)                # [B,H,S,D] strided as the model's q is
    assert not q_view.is_contiguous() or S == 1
    a = P.ops.think_prune(qd, kd, 8, 51, return_keep_idx=True, return_stats=True)
    b = P.ops.think_prune(q_view, kd, 8, 51, return_keep_idx=True, return_stats=True)
    q_other = qd.clone()
    q_other[:, :, :max(S - 32, 0)] = 100.0                                  # rows before the last 32 are never read
    c = P.ops.think_prune(q_other, kd, 8, 51, return_keep_idx=True, return_stats=True)
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(_bytes(x.cpu()), _bytes(y.cpu())) and torch.equal(_bytes(x.cpu()), _bytes(z.cpu()))
    nq = min(32, S)
    T.energy_bar(q[:, :, S - nq:], a[3][:, :, 0].cpu(), nq)
    _check_selection_and_movement(kc, 8, 51, *(t.cpu() for t in a))


def test_update_think_takes_unexpanded_kv(P):
    """g = 4: K/V with H/g heads give what the expanded tensors give."""
    from inputs import make_qkv
    q, k, v = make_qkv(1, 8, 300, 128, "bf16", "planted", 5)
    ku, vu = k[:, ::4].contiguous(), v[:, ::4].contiguous()
    ke, ve = ku.repeat_interleave(4, dim=1), vu.repeat_interleave(4, dim=1)
    cl = P.SnapKVCluster(window_size=16, max_capacity_prompt=100, kernel_size=5, pooling="avgpool", recent_size=20, ratio=0.4)
    a = cl.update_think(ku.to(DEV), q.to(DEV), vu.to(DEV), None, 4)
    b = cl.update_think(ke.to(DEV), q.to(DEV), ve.to(DEV), None, 4)
    torch.cuda.synchronize()
    assert len(a) == len(b) == 4 and a[0].shape == (1, 8, 80, 77) and a[1].shape == (1, 8, 20, 128) and a[3].shape == (1, 8, 100, 128)
    for x, y in zip(a, b):
        assert torch.equal(_bytes(x.cpu()), _bytes(y.cpu()))


# ------------------------------------------------------------------------------------------------ 7. determinism
def test_two_calls_give_the_same_bytes(P):
    q, kc = _gauss(2, 4, 64, 300, 128, "bf16", 77)
    a, b = _run(P, q, kc, 32, 51), _run(P, q, kc, 32, 51)
    for x, y in zip(a, b):
        assert torch.equal(_bytes(x), _bytes(y))


# ------------------------------------------------------------------------------------------------ 8. fixtures, end to end
@pytest.mark.parametrize("name", T.fixture_files())
def test_fixtures_end_to_end(P, name):
    meta, t = T.load_fixture(name)
    if "_pruner_" in name:                                   # key_pruner_query_driven alone
        q, kc = t["q"], t["kc"]
        kp, keep, kidx, st = _run(P, q, kc, meta["recent"], meta["n_prune"])
        assert torch.equal(_bytes(st[:, :, 2]), _bytes(T.scores(q, kc)[2])), "scaled grid: the score has one value"
        T.compare_with_reference(st[:, :, 2], meta["n_prune"], kc, meta["recent"], (kp, keep), (t["k_pruned"], t["keep"]))
        return
    q, k, v = t["q"].to(DEV), t["k"].to(DEV), t["v"].to(DEV)
    cl = P.SnapKVCluster(window_size=meta["window"], max_capacity_prompt=meta["cap"], kernel_size=meta["kernel_size"],
                         pooling=meta["pooling"], merge=meta.get("merge"), recent_size=meta["recent"], ratio=meta["ratio"])
    out = cl.update_think(k, q, v, None, 1)
    torch.cuda.synchronize()
    assert len(out) == meta["n_out"]
    if meta.get("passthrough"):
        assert out[0] is k and out[1] is v                   # the input objects
        return
    if meta.get("merge"):                                    # what update_kv returns with merge set: the merge result
        ko, vo = cl.update_kv(k, q, v, None, 1)
        assert out[0].shape == t["out0"].shape and torch.equal(_bytes(out[0].cpu()), _bytes(ko.cpu())) and torch.equal(_bytes(out[1].cpu()), _bytes(vo.cpu()))
        return
    kp, kr, keep, vc = (x.cpu() for x in out)
    assert torch.equal(_bytes(vc), _bytes(t["out3"])), "V_c differs from the reference's"
    assert torch.equal(_bytes(kr), _bytes(t["out1"])), "the recent keys differ from the reference's"
    kc = cl.update_kv(k, q, v, None, 1)[0].cpu()             # the compacted keys the pruner saw (K_c of the same call)
    score = T.scores(t["q"], kc)[2]
    T.compare_with_reference(score, meta["n_prune"], kc, meta["recent"], (kp, keep), (t["out0"], t["out2"]))


# ------------------------------------------------------------------------------------------------ 9. adapter
def test_replace_llama_think_prefill_and_decode(P):
    """replace_llama("think") on a 2-layer random Llama: prefill + 3 decode steps against the same forward driven by the
    restatement on the CPU copy; restore() undoes it."""
    pytest.importorskip("transformers")
    from transformers import LlamaConfig, LlamaForCausalLM
    from pyramidkv_amd import monkeypatch as mp
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=97, hidden_size=512, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=128, max_position_embeddings=4096)
    cpu_model = LlamaForCausalLM(cfg).eval()
    gpu_model = LlamaForCausalLM(cfg).eval()
    gpu_model.load_state_dict(cpu_model.state_dict())
    gpu_model = gpu_model.to(DEV)
    S, cap, window, recent = 200, 64, 16, 12
    ids = torch.randint(0, 97, (1, S), generator=torch.Generator().manual_seed(1))
    original = type(cpu_model.model.layers[0].self_attn).forward

    class _RefCluster:
        accepts_unexpanded_kv = True

        def update_think(self, k, q, v, mask, groups):
            g = q.shape[1] // k.shape[1]
            return T.update_think(k.repeat_interleave(g, 1), q, v.repeat_interleave(g, 1), window, cap, 5, "avgpool", recent, 0.4)

    def drive(model, ids_dev, cluster_module):
        saved = mp._cluster_module
        if cluster_module is not None:
            mp._cluster_module = cluster_module
        try:
            for layer in model.model.layers:
                c = layer.self_attn.config
                c.window_size, c.max_capacity_prompt, c.kernel_size, c.pooling, c.recent_size, c.ratio = window, cap, 5, "avgpool", recent, 0.4
                if hasattr(layer.self_attn, "kv_cluster"):
                    del layer.self_attn.kv_cluster
            cache = P.ThinKCache()
            logits = []
            with torch.no_grad():
                o = model(ids_dev, past_key_values=cache, use_cache=True)
                logits.append(o.logits[:, -1].float().cpu())
                for step in range(3):                        # the same three tokens on both sides
                    tok = torch.full((1, 1), 11 + step, dtype=torch.long, device=ids_dev.device)
                    o = model(tok, past_key_values=cache, use_cache=True)
                    logits.append(o.logits[:, -1].float().cpu())
            return logits, cache
        finally:
            mp._cluster_module = saved

    mp.replace_llama("think")
    try:
        ref_mod = types.SimpleNamespace(init_think_native=lambda self: setattr(self, "kv_cluster", _RefCluster()))
        want, _ = drive(cpu_model, ids, ref_mod)
        got, cache = drive(gpu_model, ids.to(DEV), None)
        assert isinstance(gpu_model.model.layers[0].self_attn.kv_cluster, P.SnapKVCluster)
        assert cache.key_cache_pruned[0].shape == (1, 4, cap - recent, 128 - 51) and cache.key_cache[0].shape == (1, 4, recent + 3, 128)
        for a, b in zip(got, want):
            assert torch.allclose(a, b, atol=1e-3, rtol=1e-3), float((a - b).abs().max())
    finally:
        mp.restore()
    assert type(cpu_model.model.layers[0].self_attn).forward is original
