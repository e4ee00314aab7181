"""Decode attention over the flat cache on CPU: the three symbols in header, binding and library; the argument checks of
pkv_decode_attn_flat (answered before any HIP call); the default split count; the dispatch of the flat forward; the float64
restatement (tests/decode_attn_ref.py) against varlen_decode_attention; the exact fixtures under three fp32 summation orders.
No kernel is launched here."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import decode_attn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pkv_decode_attn_splits", "pkv_decode_attn_workspace_bytes", "pkv_decode_attn_flat")
DTYPE, SHAPE, ALIGN, WORKSPACE, NULL = -1, -2, -3, -4, -7


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pyramidkv_amd", "libpkv.so")):
        g.build()
    import pyramidkv_amd
    return pyramidkv_amd


# ------------------------------------------------------------------------------------------------ ABI (no launch)
def test_symbols_declared_bound_and_exported(P):
    N = P._native
    hdr = open(os.path.join(ROOT, "include", "pkv.h")).read()
    for name in NAMES:
        assert re.search(r"PKV_API \w+ " + name + r"\(", hdr) and name in N.EXPORTED and hasattr(N.lib, name)
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pyramidkv_amd", "libpkv.so")], capture_output=True, text=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert set(NAMES) <= exported
    assert N.lib.pkv_version() == N.PKV_VERSION == 204 and "PKV_K_COUNT = 9" in hdr and len(N.KERNEL_NAMES) == 9
    assert R.chunk_rows() == N.PKV_DECODE_CHUNK and R.chunk_rows() in (128, 256)
    assert int(re.search(r"#define PKV_DECODE_MAX_SPLITS (\d+)", hdr).group(1)) == N.PKV_DECODE_MAX_SPLITS


def test_status_of_every_bad_argument(P):
    N = P._native
    call = lambda dt=0, H=4, D=128, q=16, qs=128, k=16, v=16, cu=16, mx=300, scale=0.1, sp=1, out=16, lse=None, ws=None, nb=0: \
        N.lib.pkv_decode_attn_flat(dt, H, D, q, qs, k, v, cu, mx, scale, sp, out, lse, ws, nb, None)   # noqa: E731
    for dt in (-1, 3, 7):
        assert call(dt=dt) == DTYPE
    for bad in (dict(H=0), dict(H=-3), dict(D=0), dict(D=96), dict(D=512), dict(mx=0), dict(mx=-1), dict(sp=-1),
                dict(sp=N.PKV_DECODE_MAX_SPLITS + 1), dict(scale=math.inf), dict(scale=-math.inf), dict(scale=math.nan), dict(qs=64)):
        assert call(**bad) == SHAPE, bad
    for bad in (dict(q=None), dict(k=None), dict(v=None), dict(cu=None), dict(out=None), dict(sp=2, ws=None, nb=1 << 20)):
        assert call(**bad) == NULL, bad
    for bad in (dict(q=8), dict(k=24), dict(v=2), dict(out=4), dict(qs=132), dict(cu=2), dict(lse=6), dict(sp=2, ws=8, nb=1 << 20)):
        assert call(**bad) == ALIGN, bad
    assert call(dt=2, qs=130) == ALIGN and call(dt=2, D=64, qs=68, sp=2, ws=16, nb=0) == WORKSPACE      # fp32 rows: 4 elements = 16 bytes
    # the workspace: nothing for one split, (max, sum) + an fp32 accumulator per (head, split) otherwise
    nb = N.lib.pkv_decode_attn_workspace_bytes(4, 128, 3)
    assert nb >= 4 * 3 * (128 + 2) * 4 and nb % 256 == 0
    assert call(sp=3, ws=16, nb=nb - 1) == WORKSPACE and call(sp=3, ws=16, nb=0) == WORKSPACE
    # the default route asks for the workspace of the default split count
    sp = N.lib.pkv_decode_attn_splits(4, 128, 300)
    assert sp == 3 and call(sp=0, ws=16, nb=nb - 1) == WORKSPACE and call(sp=0, ws=None, nb=nb) == NULL
    # a defect of higher rank wins: dtype before shape before null before alignment before workspace
    assert call(dt=9, D=96, q=None) == DTYPE and call(D=96, q=None) == SHAPE and call(q=None, k=24) == NULL
    assert call(k=24, sp=2, ws=16, nb=0) == ALIGN


def test_default_splits_and_workspace(P):
    N = P._native
    C, S = N.PKV_DECODE_CHUNK, N.lib.pkv_decode_attn_splits
    for H in (1, 4, 5, 32, 40, 128, 4096):
        for D in (64, 128, 256):
            prev = 0
            for mx in sorted((1, 2, C - 1, C, C + 1, 2 * C, 3 * C + 5, 17 * C, 2048, 13443, 1 << 20, (1 << 31) - 1)):
                s = S(H, D, mx)
                assert 1 <= s <= N.PKV_DECODE_MAX_SPLITS and s >= prev, (H, D, mx, s, prev)
                assert s <= (mx + C - 1) // C, "never more splits than the longest head has chunks"
                prev = s
            for sp in (1, 2, prev):
                nb = N.lib.pkv_decode_attn_workspace_bytes(H, D, sp)
                assert (nb == 0) == (sp == 1)
    assert S(32, 128, 128) == 1 and S(32, 128, 2048) == 16 and S(32, 128, 13443) == 32      # the shapes of tools/decode_attn_bench.py
    assert S(0, 128, 100) == 0 and S(4, 0, 100) == 0 and S(4, 128, 0) == 0 and S(-1, 128, 100) == 0
    W = N.lib.pkv_decode_attn_workspace_bytes
    assert W(0, 128, 2) == 0 and W(4, 0, 2) == 0 and W(4, 128, 0) == 0 and W(4, 128, N.PKV_DECODE_MAX_SPLITS + 1) == 0


def test_wrapper_needs_hip_tensors_and_int32_metadata(P):
    q, k, cu = torch.zeros(2, 64), torch.zeros(6, 64), torch.tensor([0, 3, 6], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        P.ops.decode_attn_flat(q, k, k, cu, 3, 0.125)


# ------------------------------------------------------------------------------------------------ the flat forward's dispatch
@pytest.fixture
def patched():
    pytest.importorskip("transformers")
    from pyramidkv_amd import monkeypatch as mp
    saved = mp._cluster_module, mp.native_decode_attention, mp._is_hip
    yield mp
    mp._cluster_module, mp.native_decode_attention, mp._is_hip = saved
    mp.restore()


@pytest.mark.parametrize("method", ["adakv", "headkv"])
def test_flat_forward_dispatch(P, patched, monkeypatch, method):
    """HIP tensors (faked) go through ops.decode_attn_flat with the post-increment metadata; CPU tensors, or the switch set
    to False, run varlen_decode_attention - on the same arguments."""
    from oracle import pkv_oracle as O
    from test_monkeypatch_plumbing import _flat_module, _tiny
    mp = patched
    model = _tiny("llama")
    S, cap, w = 120, 48, 8
    ids = torch.randint(0, 97, (1, S), generator=torch.Generator().manual_seed(1))
    mp._cluster_module = _flat_module()
    mp.replace_llama(method)
    Lyr, H = model.config.num_hidden_layers, model.config.num_attention_heads
    for layer in model.model.layers:
        c = layer.self_attn.config
        c.window_size, c.max_capacity_prompt, c.kernel_size, c.pooling, c.merge = w, cap, 7, "maxpool", None
        c.floor, c.normalize = 0.2, True
        c.head_capacity = torch.tensor([[30, 50]] * Lyr, dtype=torch.int32)
    monkeypatch.setattr(P.DynamicCacheSplitHeadFlatten, "_append", staticmethod(O.update_flatten_view))
    native, eager = [], []
    real_eager = mp.varlen_decode_attention

    def stub(q, kf, vf, cu_klen, max_seqlen_k, scaling):
        native.append((tuple(q.shape), kf.shape[0], cu_klen.clone(), int(max_seqlen_k), float(scaling)))
        return real_eager(q, kf, vf, cu_klen, max_seqlen_k, scaling)

    def spy(q, kf, vf, cu_klen, max_seqlen_k, scaling):
        eager.append((tuple(q.shape), kf.shape[0], cu_klen.clone(), int(max_seqlen_k), float(scaling)))
        return real_eager(q, kf, vf, cu_klen, max_seqlen_k, scaling)

    monkeypatch.setattr(P.ops, "decode_attn_flat", stub)
    monkeypatch.setattr(mp, "varlen_decode_attention", spy)
    try:
        cache = P.DynamicCacheSplitHeadFlatten()
        with torch.no_grad():
            out = model(ids, past_key_values=cache, use_cache=True)
            assert native == [] and eager == []                           # prefill attends to the full K/V
            cls = [l.self_attn.kv_cluster for l in model.model.layers]
            before = [(c.cu_klen.clone(), int(c.max_seqlen_k), int(c.klen_sum)) for c in cls]
            nxt = out.logits[:, -1:].argmax(-1)
            # 1. CPU tensors, switch on: the eager function
            assert mp.native_decode_attention is True
            o1 = model(nxt, past_key_values=cache, use_cache=True).logits
            assert native == [] and len(eager) == Lyr
            # 2. tensors taken for HIP tensors: the native wrapper, with the post-increment cu_klen / max_seqlen_k
            mp._is_hip = lambda t: True
            model(nxt, past_key_values=cache, use_cache=True)
            assert len(native) == Lyr and len(eager) == Lyr
            for (shape, rows, cu, mx, sc), (cu0, mx0, sum0) in zip(native, before):
                assert shape == (H, 128) and sc == pytest.approx(128 ** -0.5)
                assert torch.equal(cu, cu0 + 2 * torch.arange(H + 1, dtype=torch.int32)) and mx == mx0 + 2
                assert rows == sum0 + 2 * H == int(cu[-1])
            # 3. the switch off: the eager function even for them
            mp.native_decode_attention = False
            model(nxt, past_key_values=cache, use_cache=True)
            assert len(native) == Lyr and len(eager) == 2 * Lyr
            assert torch.equal(eager[-1][2], before[-1][0] + 3 * torch.arange(H + 1, dtype=torch.int32))
        assert torch.isfinite(o1).all()
    finally:
        for layer in model.model.layers:
            if hasattr(layer.self_attn, "kv_cluster"):
                del layer.self_attn.kv_cluster


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_agrees_with_the_eager_function():
    """The shapes of test_varlen_decode_attention_matches_per_head_loop, and one with skewed lengths."""
    from pyramidkv_amd.monkeypatch import varlen_decode_attention
    for lens, D, seed in (([5, 1, 17, 9], 16, 0), ([300, 2, 41], 64, 3)):
        g = torch.Generator().manual_seed(seed)
        cu = R.cu_of(lens)
        q = torch.randn(len(lens), D, generator=g)
        kf, vf = torch.randn(sum(lens), D, generator=g), torch.randn(sum(lens), D, generator=g)
        got = varlen_decode_attention(q, kf, vf, cu, max(lens), 0.25)
        ref, lse = R.ref_f64(q, kf, vf, cu, 0.25)
        assert torch.allclose(got.double(), ref, atol=1e-6, rtol=0)
        for h, n in enumerate(lens):
            a = int(cu[h])
            s = (kf[a:a + n].double() @ q[h].double()) * 0.25
            assert float(lse[h]) == pytest.approx(float(torch.logsumexp(s, 0)), abs=1e-12)
        E = R.eager_fp32_deviation(varlen_decode_attention, q, kf, vf, cu, max(lens), 0.25, ref)
        assert E.shape == (len(lens),) and float(E.max()) < 1e-6 and bool((R.out_bar(torch.float32, ref, E) > 0).all())
    ref, lse = R.ref_f64(q, kf, vf, torch.tensor([0, 0, 343, 343], dtype=torch.int32), 0.25)        # heads without rows
    assert not ref[0].any() and not ref[2].any() and lse[0] == -math.inf and lse[2] == -math.inf and torch.isfinite(ref).all()


def test_ulp_is_the_spacing_of_the_dtype():
    for dt in R.DTYPES.values():
        x = torch.tensor([1.0, 1.5, 2.0, 3.99, 0.3, 1e-3, 100.0], dtype=torch.float64)
        u = R.ulp(dt, x)
        assert u.tolist() == [2.0 ** (math.floor(math.log2(v)) - R._FMT[dt][0]) for v in x.tolist()]
        y = x.to(dt)                                             # the next value up is one spacing away
        assert torch.equal(R.ulp(dt, y.double()), torch.nextafter(y, torch.tensor(math.inf, dtype=dt)).double() - y.double())
    assert float(R.ulp(torch.float16, torch.tensor([0.0], dtype=torch.float64))) == 2.0 ** -24          # subnormal spacing


# ------------------------------------------------------------------------------------------------ the exact fixtures
def _lens_sets(C):
    return [1, 2, C - 1, C, C + 1], [3 * C + 5, 1, 2 * C, C + 1, 7]


@pytest.mark.parametrize("D", [64, 128, 256])
def test_onehot_fixture_has_one_answer_in_every_summation_order(D):
    C = R.chunk_rows()
    for dtype in R.DTYPES.values():
        for lens in _lens_sets(C):
            for plant in R.plants(lens, C) if dtype == torch.bfloat16 else R.plants(lens, C)[-1:]:
                q, k, v, cu, want, want_lse = R.onehot_fixture(lens, D, dtype, plant)
                assert torch.equal(v.double().to(dtype), v) and len({tuple(r.tolist()) for r in v[:, :3]}) == v.shape[0], "distinct rows"
                for order, kw in (("forward", {}), ("reversed", {}), ("chunked", dict(chunk=C, splits=1)), ("chunked", dict(chunk=C, splits=3))):
                    out, lse = R.attend_f32(q, k, v, cu, D ** -0.5, order, **kw)
                    assert torch.equal(out.to(dtype).view(torch.uint8), want.view(torch.uint8)), (D, dtype, lens, plant, order)
                    assert torch.equal(lse, want_lse)


@pytest.mark.parametrize("D", [64, 128, 256])
def test_uniform_fixture_has_one_answer_in_every_summation_order(D):
    C = R.chunk_rows()
    lens = [1, 2, C, 2 * C, 4 * C]
    for dtype in R.DTYPES.values():
        q, k, v, cu, want, want_lse = R.uniform_fixture(lens, D, dtype)
        for order, kw in (("forward", {}), ("reversed", {}), ("chunked", dict(chunk=C, splits=2)), ("chunked", dict(chunk=C, splits=3))):
            out, lse = R.attend_f32(q, k, v, cu, D ** -0.5, order, **kw)
            assert torch.equal(out.to(dtype).view(torch.uint8), want.view(torch.uint8)), (D, dtype, order)
            assert np.all(np.abs(lse.double().numpy() - want_lse.numpy()) <= R.ulp(torch.float32, want_lse).numpy())
    assert float(want_lse[0]) == 0.0
