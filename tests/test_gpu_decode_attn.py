"""Decode attention over the flat var-len cache on the GPU (pkv_decode_attn_flat, ops.decode_attn_flat, the decode branch of
replace_llama("adakv" | "headkv")).  Fixtures, the float64 restatement and the error bar live in tests/decode_attn_ref.py;
tests/test_decode_attn_cpu.py shows that the exact fixtures have one answer in every fp32 summation order.

Gaussian inputs, every element of every head: |out - ref| <= ulp_dtype(|ref|) + 4 E with E the eager function's own fp32
deviation in that head, measured on the device in the same test (figures: profiles/decode_attn/error.json)."""
import math

import pytest
import torch

import decode_attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = R.chunk_rows()
LENS = ([1, 2, C - 1, C, C + 1], [3 * C + 5, 1, 2 * C, C + 1, 7])
SPLITS = (1, 2, 3, None)
CASES = [(dt, D) for dt in ("bf16", "fp16", "fp32") for D in (64, 128, 256)]


@pytest.fixture(scope="module")
def P():
    import pyramidkv_amd
    return pyramidkv_amd


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _strided(q):
    """The same rows with 2 D elements between heads; what lies between them is not zero."""
    H, D = q.shape
    buf = torch.full((H, 2 * D), 7.0, dtype=q.dtype, device=q.device)
    buf[:, :D] = q
    return buf[:, :D]


def _run(P, q, k, v, cu, mx, scale, splits, strided=False):
    """q, k, v, cu already on the device.  -> (out, lse) on the CPU."""
    out, lse = P.ops.decode_attn_flat(_strided(q) if strided else q, k, v, cu, mx, scale, splits=splits, return_lse=True)
    torch.cuda.synchronize()
    return out.cpu(), lse.cpu()


def _gauss(lens, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    n = int(sum(lens))
    return (torch.randn(len(lens), D, generator=g).to(dtype), torch.randn(n, D, generator=g).to(dtype),
            torch.randn(n, D, generator=g).to(dtype), R.cu_of(lens))


# ------------------------------------------------------------------------------------------------ exact fixtures
@pytest.mark.parametrize("dtype,D", CASES)
def test_onehot_rows_come_back_bit_exact(P, dtype, D):
    """Every cu_klen / chunk / split boundary and any read across a head: the planted V row, bit for bit."""
    dt = R.DTYPES[dtype]
    for lens in LENS:
        for plant in R.plants(lens, C):
            q, k, v, cu, want, want_lse = R.onehot_fixture(lens, D, dt, plant)
            qd, kd, vd, cud = (t.to(DEV) for t in (q, k, v, cu))
            for sp in SPLITS:
                for strided in (False, True):
                    out, lse = _run(P, qd, kd, vd, cud, max(lens), D ** -0.5, sp, strided)
                    assert torch.equal(_bits(out), _bits(want)), (lens, plant, sp, strided)
                    assert torch.equal(lse, want_lse), (lens, plant, sp, strided)


@pytest.mark.parametrize("dtype,D", CASES)
def test_uniform_weights_give_the_exact_mean(P, dtype, D):
    dt = R.DTYPES[dtype]
    lens = [1, 2, C, 2 * C, 4 * C]
    q, k, v, cu, want, want_lse = R.uniform_fixture(lens, D, dt)
    qd, kd, vd, cud = (t.to(DEV) for t in (q, k, v, cu))
    for sp in SPLITS + (4, 5):
        for strided in (False, True):
            out, lse = _run(P, qd, kd, vd, cud, max(lens), D ** -0.5, sp, strided)
            assert torch.equal(_bits(out), _bits(want)), (sp, strided)
            assert bool(((lse.double() - want_lse).abs() <= R.ulp(torch.float32, want_lse)).all()), (sp, lse.tolist())
            assert float(lse[0]) == 0.0


# ------------------------------------------------------------------------------------------------ hint, repeat, empty heads
@pytest.mark.parametrize("dtype,D", CASES)
def test_hint_does_not_change_the_bits_and_two_calls_agree(P, dtype, D):
    dt = R.DTYPES[dtype]
    for i, lens in enumerate(LENS):
        qd, kd, vd, cud = (t.to(DEV) for t in _gauss(lens, D, dt, 100 * D + i))
        for sp in (1, 2, 3):
            a = _run(P, qd, kd, vd, cud, max(lens), D ** -0.5, sp)
            b = _run(P, qd, kd, vd, cud, 1, D ** -0.5, sp)
            c = _run(P, qd, kd, vd, cud, max(lens), D ** -0.5, sp, strided=True)
            for x in (b, c):
                assert torch.equal(_bits(a[0]), _bits(x[0])) and torch.equal(_bits(a[1]), _bits(x[1])), (lens, sp)
        a, b = _run(P, qd, kd, vd, cud, max(lens), D ** -0.5, None), _run(P, qd, kd, vd, cud, max(lens), D ** -0.5, None)
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
        sp = P._native.lib.pkv_decode_attn_splits(len(lens), D, max(lens))
        c = _run(P, qd, kd, vd, cud, 1, D ** -0.5, sp)                       # the default route, named: the hint is not needed
        assert torch.equal(_bits(a[0]), _bits(c[0])) and torch.equal(_bits(a[1]), _bits(c[1]))


@pytest.mark.parametrize("dtype,D", CASES)
def test_head_without_rows_gets_zeros_and_minus_infinity(P, dtype, D):
    dt = R.DTYPES[dtype]
    lens = [0, 5, 0, C + 3, 0]
    q, k, v, cu = _gauss(lens, D, dt, 7 * D)
    qd, kd, vd, cud = (t.to(DEV) for t in (q, k, v, cu))
    full = [h for h, n in enumerate(lens) if n]
    cu2 = R.cu_of([lens[h] for h in full]).to(DEV)
    for sp in SPLITS:
        out, lse = _run(P, qd, kd, vd, cud, max(lens), D ** -0.5, sp)
        assert not torch.isnan(out.float()).any() and not torch.isnan(lse).any()
        for h, n in enumerate(lens):
            if n == 0:
                assert not _bits(out[h]).any() and float(lse[h]) == -math.inf
        # the other heads: the bits they get without the empty ones beside them
        o2, l2 = _run(P, qd[full].contiguous(), kd, vd, cu2, max(lens), D ** -0.5, sp if sp else P._native.lib.pkv_decode_attn_splits(5, D, max(lens)))
        assert torch.equal(_bits(out[full]), _bits(o2)) and torch.equal(lse[full], l2) and bool(torch.isfinite(l2).all())


# ------------------------------------------------------------------------------------------------ memory safety
@pytest.mark.parametrize("dtype,D", CASES)
def test_nothing_outside_out_lse_and_workspace_is_written(P, dtype, D):
    N = P._native
    dt = R.DTYPES[dtype]
    lens = LENS[1]
    H = len(lens)
    q, k, v, cu = (t.to(DEV) for t in _gauss(lens, D, dt, 3 * D + 1))
    es = q.element_size()
    for sp in (1, 3):
        nb = N.lib.pkv_decode_attn_workspace_bytes(H, D, sp)
        pad = 256
        outb = torch.full((H * D * es + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
        lseb = torch.full((H * 4 + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
        wsb = torch.full((nb + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
        assert outb.data_ptr() % 16 == 0 and wsb.data_ptr() % 16 == 0
        rc = N.lib.pkv_decode_attn_flat(N.dtype_code(dt), H, D, q.data_ptr(), D, k.data_ptr(), v.data_ptr(), cu.data_ptr(), max(lens),
                                        D ** -0.5, sp, outb.data_ptr() + pad, lseb.data_ptr() + pad, wsb.data_ptr() + pad if nb else None, nb,
                                        torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        for buf, n in ((outb, H * D * es), (lseb, H * 4), (wsb, nb)):
            b = buf.cpu()
            assert bool((b[:pad] == 0xA5).all()) and bool((b[pad + n:] == 0xA5).all()), (sp, n)
        out, lse = _run(P, q, k, v, cu, max(lens), D ** -0.5, sp)
        assert torch.equal(outb.cpu()[pad:pad + H * D * es], _bits(out).flatten())
        assert torch.equal(lseb.cpu()[pad:pad + H * 4], _bits(lse).flatten())


# ------------------------------------------------------------------------------------------------ Gaussian inputs
@pytest.mark.parametrize("dtype,D", CASES)
def test_gaussian_inputs_within_rounding_plus_four_times_the_eager_deviation(P, dtype, D):
    """N(0,1) inputs, seeded; every element of every head.  Measured on the device (E = the eager function's largest fp32
    deviation in a head, dev = this kernel's, both against float64; worst ratio dev / bar over all heads, splits and both
    length vectors): see profiles/decode_attn/error.json and DESIGN.md section 3.12."""
    from pyramidkv_amd.monkeypatch import varlen_decode_attention
    dt = R.DTYPES[dtype]
    worst = dict(E=0.0, dev=0.0, ratio=0.0, lse_E=0.0, lse_dev=0.0, lse_ratio=0.0)
    failures = []
    for i, lens in enumerate(LENS):
        q, k, v, cu = _gauss(lens, D, dt, 1000 * D + 17 * i + len(dtype))
        ref, ref_lse = R.ref_f64(q, k, v, cu, D ** -0.5)
        qd, kd, vd, cud = (t.to(DEV) for t in (q, k, v, cu))
        E = R.eager_fp32_deviation(lambda *a: varlen_decode_attention(*a).cpu(), qd, kd, vd, cud, max(lens), D ** -0.5, ref)
        E_lse = R.eager_fp32_lse_deviation(qd, kd, cu, D ** -0.5, ref_lse)
        bar, lse_bar = R.out_bar(dt, ref, E), R.lse_bar(ref_lse, E_lse)
        for sp in SPLITS:
            for strided in (False, True):
                out, lse = _run(P, qd, kd, vd, cud, max(lens), D ** -0.5, sp, strided)
                dev, lse_dev = (out.double() - ref).abs(), (lse.double() - ref_lse).abs()
                worst = dict(E=max(worst["E"], float(E.max())), dev=max(worst["dev"], float(dev.max())),
                             ratio=max(worst["ratio"], float((dev / bar).max())), lse_E=max(worst["lse_E"], float(E_lse.max())),
                             lse_dev=max(worst["lse_dev"], float(lse_dev.max())), lse_ratio=max(worst["lse_ratio"], float((lse_dev / lse_bar).max())))
                if not bool((dev <= bar).all()) or not bool((lse_dev <= lse_bar).all()):
                    failures.append((lens, sp, strided, float((dev / bar).max()), float((lse_dev / lse_bar).max())))
    print(f"decode_attn error {dtype} D={D}: " + " ".join(f"{k}={x:.3e}" for k, x in worst.items()))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("method", ["adakv", "headkv"])
def test_flat_forward_native_decode_matches_the_eager_decode(P, method):
    """A tiny random fp32 Llama through replace_llama(method) with a DynamicCacheSplitHeadFlatten, three decode steps, once
    with the native decode attention and once with the eager function on the same tokens."""
    pytest.importorskip("transformers")
    from transformers import LlamaConfig, LlamaForCausalLM
    from pyramidkv_amd import monkeypatch as mp
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=97, hidden_size=512, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=128, max_position_embeddings=8192)
    model = LlamaForCausalLM(cfg).to(DEV).eval()
    S, cap, w = 600, 160, 8
    ids = torch.randint(0, 97, (1, S), generator=torch.Generator().manual_seed(1)).to(DEV)
    saved = mp.native_decode_attention
    runs = {}
    try:
        mp.replace_llama(method)
        for layer in model.model.layers:
            c = layer.self_attn.config
            c.window_size, c.max_capacity_prompt, c.kernel_size, c.pooling, c.merge = w, cap, 7, "maxpool", None
            c.floor, c.normalize = 0.2, True
            c.head_capacity = torch.tensor([[30, 270, 156, 120]] * 2, dtype=torch.int32)
        toks = None
        for native in (True, False):
            mp.native_decode_attention = native
            for layer in model.model.layers:
                if hasattr(layer.self_attn, "kv_cluster"):
                    del layer.self_attn.kv_cluster
            cache = P.DynamicCacheSplitHeadFlatten()
            with torch.no_grad():
                out = model(ids, past_key_values=cache, use_cache=True)
                feed = [out.logits[:, -1:].argmax(-1)] if toks is None else toks
                logits = []
                for t in range(3):
                    o = model(feed[t], past_key_values=cache, use_cache=True)
                    logits.append(o.logits.float().cpu())
                    if toks is None:
                        feed.append(o.logits[:, -1:].argmax(-1))
            toks = feed
            cls = [l.self_attn.kv_cluster for l in model.model.layers]
            runs[native] = dict(logits=logits, prefill=out.logits.float().cpu(), rows=[cache.key_cache[i].shape[0] for i in range(2)],
                                seen=cache.get_seq_length(), head_lens=[c.head_lens.cpu() for c in cls], cu=[c.cu_klen.cpu() for c in cls],
                                mx=[int(c.max_seqlen_k) for c in cls], total=[int(c.klen_sum) for c in cls],
                                k=[cache.key_cache[i].cpu() for i in range(2)])
    finally:
        mp.native_decode_attention = saved
        mp.restore()
        for layer in model.model.layers:
            if hasattr(layer.self_attn, "kv_cluster"):
                del layer.self_attn.kv_cluster
    a, b = runs[True], runs[False]
    assert torch.equal(a["prefill"], b["prefill"])
    for x, y in zip(a["logits"], b["logits"]):
        assert torch.isfinite(x).all() and torch.allclose(x, y, atol=1e-4, rtol=1e-4), float((x - y).abs().max())
    assert a["rows"] == b["rows"] and a["seen"] == b["seen"] == S + 3 and a["mx"] == b["mx"] and a["total"] == b["total"]
    assert a["rows"] == a["total"] and all(m > C for m in a["mx"]), "some head is longer than one chunk"
    for i in range(2):
        assert torch.equal(a["head_lens"][i], b["head_lens"][i]) and torch.equal(a["cu"][i], b["cu"][i])
    assert torch.equal(a["k"][0], b["k"][0])                                 # layer 0's cache does not depend on the attention
