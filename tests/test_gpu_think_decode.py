"""Decode attention over the ThinK cache on the GPU (pkv_decode_attn_think, ops.decode_attn_think, the decode branch of
replace_llama("think")).  Masks, fixtures, the float64 restatement and the error bar live in tests/think_decode_ref.py;
tests/test_think_decode_cpu.py shows that the exact fixtures have one answer in every fp32 summation order.

Gaussian inputs, every element of every head: |out - ref| <= ulp_dtype(|ref|) + 4 E with E the eager function's own fp32
deviation in that head, measured on the device in the same test (figures: profiles/think_decode/error.json)."""
import math

import pytest
import torch

import think_decode_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = R.chunk_rows()
H = 5
SHAPES = R.shapes(C)
SPLITS = (1, 2, 3, None)
CASES = [(dt, D) for dt in ("bf16", "fp16", "fp32") for D in (64, 128, 256)]


@pytest.fixture(scope="module")
def P():
    import pyramidkv_amd
    return pyramidkv_amd


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b):
    return torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


def _padded(t, filler=7.0):
    """The same heads, twice the head stride; what lies between them is not zero."""
    buf = torch.full((t.shape[0], 2) + tuple(t.shape[1:]), filler, dtype=t.dtype, device=t.device)
    buf[:, 0] = t
    return buf[:, 0]


def _run(P, q, keep, kp, kf, v, scale, splits, strided=False):
    """Tensors already on the device.  -> (out, lse) on the CPU."""
    if strided:
        q, kf, v = _padded(q), _padded(kf), _padded(v)
    out, lse = P.ops.decode_attn_think(q, keep, kp, kf, v, scale, splits=splits, return_lse=True)
    torch.cuda.synchronize()
    return out.cpu(), lse.cpu()


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


# ------------------------------------------------------------------------------------------------ exact fixtures
@pytest.mark.parametrize("dtype,D", CASES)
def test_onehot_rows_come_back_bit_exact(P, dtype, D):
    """A wrong channel map, a row walked at the wrong width, a misaligned head base (R = 3, Dk = 77: 462-byte heads) and every
    chunk / split boundary of either part: the planted V row, bit for bit, and the planted score as lse."""
    dt = R.DTYPES[dtype]
    for Dk in R.kept_widths(D):
        keep = R.masks(H, D, Dk)
        keepd = keep.to(DEV)
        for Rn, Tn in SHAPES:
            for row in R.plant_rows(Rn, Tn, C):
                q, kp, kf, v, want, want_lse = R.onehot_fixture(H, Rn, Tn, D, keep, dt, row)
                qd, kpd, kfd, vd = _dev(q, kp, kf, v)
                for sp in SPLITS:
                    out, lse = _run(P, qd, keepd, kpd, kfd, vd, D ** -0.5, sp, strided=sp == 2)
                    assert torch.equal(_bits(out), _bits(want)), (Dk, Rn, Tn, row, sp)
                    assert torch.equal(lse, want_lse), (Dk, Rn, Tn, row, sp)


@pytest.mark.parametrize("dtype,D", CASES)
def test_uniform_weights_give_the_exact_mean(P, dtype, D):
    dt = R.DTYPES[dtype]
    for Dk in R.kept_widths(D):
        for Rn, Tn in ((0, 1), (1, 1), (C - 1, 1), (2 * C - 2, 2), (3 * C, C)):
            q, keep, kp, kf, v, want, want_lse = R.uniform_fixture(H, Rn, Tn, D, Dk, dt)
            qd, keepd, kpd, kfd, vd = _dev(q, keep, kp, kf, v)
            for sp in SPLITS + (4, 5):
                out, lse = _run(P, qd, keepd, kpd, kfd, vd, D ** -0.5, sp)
                assert torch.equal(_bits(out), _bits(want)), (Dk, Rn, Tn, sp)
                assert bool(((lse.double() - want_lse).abs() <= R.ulp(torch.float32, want_lse)).all()), (Dk, Rn, Tn, sp, lse.tolist())
                assert Rn + Tn > 1 or float(lse[0]) == 0.0


# ------------------------------------------------------------------------------------------------ what must not enter the result
@pytest.mark.parametrize("dtype,D", CASES)
def test_dropped_channels_stay_out(P, dtype, D):
    """q is huge on the dropped channels and zero on the kept ones; the full-width rows are zero in the dropped channels.  The
    result is that of the same call with those q entries zeroed (uniform weights over Gaussian V, whatever the pruned keys hold)."""
    dt = R.DTYPES[dtype]
    for Dk in R.kept_widths(D)[:3]:
        for Rn, Tn in ((3, 2), (C + 1, 2), (3 * C + 5, C)):
            q, keep, kp, kf, v = R.gauss(H, Rn, Tn, D, Dk, dt, 31 * D + Dk)
            q = torch.where(keep, torch.zeros((), dtype=dt), torch.full((), 3e4, dtype=dt))
            kf = torch.where(keep[:, None, :], kf, torch.zeros((), dtype=dt))
            qd, keepd, kpd, kfd, vd = _dev(q, keep, kp, kf, v)
            zero = torch.zeros_like(qd)
            for sp in SPLITS:
                a, b = _run(P, qd, keepd, kpd, kfd, vd, D ** -0.5, sp), _run(P, zero, keepd, kpd, kfd, vd, D ** -0.5, sp)
                assert _same(a, b) and bool(torch.isfinite(a[0].float()).all()), (Dk, Rn, Tn, sp)
                assert float(a[1][0]) == pytest.approx(math.log(Rn + Tn), abs=1e-5)


@pytest.mark.parametrize("dtype,D", CASES)
def test_neighbours_of_the_pruned_keys_do_not_leak(P, dtype, D):
    """k_pruned inside a larger 16-byte aligned buffer that is NaN before and behind it: the enclosing 16-byte blocks are read,
    what they hold beyond the tensor does not reach the result."""
    dt = R.DTYPES[dtype]
    es = torch.empty((), dtype=dt).element_size()
    for Dk in R.kept_widths(D)[:3]:
        for Rn, Tn in ((1, 1), (3, 2), (C + 1, 2)):
            qd, keepd, kpd, kfd, vd = _dev(*R.gauss(H, Rn, Tn, D, Dk, dt, 57 * D + Dk + Rn))
            n = H * Rn * Dk
            front = 16 // es * 4
            buf = torch.full((front + n + 64,), math.nan, dtype=dt, device=DEV)
            inner = buf[front:front + n].view(H, Rn, Dk)
            inner.copy_(kpd)
            assert inner.data_ptr() % 16 == 0 and inner.is_contiguous()
            for sp in (1, 2, None):
                a, b = _run(P, qd, keepd, kpd, kfd, vd, D ** -0.5, sp), _run(P, qd, keepd, inner, kfd, vd, D ** -0.5, sp)
                assert _same(a, b) and not torch.isnan(b[0].float()).any(), (Dk, Rn, Tn, sp)


@pytest.mark.parametrize("dtype,D", CASES)
def test_mask_content_is_free(P, dtype, D):
    """The library does not count the mask: with more than Dk ones the first Dk are used, with fewer the missing ones meet a zero
    query - the result of the call whose pruned keys carry zeros in those columns.  An all-zero and an all-255 mask run too."""
    dt = R.DTYPES[dtype]
    Dk, Rn, Tn = R.kept_widths(D)[1], C + 3, 2
    q, keep, kp, kf, v = R.gauss(H, Rn, Tn, D, Dk, dt, 11 * D)
    qd, keepd, kpd, kfd, vd = _dev(q, keep, kp, kf, v)
    base = _run(P, qd, keepd, kpd, kfd, vd, D ** -0.5, 1)
    more = keep.clone()
    more[:, -1] = True                                           # heads whose last channel was dropped now have Dk + 1 ones
    assert _same(base, _run(P, qd, more.to(DEV), kpd, kfd, vd, D ** -0.5, 1))
    fewer, kz = keep.clone(), kp.clone()
    idx = R.keep_index(keep)
    for h in range(H):
        fewer[h, idx[h, -3:]] = False                            # the last three kept channels go: columns Dk-3 .. Dk-1 meet zeros
    kz[:, :, -3:] = 0
    assert _same(_run(P, qd, fewer.to(DEV), kpd, kfd, vd, D ** -0.5, 1), _run(P, qd, keepd, kz.to(DEV), kfd, vd, D ** -0.5, 1))
    for fill in (0, 255):
        out, lse = _run(P, qd, torch.full((H, D), fill, dtype=torch.uint8, device=DEV), kpd, kfd, vd, D ** -0.5, None)
        assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all())


# ------------------------------------------------------------------------------------------------ memory safety
@pytest.mark.parametrize("dtype,D", CASES)
def test_nothing_outside_out_lse_and_workspace_is_written(P, dtype, D):
    N = P._native
    dt = R.DTYPES[dtype]
    Dk, Rn, Tn = R.kept_widths(D)[1], 3 * C + 5, C
    q, keep, kp, kf, v = _dev(*R.gauss(H, Rn, Tn, D, Dk, dt, 3 * D + 1))
    es = q.element_size()
    for sp in (1, 3):
        nb = N.lib.pkv_decode_attn_workspace_bytes(H, D, sp)
        pad = 256
        outb = torch.full((H * D * es + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
        lseb = torch.full((H * 4 + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
        wsb = torch.full((nb + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
        assert outb.data_ptr() % 16 == 0 and wsb.data_ptr() % 16 == 0
        ins = [t.clone() for t in (q, kp, kf, v)] + [keep.clone()]
        rc = N.lib.pkv_decode_attn_think(N.dtype_code(dt), H, D, Dk, q.data_ptr(), D, keep.data_ptr(), kp.data_ptr(), Rn, kf.data_ptr(), Tn * D, Tn,
                                         v.data_ptr(), (Rn + Tn) * D, D ** -0.5, sp, outb.data_ptr() + pad, lseb.data_ptr() + pad,
                                         wsb.data_ptr() + pad if nb else None, nb, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        for buf, n in ((outb, H * D * es), (lseb, H * 4), (wsb, nb)):
            b = buf.cpu()
            assert bool((b[:pad] == 0xA5).all()) and bool((b[pad + n:] == 0xA5).all()), (sp, n)
        for a, b in zip(ins, (q, kp, kf, v, keep)):
            assert torch.equal(_bits(a), _bits(b))
        out, lse = _run(P, q, keep, kp, kf, v, D ** -0.5, sp)
        assert torch.equal(outb.cpu()[pad:pad + H * D * es], _bits(out).flatten())
        assert torch.equal(lseb.cpu()[pad:pad + H * 4], _bits(lse).flatten())


# ------------------------------------------------------------------------------------------------ repeat, strides, no rows
@pytest.mark.parametrize("dtype,D", CASES)
def test_two_calls_and_padded_head_strides_give_the_same_bits(P, dtype, D):
    dt = R.DTYPES[dtype]
    for Dk in R.kept_widths(D):
        for i, (Rn, Tn) in enumerate(SHAPES):
            t = _dev(*R.gauss(H, Rn, Tn, D, Dk, dt, 100 * D + i))
            for sp in SPLITS:
                a = _run(P, *t, D ** -0.5, sp)
                assert _same(a, _run(P, *t, D ** -0.5, sp)) and _same(a, _run(P, *t, D ** -0.5, sp, strided=True)), (Dk, Rn, Tn, sp)
            named = P._native.lib.pkv_decode_attn_splits(H, D, Rn + Tn)                          # the default route, named
            assert 1 <= named <= (Rn + C - 1) // C + (Tn + C - 1) // C and _same(a, _run(P, *t, D ** -0.5, named))


@pytest.mark.parametrize("dtype,D", CASES)
def test_no_rows_give_zeros_and_minus_infinity(P, dtype, D):
    dt = R.DTYPES[dtype]
    for Dk in (R.kept_widths(D)[1], D):
        t = _dev(*R.gauss(H, 0, 0, D, Dk, dt, 5))
        for sp in SPLITS:
            out, lse = _run(P, *t, D ** -0.5, sp)
            assert not _bits(out).any() and bool((lse == -math.inf).all()), (Dk, sp)


# ------------------------------------------------------------------------------------------------ Gaussian inputs
@pytest.mark.parametrize("dtype,D", CASES)
def test_gaussian_inputs_within_rounding_plus_four_times_the_eager_deviation(P, dtype, D):
    """N(0,1) inputs, seeded; every element of every head.  Measured on the device (E = the eager function's largest fp32
    deviation in a head, dev = this kernel's, both against float64; worst ratio dev / bar over all heads, splits, widths and
    shapes): see profiles/think_decode/error.json and DESIGN.md section 3.13.

    Measured on an MI355X with a row's dot product summed in fp64 and rounded to fp32 once: dev / bar <= 0.4999 (bf16 / fp16) and
    <= 0.55 (fp32) for `out`, <= 0.99 for lse.  With fp32 FMA chains for the dot products the lse bar was missed in three cases,
    each in one head of the one- and two-row shapes, where lse is a score: up to 1.99 of the bar."""
    from pyramidkv_amd.monkeypatch import think_decode_attention
    dt = R.DTYPES[dtype]
    worst = dict(E=0.0, dev=0.0, ratio=0.0, lse_E=0.0, lse_dev=0.0, lse_ratio=0.0)
    failures = []
    for Dk in R.kept_widths(D):
        for i, (Rn, Tn) in enumerate(SHAPES):
            t = R.gauss(H, Rn, Tn, D, Dk, dt, 1000 * D + 17 * i + len(dtype))
            ref, ref_lse = R.ref_f64(*t, D ** -0.5)
            td = _dev(*t)
            E, E_lse = R.eager_fp32_deviation(think_decode_attention, *td, D ** -0.5, ref, ref_lse)
            bar, lse_bar = R.out_bar(dt, ref, E), R.lse_bar(ref_lse, E_lse)
            for sp in SPLITS:
                out, lse = _run(P, *td, D ** -0.5, sp, strided=sp == 3)
                dev, lse_dev = (out.double() - ref).abs(), (lse.double() - ref_lse).abs()
                for key, val in (("E", E.max()), ("dev", dev.max()), ("ratio", (dev / bar).max()), ("lse_E", E_lse.max()),
                                 ("lse_dev", lse_dev.max()), ("lse_ratio", (lse_dev / lse_bar).max())):
                    worst[key] = max(worst[key], float(val))
                if not bool((dev <= bar).all()) or not bool((lse_dev <= lse_bar).all()):
                    failures.append((Dk, Rn, Tn, sp, float((dev / bar).max()), float((lse_dev / lse_bar).max())))
    print(f"think_decode error {dtype} D={D}: " + " ".join(f"{k}={x:.3e}" for k, x in worst.items()))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_think_forward_native_decode_matches_the_eager_decode(P, dtype):
    """The 2-layer random Llama of test_gpu_think.py through replace_llama("think") with a ThinKCache: prefill + three decode
    steps on the same tokens, once with the native decode attention and once with the eager function, on the same GPU model.
    fp32: the logits agree within 1e-3, the tolerance of the existing adapter test.  bf16: the bound is measured here - twice the
    largest deviation of the native-off run's own logits from those of an fp32 copy of the model (same weights upcast, same
    tokens, native off): two bf16 evaluations of one step may differ by what each differs from the exact one.  The native run
    never enters think_decode_attention."""
    pytest.importorskip("transformers")
    from transformers import LlamaConfig, LlamaForCausalLM
    from pyramidkv_amd import monkeypatch as mp
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=97, hidden_size=512, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=128, max_position_embeddings=4096)
    dt = R.DTYPES[dtype]
    model32 = LlamaForCausalLM(cfg).eval()
    model = LlamaForCausalLM(cfg).eval()
    model.load_state_dict(model32.state_dict())
    model = model.to(dt).to(DEV)
    S, cap, window, recent = 200, 64, 16, 12
    ids = torch.randint(0, 97, (1, S), generator=torch.Generator().manual_seed(1)).to(DEV)
    calls = []
    real = mp.think_decode_attention

    def spy(*a):
        calls.append(1)
        return real(*a)

    def drive(m, native):
        mp.native_decode_attention = native
        for layer in m.model.layers:
            c = layer.self_attn.config
            c.window_size, c.max_capacity_prompt, c.kernel_size, c.pooling, c.recent_size, c.ratio = window, cap, 5, "avgpool", recent, 0.4
            if hasattr(layer.self_attn, "kv_cluster"):
                del layer.self_attn.kv_cluster
        cache = P.ThinKCache()
        logits = []
        with torch.no_grad():
            logits.append(m(ids, past_key_values=cache, use_cache=True).logits[:, -1].float().cpu())
            for step in range(3):
                tok = torch.full((1, 1), 11 + step, dtype=torch.long, device=DEV)
                logits.append(m(tok, past_key_values=cache, use_cache=True).logits[:, -1].float().cpu())
        return logits, cache

    saved = mp.native_decode_attention
    mp.replace_llama("think")
    mp.think_decode_attention = spy
    try:
        on, cache = drive(model, True)
        assert calls == [], "the native run stays out of the eager function"
        off, _ = drive(model, False)
        assert len(calls) == 3 * 2
        assert cache.key_cache_pruned[0].shape == (1, 4, cap - recent, 128 - 51) and cache.key_cache[0].shape == (1, 4, recent + 3, 128)
        if dtype == "fp32":
            tol = [1e-3] * 4
        else:
            exact, _ = drive(model32.to(DEV), False)
            tol = [2.0 * float((a - b).abs().max()) for a, b in zip(off, exact)]
    finally:
        mp.think_decode_attention = real
        mp.native_decode_attention = saved
        mp.restore()
    assert torch.equal(on[0], off[0])                            # the prefill does not depend on the switch
    for a, b, t in zip(on[1:], off[1:], tol[1:]):
        print(f"think e2e {dtype}: max |native - eager| = {float((a - b).abs().max()):.3e}, bound {t:.3e}")
        assert torch.isfinite(a).all() and float((a - b).abs().max()) <= t
