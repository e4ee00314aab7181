"""Decode attention over the ThinK cache on CPU: the symbol in header, binding and library; the argument checks of
pkv_decode_attn_think (answered before any HIP call - every call below carries a defect, none reaches a launch); the wrapper's
own checks; the dispatch of the ThinK forward; the float64 restatement (tests/think_decode_ref.py) against
think_decode_attention; the exact fixtures under three fp32 summation orders.  No kernel is launched here."""
import math
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import think_decode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pkv_decode_attn_think"
DTYPE, SHAPE, ALIGN, WORKSPACE, NULL = -1, -2, -3, -4, -7


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "pyramidkv_amd", "libpkv.so")):
        g.build()
    import pyramidkv_amd
    return pyramidkv_amd


# ------------------------------------------------------------------------------------------------ ABI (no launch)
def test_symbol_declared_bound_and_exported(P):
    N = P._native
    hdr = open(os.path.join(ROOT, "include", "pkv.h")).read()
    assert re.search(r"PKV_API int " + NAME + r"\(", hdr) and NAME in N.EXPORTED and hasattr(N.lib, NAME)
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pyramidkv_amd", "libpkv.so")], capture_output=True, text=True).stdout
        assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert N.lib.pkv_version() == N.PKV_VERSION == 204 and "PKV_K_COUNT = 9" in hdr and len(N.KERNEL_NAMES) == 9
    from pyramidkv_amd import monkeypatch as mp
    assert hasattr(P.ops, "decode_attn_think") and hasattr(mp, "think_decode_attention")
    src = open(os.path.join(ROOT, "pyramidkv_amd", "csrc", "pkv_kernels.hpp")).read()
    assert int(re.search(r"constexpr int DECODE_TILE_BYTES = (\d+);", src).group(1)) == N.DECODE_TILE_BYTES


def test_status_of_every_bad_argument(P):
    N = P._native
    D, Rn, Tn = 128, 40, 9

    def call(dt=0, H=4, D=D, kept=77, q=16, qs=D, keep=16, kp=16, R=Rn, kf=16, kfs=None, T=Tn, v=16, vs=None, scale=0.1, sp=1, out=16,
             lse=None, ws=None, nb=0):
        kfs = max(T, 0) * D if kfs is None else kfs
        vs = (max(R, 0) + max(T, 0)) * D if vs is None else vs
        return N.lib.pkv_decode_attn_think(dt, H, D, kept, q, qs, keep, kp, R, kf, kfs, T, v, vs, scale, sp, out, lse, ws, nb, None)

    for dt in (-1, 3, 7):
        assert call(dt=dt) == DTYPE
    for bad in (dict(H=0), dict(H=-3), dict(D=0), dict(D=96), dict(D=512), dict(kept=0), dict(kept=-1), dict(kept=D + 1), dict(R=-1),
                dict(T=-1), dict(qs=64), dict(kfs=Tn * D - 8), dict(kfs=-8), dict(vs=(Rn + Tn) * D - 8), dict(vs=0), dict(sp=-1),
                dict(sp=N.PKV_DECODE_MAX_SPLITS + 1), dict(scale=math.inf), dict(scale=-math.inf), dict(scale=math.nan)):
        assert call(**bad) == SHAPE, bad
    for bad in (dict(q=None), dict(keep=None), dict(kp=None), dict(kf=None), dict(v=None), dict(out=None), dict(sp=2, ws=None, nb=1 << 20)):
        assert call(**bad) == NULL, bad
    for bad in (dict(q=8), dict(kp=24), dict(kp=2), dict(kf=24), dict(v=2), dict(out=4), dict(qs=D + 4), dict(kfs=Tn * D + 4),
                dict(vs=(Rn + Tn) * D + 4), dict(lse=6), dict(sp=2, ws=8, nb=1 << 20)):
        assert call(**bad) == ALIGN, bad
    assert call(dt=2, qs=D + 2) == ALIGN and call(dt=2, kfs=Tn * D + 6) == ALIGN      # fp32 rows: 4 elements = 16 bytes
    # the workspace is the flat-cache one: (max, sum) + an fp32 accumulator per (head, split)
    nb = N.lib.pkv_decode_attn_workspace_bytes(4, D, 3)
    assert nb >= 4 * 3 * (D + 2) * 4
    assert call(sp=3, ws=16, nb=nb - 1) == WORKSPACE and call(sp=3, ws=16, nb=0) == WORKSPACE
    assert call(dt=2, D=64, kept=64, qs=68, sp=2, ws=16, nb=0) == WORKSPACE                  # qs = 68 keeps fp32 rows aligned
    # an empty part needs no pointer, and one that is given is not looked at: the call gets as far as the workspace
    assert call(kp=None, R=0, sp=3, ws=16, nb=0) == WORKSPACE and call(kp=24, R=0, sp=3, ws=16, nb=0) == WORKSPACE
    assert call(kf=None, T=0, sp=3, ws=16, nb=0) == WORKSPACE and call(kf=24, T=0, sp=3, ws=16, nb=0) == WORKSPACE
    # the default route: the flat-cache default for R + T rows, and its workspace
    assert N.lib.pkv_decode_attn_splits(4, D, 260 + 40) == 3
    assert call(R=260, T=40, sp=0, ws=16, nb=nb - 1) == WORKSPACE and call(R=260, T=40, sp=0, ws=None, nb=nb) == NULL
    # a defect of higher rank wins: dtype before shape before null before alignment before workspace
    assert call(dt=9, D=96, q=None) == DTYPE and call(D=96, q=None) == SHAPE and call(kept=0, keep=None) == SHAPE
    assert call(q=None, kf=24) == NULL and call(kp=None, out=4) == NULL and call(kf=24, sp=2, ws=16, nb=0) == ALIGN


def test_wrapper_needs_hip_tensors_and_matching_shapes(P, monkeypatch):
    H, D, Rn, Tn, Dk = 2, 64, 5, 3, 39
    q, keep, kp, kf, v = R.gauss(H, Rn, Tn, D, Dk, torch.bfloat16, 0)
    with pytest.raises(RuntimeError):
        P.ops.decode_attn_think(q, keep, kp, kf, v, 0.125)
    monkeypatch.setattr(P.ops, "_require_gpu", lambda *ts: None)             # the shape checks come next, before any native call
    called = []
    monkeypatch.setattr(P.ops, "_workspace_and_stream", lambda *a: called.append(a))
    for bad in (dict(q=q[0]), dict(keep=keep[:, :-1]), dict(keep=keep.float()), dict(kp=kp[:1]), dict(kp=kp[0]), dict(kf=kf[:, :, :-1]),
                dict(v=v[:, :-1]), dict(v=v[:, :, :32]), dict(kf=kf.float()), dict(kp=torch.zeros(H, Rn, D + 1, dtype=q.dtype)),
                dict(kp=torch.zeros(H, Rn, 0, dtype=q.dtype)), dict(q=q.float())):
        a = dict(q=q, keep=keep, kp=kp, kf=kf, v=v)
        a.update(bad)
        with pytest.raises(ValueError):
            P.ops.decode_attn_think(a["q"], a["keep"], a["kp"], a["kf"], a["v"], 0.125)
    assert called == []


# ------------------------------------------------------------------------------------------------ the ThinK forward's dispatch
@pytest.fixture
def patched():
    pytest.importorskip("transformers")
    import types
    from pyramidkv_amd import monkeypatch as mp
    from test_think_cpu import _RefThinkCluster
    saved = mp._cluster_module, mp.native_decode_attention, mp._is_hip
    mp._cluster_module = types.SimpleNamespace(init_think_native=lambda self: setattr(self, "kv_cluster", _RefThinkCluster(self.config)))
    yield mp
    mp._cluster_module, mp.native_decode_attention, mp._is_hip = saved
    mp.restore()


S, CAP, RECENT, WINDOW = 90, 48, 8, 16


def _prefilled(P, mp, cap=CAP):
    from test_think_cpu import _tiny
    model = _tiny("llama")
    mp.replace_llama("think")
    for layer in model.model.layers:
        c = layer.self_attn.config
        c.window_size, c.max_capacity_prompt, c.kernel_size, c.pooling, c.recent_size, c.ratio = WINDOW, cap, 5, "avgpool", RECENT, 0.4
    ids = torch.randint(0, 97, (1, S), generator=torch.Generator().manual_seed(1))
    cache = P.ThinKCache()
    with torch.no_grad():
        out = model(ids, past_key_values=cache, use_cache=True)
    return model, cache, out.logits[:, -1:].argmax(-1)


@pytest.mark.parametrize("cap", [CAP, 4096])
def test_think_forward_dispatch(P, patched, monkeypatch, cap):
    """HIP tensors (faked) go through ops.decode_attn_think with the layer's mask and its four cache tensors, batch dimension
    squeezed, after the append; CPU tensors, or the switch set to False, run think_decode_attention on the same tensors.
    cap 4096: an unpruned layer (no pruned rows, every channel kept) takes the same call."""
    mp = patched
    model, cache, nxt = _prefilled(P, mp, cap)
    Lyr, H, D = model.config.num_hidden_layers, 4, 64
    Rn, T0, Dk = (cap - RECENT, RECENT, D - int(D * 0.4)) if cap <= S else (0, S, D)
    native, eager = [], []
    real_eager = mp.think_decode_attention

    def stub(q, keep, kp, kf, v, scaling):
        native.append((q, keep, kp, kf, v, float(scaling)))
        return real_eager(q[None, :, None, :], R.keep_index(keep)[None], kp[None], kf[None], v[None], scaling)[0, 0]

    def spy(q, keep_idx, kp, kf, v, scaling):
        eager.append((q, keep_idx, kp, kf, v, float(scaling)))
        return real_eager(q, keep_idx, kp, kf, v, scaling)

    monkeypatch.setattr(P.ops, "decode_attn_think", stub)
    monkeypatch.setattr(mp, "think_decode_attention", spy)
    with torch.no_grad():
        # 1. CPU tensors, switch on: the eager function
        assert mp.native_decode_attention is True
        o1 = model(nxt, past_key_values=cache, use_cache=True).logits
        assert native == [] and len(eager) == Lyr
        for l, (q, idx, kp, kf, v, sc) in enumerate(eager):
            assert q.shape == (1, H, 1, D) and idx is cache.keep_idx[l] and kp is cache.key_cache_pruned[l] and sc == pytest.approx(D ** -0.5)
            assert kp.shape == (1, H, Rn, Dk) and kf.shape == (1, H, T0 + 1, D) and v.shape == (1, H, Rn + T0 + 1, D)
        # 2. tensors taken for HIP tensors: the native wrapper, with the squeezed views after the append
        mp._is_hip = lambda t: True
        o2 = model(nxt, past_key_values=cache, use_cache=True).logits
        assert len(native) == Lyr and len(eager) == Lyr
        for l, (q, keep, kp, kf, v, sc) in enumerate(native):
            assert q.shape == (H, D) and sc == pytest.approx(D ** -0.5)
            assert keep.dtype == torch.bool and keep.shape == (H, D) and keep.data_ptr() == cache.mask[l].data_ptr()
            assert kp.shape == (H, Rn, Dk) and (Rn == 0 or kp.data_ptr() == cache.key_cache_pruned[l].data_ptr())
            assert kf.shape == (H, T0 + 2, D) and kf.data_ptr() == cache.key_cache[l].data_ptr()
            assert v.shape == (H, Rn + T0 + 2, D) and v.data_ptr() == cache.value_cache[l].data_ptr()
            assert int(keep.sum()) == H * Dk
        # 3. the switch off: the eager function even for them
        mp.native_decode_attention = False
        model(nxt, past_key_values=cache, use_cache=True)
        assert len(native) == Lyr and len(eager) == 2 * Lyr and eager[-1][3].shape == (1, H, T0 + 3, D)
    assert torch.isfinite(o1).all() and torch.isfinite(o2).all()


def test_eager_decode_logits_are_those_of_the_inline_arithmetic(P, patched, monkeypatch):
    """think_decode_attention is the decode body the forward used to carry inline; restated here, it gives the same bits."""
    mp = patched

    def inline(q, keep_idx, kp, kr, vv, scaling):
        qp = q.gather(-1, keep_idx.unsqueeze(2))
        w = torch.cat([torch.matmul(qp, kp.transpose(2, 3)), torch.matmul(q, kr.transpose(2, 3))], dim=-1) * scaling
        w = F.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
        return torch.matmul(w, vv).transpose(1, 2).contiguous()

    logits = []
    for fn in (None, inline):
        model, cache, nxt = _prefilled(P, mp)
        if fn is not None:
            monkeypatch.setattr(mp, "think_decode_attention", fn)
        with torch.no_grad():
            steps = []
            for _ in range(3):
                o = model(nxt, past_key_values=cache, use_cache=True).logits
                steps.append(o)
                nxt = o[:, -1:].argmax(-1)
        logits.append(steps)
    for a, b in zip(*logits):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_agrees_with_the_eager_function():
    from pyramidkv_amd.monkeypatch import think_decode_attention
    for (H, Rn, Tn, D, Dk), seed in (((4, 17, 5, 16, 9), 0), ((3, 300, 41, 64, 39), 3), ((2, 0, 7, 64, 64), 5)):
        q, keep, kp, kf, v = R.gauss(H, Rn, Tn, D, Dk, torch.float32, seed)
        idx = R.keep_index(keep)
        assert torch.equal(R.prune(R.widen(kp, keep), keep), kp) and bool((idx[:, 1:] > idx[:, :-1]).all())
        got = think_decode_attention(q[None, :, None, :], idx[None], kp[None], kf[None], v[None], 0.25)[0, 0]
        ref, lse = R.ref_f64(q, keep, kp, kf, v, 0.25)
        assert torch.allclose(got.double(), ref, atol=1e-6, rtol=0)
        for h in range(H):                                        # the same head over full-width keys with zeros in the dropped channels
            s = (torch.cat([R.widen(kp, keep)[h], kf[h]]).double() @ q[h].double()) * 0.25
            assert float(lse[h]) == pytest.approx(float(torch.logsumexp(s, 0)), abs=1e-12)
        E, E_lse = R.eager_fp32_deviation(think_decode_attention, q, keep, kp, kf, v, 0.25, ref, lse)
        assert E.shape == E_lse.shape == (H,) and float(E.max()) < 1e-6 and float(E_lse.max()) < 1e-5
        assert bool((R.out_bar(torch.float32, ref, E) > 0).all())
    ref, lse = R.ref_f64(q, keep, kp[:, :0], kf[:, :0], v[:, :0], 0.25)                      # no rows at all
    assert not ref.any() and bool((lse == -math.inf).all())


def test_masks_differ_per_head_and_cover_the_named_cases():
    for D in (64, 128, 256):
        for Dk in R.kept_widths(D):
            keep = R.masks(5, D, Dk)
            assert keep.sum(1).tolist() == [Dk] * 5
            assert bool(keep[1, D - Dk:].all()) and (Dk == D or (not bool(keep[0, 0]) and not bool(keep[1, :D - Dk].any())))
            if 1 < Dk < D - 1:
                assert len({tuple(r.tolist()) for r in keep}) == 5
    assert R.kept_widths(64)[1] == 39 and R.kept_widths(128)[1] == 77 and R.kept_widths(256)[1] == 154


# ------------------------------------------------------------------------------------------------ the exact fixtures
ORDERS = lambda C: (("forward", {}), ("reversed", {}), ("chunked", dict(chunk=C, splits=1)), ("chunked", dict(chunk=C, splits=3)))  # noqa: E731


@pytest.mark.parametrize("D", [64, 128, 256])
def test_onehot_fixture_has_one_answer_in_every_summation_order(D):
    """Two heads (the mask that drops channel 0, the mask that keeps the last channels) keep the numpy loops short."""
    C, H = R.chunk_rows(), 2
    for dtype in R.DTYPES.values():
        for Dk in R.kept_widths(D):
            keep = R.masks(H, D, Dk)
            pos_differs = R.keep_index(keep)[:, -1] != Dk - 1
            assert Dk == D or bool(pos_differs.all()), "the planted channel's stored column is not its channel index"
            for Rn, Tn in R.shapes(C):
                rows = R.plant_rows(Rn, Tn, C)
                for row in rows if dtype == torch.bfloat16 else rows[-1:]:
                    q, kp, kf, v, want, want_lse = R.onehot_fixture(H, Rn, Tn, D, keep, dtype, row)
                    assert torch.equal(v.double().to(dtype), v) and len({tuple(r.tolist()) for r in v[0, :, :3]}) == Rn + Tn, "distinct rows"
                    for order, kw in ORDERS(C):
                        out, lse = R.attend_f32(q, keep, kp, kf, v, D ** -0.5, order, **kw)
                        assert torch.equal(out.to(dtype).view(torch.uint8), want.view(torch.uint8)), (D, dtype, Dk, Rn, Tn, row, order)
                        assert torch.equal(lse, want_lse)


@pytest.mark.parametrize("D", [64, 128, 256])
def test_uniform_fixture_has_one_answer_in_every_summation_order(D):
    C, H = R.chunk_rows(), 2
    for dtype in R.DTYPES.values():
        for Dk in (R.kept_widths(D)[1], D):
            for Rn, Tn in ((0, 1), (1, 1), (C - 1, 1), (2 * C - 2, 2), (3 * C, C)):
                q, keep, kp, kf, v, want, want_lse = R.uniform_fixture(H, Rn, Tn, D, Dk, dtype)
                for order, kw in ORDERS(C)[:2] + (("chunked", dict(chunk=C, splits=2)),):
                    out, lse = R.attend_f32(q, keep, kp, kf, v, D ** -0.5, order, **kw)
                    assert torch.equal(out.to(dtype).view(torch.uint8), want.view(torch.uint8)), (D, dtype, Dk, Rn, Tn, order)
                    assert bool(((lse.double() - want_lse).abs() <= R.ulp(torch.float32, want_lse)).all())
    assert float(R.uniform_fixture(H, 0, 1, D, D, torch.bfloat16)[6][0]) == 0.0
