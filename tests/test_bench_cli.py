"""bench.py's options and its --dump-outputs writer, on the CPU: a plain run is the headline alone, --steps is the number of
timed steps, and the dump is float, exact and bounded (no GPU: the writer is fed tensors shaped like the headline step's)."""
import os

import numpy as np
import pytest
import torch

import bench


def test_plain_run_is_the_headline_alone():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert bench.parse(["--full", "--dump-outputs", "d"]).full


@pytest.mark.parametrize("argv", (["--steps", "0"], ["--warmup", "-1"]))
def test_steps_must_be_positive(argv):
    with pytest.raises(SystemExit):
        bench.parse(argv)


@pytest.mark.parametrize("B,cap", ((1, 128), (8, 2048)))
def test_dump_outputs_is_float_exact_and_bounded(tmp_path, B, cap):
    ks = [max(1, cap - bench.W - 7 * layer) for layer in range(bench.NUM_LAYERS)]
    g = torch.Generator().manual_seed(5)
    kv = [tuple(torch.randn(B, 4, k + bench.W, bench.D, generator=g).bfloat16() for _ in range(2)) for k in ks]
    idx = [torch.randint(0, 32760, (B, 4, k), dtype=torch.int32, generator=g) for k in ks]
    last = {"kv": kv, "indices": idx, "exchanged": None}
    bench.dump_outputs(str(tmp_path / "a"), last)
    bench.dump_outputs(str(tmp_path / "b"), last)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10 ** 6
    out = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for name, arr in out.items():
        assert arr.dtype in (np.float32, np.float64), name
        assert np.array_equal(arr, np.load(tmp_path / "b" / (name + ".npy"))), name        # same arguments, same files
    want_idx = torch.cat(idx, -1).double().reshape(-1)
    got_idx = out["indices"].reshape(-1)
    if "indices_elements" in out:
        want_idx = want_idx[torch.from_numpy(out["indices_elements"].astype(np.int64))]
    assert np.array_equal(got_idx, want_idx.numpy())
    for j, name in enumerate(("k_compressed", "v_compressed")):
        want = torch.cat([t[j] for t in kv], 2).float()
        if "kv_rows" in out:
            want = want.reshape(-1, bench.D)[torch.from_numpy(out["kv_rows"].astype(np.int64))]
        assert np.array_equal(out[name], want.numpy()), name
