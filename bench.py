#!/usr/bin/env python
"""bench.py - headline benchmark of the KV-compress hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
        N > 1 from a plain shell: bench.py re-executes itself under torch.distributed.run (N ranks, rank r on GPU r,
        backend nccl = RCCL); already under torch.distributed.run (RANK in the environment): runs as that rank.

Workload (BASELINE.json metric: "prefill tokens/s + KV-compress ms at S=32k budget=128, Llama-3-8B"):
  PyramidKV, budget 128, window 8, maxpool-7 (the reference runners' knobs, run_longbench.py:221,236-237),
  Llama-3-8B attention shapes H=32, D=128, S=32768, bf16, synthetic N(0,1) Q/K/V resident in HBM.
  One STEP = the compress work of one model prefill: 32 update_kv calls, layer budgets 234..17
  (pyramidkv_utils.py:205-215), each on a [B,H,S,D] batch.  value = B*S*steps / time.
The step calls the operator API the reference exposes - 32 pre-built PyramidKVCluster objects, `update_kv(K, Q, V, None, g)`
(pyramidkv_utils.py:197) - not the layer below it.
Multi-GPU (N > 1): the headline IS BASELINE config 4 - ONE [1,32,32768,128] sequence, head-sharded: rank r owns 32/N query
heads and their 8/N un-expanded KV heads (one KV head per GPU at N = 8), one RCCL all-gather of the selected indices
(pyramidkv_amd/dist.py); "scaling": "strong".  The embarrassingly parallel weak leg (B = N sequences, H/N heads of each
per GPU) is reported under `scaling_legs` (--full), next to the all-gather's own latency.

A plain run sets up, warms up, times the K steps and prints ONE JSON line with the contract fields (`metric`, `value`,
`unit`, `higher_is_better`, `dtype`, `ms_per_step`, ...) and nothing it would have to run more work for.
`--dump-outputs DIR` then also writes what the last timed step returned to its caller (rank 0's share), as float arrays:
  DIR/indices.npy       [B, H, sum of the 32 layer budgets] every layer's selected token indices, layer after layer
                        (beyond a quarter of the size bound: a fixed seeded sample, flat positions in indices_elements.npy),
  DIR/k_compressed.npy  every layer's compacted K ([B, H, k + window, D] each), concatenated along the token axis,
  DIR/v_compressed.npy  the same for V, and where it would exceed the size bound, a fixed seeded sample of the
  DIR/kv_rows.npy       rows of both (flat row index b * H * T + h * T + t of the concatenated [B, H, T, D]),
  DIR/exchanged_indices.npy  (under torch.distributed.run) the last layer's all-gathered indices.
The inputs are seeded, so two builds given the same arguments can be compared output for output.

`--full` adds everything else, each part measured after the headline; rank 0's line then also carries
  `roofline`          dominant kernel (the K scan) of the headline workload,
  `roofline_kernels`  every kernel of the headline workload AND the north-star kernel at its target configuration:
                      `gather_cap2048_B1` / `gather_cap2048_B8` (SnapKV budget 2048, S = 32768; 67.1 MB x B),
  `grid`              single update_kv calls at B in {1,8} x budget in {128,2048} (device time per kernel),
  `sweep`             BASELINE.json's synthetic sweep: B in {1,2,4,8} x S in {4k,8k,16k,32k}; per single update_kv call (one
                      layer): tokens/s = B*S / call time, and the call's algorithmic bytes against the HBM roofline,
  `gpu_eager_baseline` the reference's eager op sequence (oracle restatement) run by PyTorch-ROCm on this same GPU,
  `cpu_baseline`      the same op sequence on this node's host cores.
"""
import argparse
import contextlib
import hashlib
import io
import json
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling
NUM_LAYERS = 32
D, W, E = 128, 8, 2


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5, help="timed steps (>= 1)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="also the parity check, per-kernel rooflines, extras, sweeps and CPU baselines (--no-cpu-baseline, --no-parity, --no-extras, --only-gqa-extra trim it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float, at most 64 MB in all)")
    ap.add_argument("--seq", type=int, default=32768)
    ap.add_argument("--budget", type=int, default=128)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=8, help="KV heads of the model (Llama-3-8B: 8); the N > 1 headline shards them un-expanded")
    ap.add_argument("--batch", type=int, default=0, help="0 = one sequence per GPU (weak scaling)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--policy", default="pyramidkv", choices=["pyramidkv", "snapkv"])
    ap.add_argument("--allgather", default="prefill", choices=["prefill", "layer"],
                    help="multi-GPU exchange of the selected indices: one all-gather per prefill (all 32 layers) or one per layer")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the oracle comparison of the timed step (layers 0 and 31)")
    ap.add_argument("--no-extras", action="store_true", help="skip grid / gqa / gpu_eager_baseline / strong leg")
    ap.add_argument("--only-gqa-extra", action="store_true", help="of the extras run only the un-expanded-GQA leg (A/B sessions)")
    ap.add_argument("--cpu-layers", type=int, default=32, help="layer-calls per CPU-baseline pass (32 = the whole step)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="CPU work spent on the cpu_baseline sample")
    a = ap.parse_args(argv)
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return a


def layer_budgets(P, policy, cap, w, S):
    ks = []
    for layer in range(NUM_LAYERS):
        if policy == "pyramidkv":
            cl = P.PyramidKVCluster(num_hidden_layers=NUM_LAYERS, layer_idx=layer, window_size=w,
                                    max_capacity_prompt=cap, kernel_size=7, pooling="maxpool")
            _, k = cl.layer_budget(S)
        else:
            k = cap - w
        ks.append(k)
    return ks


def kernel_src_sha16():
    """Identity of the kernel sources a PMC traffic profile belongs to (profiles/*/pmc_traffic.json records it): sha256 over the
    .hip / .hpp files of pyramidkv_amd/csrc with // comments and whitespace runs removed - a comment edit does not orphan a
    profile, a code edit does."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "pyramidkv_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".hpp")):
            code = []
            for line in open(os.path.join(d, f), encoding="utf-8", errors="replace"):
                line = line.split("//", 1)[0]
                line = " ".join(line.split())
                if line:
                    code.append(line)
            h.update(("\n".join(code)).encode())
    return h.hexdigest()[:16]


def make_sets(B, Hl, S, dt, dev, seed, nsets, Hkv=None):
    """(Q, K, V) sets; Hkv < Hl: K/V un-expanded ([B,Hkv,S,D] next to Q [B,Hl,S,D])."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    sets = []
    for _ in range(nsets):
        sets.append(tuple(torch.randn(B, Hl if i == 0 or Hkv is None else Hkv, S, D, generator=gen, device=dev, dtype=torch.float32).to(dt)
                          for i in range(3)))
    return sets


DUMP_BYTES = 60 * 10 ** 6         # --dump-outputs: all arrays together, leaving room for the .npy headers under 64 MB


def dump_outputs(path, last):
    """--dump-outputs: the last timed step's outputs (module docstring) as DIR/<name>.npy.  Indices are written as float64
    (exact), bf16 / fp16 K and V as float32 (exact).  K and V are written whole when they fit in what DUMP_BYTES leaves;
    otherwise the same fixed, seeded sample of rows of both, sorted, with the flat row numbers in kv_rows.npy.  Indices
    beyond a quarter of the bound (large batches and budgets) are sampled the same way (indices_elements.npy)."""
    import numpy as np

    def sample(n, fit):
        return torch.randperm(n, generator=torch.Generator().manual_seed(0))[:fit].sort().values

    os.makedirs(path, exist_ok=True)
    arrays = {"indices": torch.cat(last["indices"], -1).double()}
    fit = DUMP_BYTES // 4 // 16
    if arrays["indices"].numel() > fit:
        sel = sample(arrays["indices"].numel(), fit)
        arrays["indices"] = arrays["indices"].reshape(-1)[sel.to(arrays["indices"].device)]
        arrays["indices_elements"] = sel.double()
    if last["exchanged"] is not None:
        x = last["exchanged"].double()                       # [B, H, k] of the last layer: small; bounded all the same
        arrays["exchanged_indices"] = x if x.numel() <= DUMP_BYTES // 128 else x.reshape(-1)[:DUMP_BYTES // 128]
    kc = torch.cat([kv[0] for kv in last["kv"]], 2)
    vc = torch.cat([kv[1] for kv in last["kv"]], 2)
    left = DUMP_BYTES - sum(t.numel() * 8 for t in arrays.values())
    rows = kc.numel() // kc.shape[-1]
    fit = max(1, left // (2 * kc.shape[-1] * 4 + 8))        # a sampled row: its K and V in float32 + its row number
    if rows > fit:
        sel = sample(rows, fit)
        arrays["kv_rows"] = sel.double()
        sel = sel.to(kc.device)
        kc, vc = kc.reshape(rows, -1)[sel], vc.reshape(rows, -1)[sel]
    arrays["k_compressed"], arrays["v_compressed"] = kc.float(), vc.float()
    for name, t in arrays.items():
        np.save(os.path.join(path, name + ".npy"), t.cpu().numpy())


def make_clusters(P, policy, cap):
    """The operator objects the reference builds per layer (init_pyramidkv / init_snapkv, pyramidkv_utils.py:880-935)."""
    if policy == "pyramidkv":
        return [P.PyramidKVCluster(num_hidden_layers=NUM_LAYERS, layer_idx=layer, window_size=W, max_capacity_prompt=cap,
                                   kernel_size=7, pooling="maxpool") for layer in range(NUM_LAYERS)]
    return [P.SnapKVCluster(window_size=W, max_capacity_prompt=cap, kernel_size=7, pooling="maxpool") for _ in range(NUM_LAYERS)]


def self_launch(a):
    """`python bench.py --gpus N` (N > 1) from a plain shell: start the N ranks ourselves - one process per GPU through
    torch.distributed.run on 127.0.0.1, rank r on device r, process group "nccl" (= RCCL over xGMI).  Rank 0's JSON line
    passes through on stdout; returns the launcher's exit status.  Fewer visible devices than ranks is an error, never a
    silent change of backend (PKV_BENCH_BACKEND=gloo is the explicit opt-in that puts every rank on GPU 0 of a 1-GPU box)."""
    backend = os.environ.get("PKV_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend == "nccl" and ndev < a.gpus:
        sys.stderr.write("bench.py: --gpus %d needs %d visible GPUs for the RCCL process group, found %d "
                         "(PKV_BENCH_BACKEND=gloo runs all ranks on one device: a code-path smoke run, not a measurement)\n"
                         % (a.gpus, a.gpus, ndev))
        return 2
    if ndev < 1:
        sys.stderr.write("bench.py: no GPU visible\n")
        return 2
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // a.gpus)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % a.gpus,
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    a = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    launched = "RANK" in os.environ and "MASTER_PORT" in os.environ      # under torch.distributed.run, any world size
    if a.gpus > 1 and not launched:
        raise SystemExit(self_launch(a))
    if launched and a.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: start one rank per GPU (torch.distributed.run --nproc-per-node %d)"
                         % (a.gpus, world, a.gpus))
    import pyramidkv_amd as P
    from pyramidkv_amd import _native as N, dist as pdist

    # PKV_BENCH_BACKEND=gloo (+ all ranks on one GPU) exists only to exercise the N>1 code path on a 1-GPU box
    backend = os.environ.get("PKV_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    local = local % max(ndev, 1)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if launched:           # also at world size 1: the RCCL communicator and the all-gather are exercised with nranks = 1
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)       # RCCL over xGMI
        else:
            dist.init_process_group(backend)
    collective = dist is not None

    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    S, H, cap = a.seq, a.heads, a.budget
    h0, h1 = pdist.shard_heads(H, rank, world)
    Hl = h1 - h0
    ks = layer_budgets(P, a.policy, cap, W, S)
    NSETS = 4        # distinct (Q,K,V) sets cycled over the layers: a layer never finds its K in the 256 MB Infinity Cache

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    clusters = make_clusters(P, a.policy, cap)
    host_issue = [0.0]

    def timed_leg(B, steps, warmup, sets, dump=False):
        xch = pdist.PrefillIndexExchange(ks, B, Hl, dev, force=collective) if (collective and a.allgather == "prefill") else None
        # every layer's update_kv also leaves its selected indices in a buffer: the exchange's slot, or a plain tensor
        slots = [xch.slot(layer) if xch is not None else torch.empty(B, Hl, ks[layer], dtype=torch.int32, device=dev)
                 for layer in range(NUM_LAYERS)]
        g = sets[0][0].shape[1] // sets[0][1].shape[1]         # query heads per KV head handed over (1 = expanded K/V)

        def one_step(keep=None, collect=None):
            # The one exchange step of the path: the selected indices (KBs).  No layer's update_kv depends on another layer's
            # gathered indices, so (default) all 32 layers write into one buffer that is all-gathered ONCE per prefill;
            # "--allgather layer" issues one asynchronous collective per layer instead (at most two in flight).
            # keep = {layer: None}: the parity leg asks for these layers' (K_c, V_c, local indices) of THIS step function.
            # collect = {} (--dump-outputs): every layer's (K_c, V_c) of this step and the exchanged indices; the previous
            # step's are dropped first, so that every step reuses the same allocations.
            outs, pending = None, []
            if collect is not None:
                collect.clear()
                collect["kv"] = []
            for layer in range(NUM_LAYERS):
                q, k, v = sets[layer % len(sets)]
                cl = clusters[layer]
                cl.index_out = slots[layer]
                kc, vc = cl.update_kv(k, q, v, None, g)
                idx = slots[layer]
                if keep is not None and layer in keep:
                    keep[layer] = (kc, vc, idx.clone())
                if collect is not None:
                    collect["kv"].append((kc, vc))
                if xch is None:
                    if collective:
                        pending.append(pdist.allgather_indices_async(idx, force=True))
                        if len(pending) > 2:
                            idx = pending.pop(0).wait()
                outs = (kc, vc, idx)
            if xch is not None:
                outs = (outs[0], outs[1], xch.views(xch.gather_async())[-1])
            for h in pending:
                outs = (outs[0], outs[1], h.wait())
            if collect is not None:
                collect["exchanged"] = outs[2] if collective else None
            return outs

        collect = {} if dump else None
        for _ in range(warmup):
            one_step(collect=collect)
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            one_step(collect=collect)
        barrier()
        el = time.perf_counter() - t0
        last = None
        if dump:                             # the last timed step's outputs, before anything else runs the step again
            last = {"kv": collect["kv"], "indices": [s.clone() for s in slots],
                    "exchanged": collect["exchanged"].clone() if collect["exchanged"] is not None else None}
        if dist is not None and world > 1:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        ag_us = None
        if not a.full:
            return el, one_step, ag_us, last
        # this rank's host time to ISSUE one step (32 calls) into an empty queue - measured on its own: inside the timed loop the
        # host runs ahead of the device until the hardware queue is full and then waits for it
        barrier()
        h0 = time.perf_counter()
        one_step()
        host_issue[0] = time.perf_counter() - h0
        barrier()
        if xch is not None:                  # the collective alone: issue + wait, nothing else on the device
            barrier()
            t0 = time.perf_counter()
            for _ in range(20):
                xch.views(xch.gather_async())
            torch.cuda.synchronize()
            ag_us = (time.perf_counter() - t0) / 20 * 1e6
        return el, one_step, ag_us, last

    # ---- headline leg ----
    # N = 1: one [B,H,S,D] sequence batch with K/V as the reference's update_kv receives them (after repeat_kv).
    # N > 1: BASELINE config 4 - ONE sequence, rank r owns H/N query heads and their KV heads UN-EXPANDED (Llama-3-8B: 8 KV
    # heads, one per GPU at N = 8); strong scaling.  --batch B overrides the batch size.
    strong = world > 1 and a.batch == 0
    B = a.batch if a.batch > 0 else 1
    Hkv = None
    if strong and a.kv_heads % world == 0 and (H // a.kv_heads) * W <= 256:
        Hkv = a.kv_heads // world
    sets = make_sets(B, Hl, S, dt, dev, 1234 + rank, NSETS, Hkv)
    el, one_step, ag_us, last = timed_leg(B, a.steps, a.warmup, sets, dump=bool(a.dump_outputs))
    host_us_per_call = host_issue[0] / NUM_LAYERS * 1e6
    ms_per_step = el / a.steps * 1e3
    tokens_per_s = B * S * a.steps / el
    if last is not None and rank == 0:
        dump_outputs(a.dump_outputs, last)
    del last
    headline = {
        "metric": "prefill tokens/s through KV-compress (PyramidKV budget=%d, S=%d, Llama-3-8B shapes)" % (cap, S),
        "value": round(tokens_per_s, 1), "unit": "tokens/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(ms_per_step, 4), "kv_compress_ms_per_layer": round(ms_per_step / NUM_LAYERS, 5),
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": a.dtype,
        "data": "synthetic",
        "config": {"workload": "%s budget=%d window=8 maxpool7, 32 update_kv calls/step, [B=%d,H=%d,S=%d,D=128] %s"
                               % (a.policy, cap, B, H, S, a.dtype),
                   "global_batch": B, "seq_len": S, "heads_per_gpu": Hl,
                   "kv_heads_per_gpu": Hkv if Hkv else Hl,
                   "kv_layout": ("un-expanded GQA: %d of the model's %d KV heads per GPU, kv_group %d" % (Hkv, a.kv_heads, Hl // Hkv)) if Hkv
                                else "expanded (after repeat_kv, as the reference's update_kv receives it)",
                   "timed_through": "PyramidKVCluster.update_kv" if a.policy == "pyramidkv" else "SnapKVCluster.update_kv",
                   "parallelism": ("head-shard x%d + 1 all-gather(indices) per %s" % (world, a.allgather)) if collective else "single GPU",
                   "collective_backend": (backend if collective else None)},
    }
    if not a.full:
        if rank == 0:
            print(json.dumps(headline))
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    # ---- parity of the TIMED path: the step function that was just timed, layers 0 and 31, against the CPU oracle ----
    parity = None
    if not a.no_parity:
        keep = {0: None, NUM_LAYERS - 1: None}
        one_step(keep)                       # every rank: the step holds the collective
        torch.cuda.synchronize()
        if rank == 0:
            parity = parity_block(keep, sets, ks, cap, a, S)

    # ---- per-kernel device time over the same K steps (events on the dispatches, inside libpkv) ----
    N.prof_enable(True)
    N.prof_read(reset=True)
    for _ in range(a.steps):
        one_step()
    torch.cuda.synchronize()
    prof = N.prof_read(reset=True)
    N.prof_enable(False)

    def rl(prof_, name, bytes_per_launch, label=None):
        ms, n = prof_[name]
        if n == 0:
            return None
        avg_ms = ms / n
        ach = bytes_per_launch / (avg_ms * 1e-3) / 1e9
        return {"kernel": label or name, "bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None, "avg_us": round(avg_ms * 1e3, 2),
                "launches": int(n), "algorithmic_bytes": int(bytes_per_launch)}

    def alg_bytes(B_, Hl_, S_, k_mean, g_=1):
        n = B_ * Hl_
        return {
            "logits": (n // g_) * S_ * D * E + n * W * D * E,            # K read once per KV head + the w query rows
            "finalize": n * (W * S_ * E + (S_ - W) * E),                 # logits [w][S] read once, pooled scores written
            "topk": n * ((S_ - W) * E + k_mean * 4),
            "gather": 4 * (k_mean + W) * D * E * n,                      # 2 tensors x (k+w) rows x D x e x (read+write)
        }

    def kernel_rows(prof_, alg_):
        """One roofline row per kernel that ran."""
        rows_ = {}
        for name, by in alg_.items():
            r = rl(prof_, name, by)
            if r:
                rows_[name] = r
        return rows_

    alg = alg_bytes(B, Hl, S, sum(ks) / NUM_LAYERS, (Hl // Hkv) if Hkv else 1)
    kernels = kernel_rows(prof, alg)
    # HBM traffic per launch from rocprofv3 PMC passes (tools/pmc_summary.py).  Only attached when the profile was taken
    # from exactly these kernel sources and this workload; otherwise the field stays null instead of going stale.
    src_id = kernel_src_sha16()
    for pmc_path in sorted(__import__("glob").glob(os.path.join(ROOT, "profiles", "r*", "pmc_traffic.json")), reverse=True):
        pmc = json.load(open(pmc_path))
        if pmc.get("kernel_src_sha16") == src_id and a.seq == 32768 and a.budget == 128 and B == 1 and world == 1:
            for k_, v_ in kernels.items():
                if k_ in pmc.get("kernels", {}):
                    v_["traffic"] = pmc["kernels"][k_].get("hbm_bytes_per_launch")
                    v_["traffic_source"] = os.path.relpath(pmc_path, ROOT)
                    v_["traffic_measured_in_run"] = False      # rocprofv3 --pmc passes of the same workload, same kernel sources
                    v_["traffic_kernel_src_sha16"] = pmc.get("kernel_src_sha16")
            break

    def attach_north_traffic(north):
        """PMC traffic of the budget-2048 gather (tools/gather_pmc.py under rocprofv3 --pmc), same staleness rule."""
        for pmc_path in sorted(__import__("glob").glob(os.path.join(ROOT, "profiles", "r*", "pmc_traffic.json")), reverse=True):
            pmc = json.load(open(pmc_path))
            if pmc.get("kernel_src_sha16") == src_id:
                for k_, v_ in (north or {}).items():
                    if v_ and k_ in pmc.get("kernels", {}):
                        v_["traffic"] = pmc["kernels"][k_].get("hbm_bytes_per_launch")
                        v_["traffic_source"] = os.path.relpath(pmc_path, ROOT)
                        v_["traffic_measured_in_run"] = False
                        v_["traffic_kernel_src_sha16"] = pmc.get("kernel_src_sha16")
                break

    out = dict(headline)
    out.update({
        "roofline": kernels.get("logits"),
        "roofline_kernels": kernels,
        # one update_kv of this rank: host time to issue it (Python + the C call with its four launches) next to the device time
        # of its kernels (events on the dispatches).  The timed loop issues calls back to back, so a call costs
        # max(host_us_per_call, device_us_per_call + launch gaps): where the host figure is the larger one the line is
        # host-issue-bound (expected for the strong leg from N = 4 up)
        "host_us_per_call": round(host_us_per_call, 2),
        "device_us_per_call": round(sum(r_["avg_us"] for r_ in kernels.values()), 2),
        "parity": parity,
        "kernel_src_sha16": src_id,
    })
    if collective:
        out["config"]["process_group_backend"] = dist.get_backend()
        out["rccl_nranks"] = dist.get_world_size() if dist.get_backend() == "nccl" else None
        out["allgather_us"] = round(ag_us, 1) if ag_us is not None else None      # one all-gather of the whole prefill's indices, alone
        out.update(first_contact(dist, backend, world, rank, dev, pdist, ks, B, Hl, a))
    # whole-call effective bandwidth: all algorithmic bytes of a call / its wall time
    out["call_effective"] = {"GBps": round(sum(alg.values()) / (ms_per_step / NUM_LAYERS * 1e-3) / 1e9, 1),
                             "frac_of_8TBps": round(sum(alg.values()) / (ms_per_step / NUM_LAYERS * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    del sets
    torch.cuda.empty_cache()

    # ---- second multi-GPU leg: weak scaling (B = N sequences, H/N expanded heads of each per GPU: per-GPU bytes constant) ----
    if strong and not a.no_extras:
        wsets = make_sets(world, Hl, S, dt, dev, 99 + rank, 2)
        wel, _, _, _ = timed_leg(world, a.steps, 1, wsets)
        out["scaling_legs"] = {
            "strong_config4": {"global_batch": 1, "tokens_per_s": round(tokens_per_s, 1), "ms_per_step": round(ms_per_step, 4),
                               "kv_compress_ms_per_layer": round(ms_per_step / NUM_LAYERS, 5),
                               "note": "BASELINE config 4 (this is `value`): one 32k sequence, %d query heads%s per GPU; every call is a "
                                       "%.1f MB K scan under a ~20 us latency tail, so this leg cannot scale linearly (DESIGN.md section 7)"
                                       % (Hl, (" / %d KV heads" % Hkv) if Hkv else "", (Hkv or Hl) * S * D * E / 1e6)},
            "weak": {"global_batch": world, "tokens_per_s": round(world * S * a.steps / wel, 1), "ms_per_step": round(wel / a.steps * 1e3, 4),
                     "note": "B = N sequences, H/N expanded heads of each per GPU: per-GPU bytes constant, no data-path dependency between ranks"}}
        del wsets
        torch.cuda.empty_cache()

    if world == 1 and a.only_gqa_extra:
        out["extras"], gqa_rows = gqa_extra(P, N, rl, dt, dev, S, H, ks, a.steps)
        if S == 32768 and a.budget == 128:
            attach_north_traffic(gqa_rows)       # logits_gqa4: K read once per KV head + the logits write (PMC passes of this leg)
        out["roofline_kernels"].update(gqa_rows)
    elif world == 1 and not a.no_extras:
        out["grid"], north = grid_rows(P, N, dt, dev, S, H, rl, alg_bytes, kernel_rows)
        attach_north_traffic(north)
        out["roofline_kernels"].update(north)
        out["extras"], gqa_rows = gqa_extra(P, N, rl, dt, dev, S, H, ks, a.steps)
        if S == 32768 and a.budget == 128:
            attach_north_traffic(gqa_rows)
        out["roofline_kernels"].update(gqa_rows)
        out["extras"]["two_streams"] = two_stream_extra(P, dt, dev, S, H, ks, a.steps)
        out["extras"]["h2o"] = h2o_extra(P, N, dt, dev, S, H)
        # the BASELINE configurations the headline does not time (review of round 4): config 2 (PyramidKV at S = 8192), config 5
        # (Mistral GQA Ada-SnapKV at S = 32768) and the LOOK-M merge, each with per-kernel rows, a roofline row and a parity block
        out["extras"]["config2_pyramidkv_8k"] = config2_extra(P, N, rl, alg_bytes, kernel_rows, a, dt, dev, H)
        out["extras"]["config5_adakv_gqa_32k"] = config5_extra(P, N, a, dt, dev)
        out["extras"]["merge"] = merge_extra(P, dt, dev, H)
        out["sweep"] = seq_batch_sweep(P, dt, dev, H, alg_bytes)
        out["gpu_eager_baseline"] = gpu_eager_baseline(dt, dev, S, H, cap)
        # round 6: the same-chip three-way parity block, the real-distribution leg, BASELINE.md section 3's remaining grid rows and
        # the metric's "prefill tokens/s" on a model with Llama-3-8B's dimensions
        if not a.no_parity and out.get("parity") is not None:
            out["parity"]["vs_device_reference"] = three_way_block(P, dev, S, H)
        out["extras"]["robust"] = robust_extra(P, N, dev, S, H, a)
        out["extras"]["baseline_grid"] = baseline_grid_extra(P, N, rl, alg_bytes, kernel_rows, a, dev, S, H)
        out["extras"]["e2e_prefill"] = e2e_prefill_extra(P, N, dev)
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        sets = make_sets(1, Hl, S, dt, dev, 1234 + rank, 1)
        out["cpu_baseline"] = cpu_baseline(sets[0], ks, W, cap, a)
        del sets
        torch.cuda.empty_cache()
        if not a.no_extras:
            out["cpu_baselines_more"] = cpu_baselines_more(P, dev, a)
    if rank == 0:
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def parity_block(keep, sets, ks, cap, a, S):
    return parity_block_for(keep, sets, ks, cap, a.policy, a.dtype, S)


def parity_block_for(keep, sets, ks, cap, policy, dtype_name, S):
    """The timed step's own outputs for layers 0 and 31 (first sequence, this rank's heads) against the CPU oracle
    (oracle.pyramidkv_update_kv / snapkv_update_kv == the reference's update_kv, canonical tie order) on the same tensors:
    fraction of heads whose selected index SET / index SEQUENCE / compacted K and V bits are the oracle's.  Where a
    sequence differs, `max_order_inversion_ulp` is the largest rise of the oracle's scores read in the kernel's order, in
    units of the last place: two implementations whose scores agree within one unit can swap neighbours at most two units
    apart (the documented floor: ATen's own CPU softmax sums in a machine-dependent order)."""
    from oracle import pkv_oracle as O
    res = {"checker": "oracle/pkv_oracle.py on the host CPU, same tensors as the timed step", "layers": {}}
    agg = {"heads_identical_set": 1.0, "heads_identical_sequence": 1.0, "kv_bit_identical_heads": 1.0, "max_order_inversion_ulp": 0}
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    for layer, got in sorted(keep.items()):
        q, k, v = (t[:1].cpu() for t in sets[layer % len(sets)])
        if k.shape[1] != q.shape[1]:                                   # un-expanded K/V: the oracle takes what repeat_kv hands the reference
            k, v = (t.repeat_interleave(q.shape[1] // t.shape[1], dim=1) for t in (k, v))
        kc, vc, idx = (t[:1].cpu() for t in got)
        with contextlib.redirect_stdout(io.StringIO()):
            if policy == "pyramidkv":
                kr, vr, ridx = O.pyramidkv_update_kv(k, q, v, W, cap, 7, "maxpool", NUM_LAYERS, layer, return_indices=True)
            else:
                kr, vr, ridx = O.snapkv_update_kv(k, q, v, W, cap, 7, "maxpool", return_indices=True)
            so = O.pool_scores(O.window_scores(q, k, W), "maxpool", 7)
        ia = idx.long()
        seq_h = (ia == ridx).all(-1)[0]
        set_h = (torch.sort(ia, -1).values == torch.sort(ridx, -1).values).all(-1)[0]
        kv_h = ((kc == kr).flatten(2).all(-1) & (vc == vr).flatten(2).all(-1))[0]
        # oracle scores read in the kernel's order must be non-increasing up to one unit in the last place
        sel = torch.gather(so, -1, ia).view(torch.int16).int()
        key = torch.where(sel < 0, -(sel & 0x7fff), sel)                       # monotone integer image of the 16-bit floats
        inv = max(0, int((key[..., 1:] - key[..., :-1]).max().item())) if key.shape[-1] > 1 else 0
        row = {"k": int(ks[layer]), "heads": int(seq_h.numel()),
               "heads_identical_set": float(set_h.float().mean()), "heads_identical_sequence": float(seq_h.float().mean()),
               "kv_bit_identical_heads": float(kv_h.float().mean()), "max_order_inversion_ulp": inv}
        res["layers"][str(layer)] = row
        for f in ("heads_identical_set", "heads_identical_sequence", "kv_bit_identical_heads"):
            agg[f] = min(agg[f], row[f])
        agg["max_order_inversion_ulp"] = max(agg["max_order_inversion_ulp"], inv)
    res.update(agg)
    res["shape"] = "[1,%d,%d,128] %s, layers %s of the timed step" % (sets[0][0].shape[1], S, dtype_name, sorted(keep))
    return res


def seq_batch_sweep(P, dt, dev, H, alg_bytes):
    """The synthetic sweep BASELINE.json names ([B = 1..8, H = 32, S = 4k..32k, D = 128]): one SnapKVCluster.update_kv (budget
    128) per point, wall time per call (events around 10 calls on rotating inputs) as tokens/s and as a fraction of the HBM
    roofline over the call's algorithmic bytes; `host_us` = host time to issue one call."""
    rows = []
    for S in (4096, 8192, 16384, 32768):
        for B in (1, 2, 4, 8):
            k_sel = 128 - W
            nset = max(2, min(4, int(1.6e9 // (3 * B * H * S * 256))))
            sets = make_sets(B, H, S, dt, dev, 100 + B + S, nset)
            cl = P.SnapKVCluster(window_size=W, max_capacity_prompt=128, kernel_size=7, pooling="maxpool")
            for it in range(3):
                q, k, v = sets[it % len(sets)]
                cl.update_kv(k, q, v, None, 1)
            torch.cuda.synchronize()
            iters = 10
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            h0 = time.perf_counter()
            for it in range(iters):
                q, k, v = sets[it % len(sets)]
                cl.update_kv(k, q, v, None, 1)
            host_us = (time.perf_counter() - h0) / iters * 1e6       # host time to ISSUE one call (no sync): the floor a faster GPU path runs into
            ev1.record()
            torch.cuda.synchronize()
            call_us = ev0.elapsed_time(ev1) / iters * 1e3
            alg = alg_bytes(B, H, S, k_sel)
            rows.append({"B": B, "S": S, "update_kv_us": round(call_us, 2), "host_us": round(host_us, 2), "tokens_per_s": round(B * S / call_us * 1e6, 0),
                         "call_effective_frac_of_8TBps": round(sum(alg.values()) / (call_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)})
            del sets
            torch.cuda.empty_cache()
    return rows


def grid_rows(P, N, dt, dev, S, H, rl, alg_bytes, kernel_rows):
    """Single SnapKV update_kv calls at B in {1,8} x budget in {128,2048}: wall time per call (events around 10 calls) and
    device time per kernel (events on the dispatches).  Returns (rows, {gather_cap2048_B1, gather_cap2048_B8})."""
    rows, north = [], {}
    for B in (1, 8):
        sets = make_sets(B, H, S, dt, dev, 7 + B, 2 if B > 1 else 4)
        for cap in (128, 2048):
            k_sel = cap - W
            for it in range(3):
                q, k, v = sets[it % len(sets)]
                P.ops.compress(q, k, v, W, k_sel, "maxpool", 7)
            torch.cuda.synchronize()
            iters = 10
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for it in range(iters):
                q, k, v = sets[it % len(sets)]
                P.ops.compress(q, k, v, W, k_sel, "maxpool", 7)
            ev1.record()
            torch.cuda.synchronize()
            call_us = ev0.elapsed_time(ev1) / iters * 1e3
            N.prof_enable(True)
            N.prof_read(reset=True)
            for it in range(iters):
                q, k, v = sets[it % len(sets)]
                P.ops.compress(q, k, v, W, k_sel, "maxpool", 7)
            torch.cuda.synchronize()
            prof = N.prof_read(reset=True)
            N.prof_enable(False)
            alg = alg_bytes(B, H, S, k_sel)
            row = {"policy": "snapkv", "B": B, "budget": cap, "S": S, "update_kv_us": round(call_us, 2),
                   "tokens_per_s": round(B * S / call_us * 1e6, 0),
                   "call_effective_frac_of_8TBps": round(sum(alg.values()) / (call_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
            for name, r in kernel_rows(prof, alg).items():
                row[name] = {"us": r["avg_us"], "GBps": r["achieved"], "frac": r["frac"],
                             "alg_MB": round(r["algorithmic_bytes"] / 1e6, 2)}
            rows.append(row)
            if cap == 2048:
                north["gather_cap2048_B%d" % B] = rl(prof, "gather", alg["gather"], "gather (SnapKV budget 2048, S=%d, B=%d)" % (S, B))
        del sets
        torch.cuda.empty_cache()
    return rows, north


def gqa_extra(P, N, rl, dt, dev, S, H, ks, steps):
    """Extra (not `value`): the headline workload when K/V are handed over BEFORE repeat_kv (8 KV heads, what the
    transformers adapter does): the kernels read every KV head once per group."""
    if H % 4:
        return {}, {}
    sets = []
    for (q, k, v) in make_sets(1, H, S, dt, dev, 4321, 4):
        sets.append((q, k[:, ::4].contiguous(), v[:, ::4].contiguous()))

    def gstep():
        for layer in range(NUM_LAYERS):
            q, k, v = sets[layer % len(sets)]
            P.ops.compress(q, k, v, W, ks[layer], "maxpool", 7, kv_group=4)
    gstep()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        gstep()
    torch.cuda.synchronize()
    ge = time.perf_counter() - t0
    # per-kernel device time of the same steps: this is the configuration the transformers adapter runs
    # (monkeypatch.skip_repeat_kv), so its K scan gets a roofline row of its own (K bytes / 4)
    N.prof_enable(True)
    N.prof_read(reset=True)
    for _ in range(steps):
        gstep()
    torch.cuda.synchronize()
    prof = N.prof_read(reset=True)
    N.prof_enable(False)
    k_mean = sum(ks) / NUM_LAYERS
    rows = {
        "logits_gqa4": rl(prof, "logits", (H // 4) * S * D * E + H * W * D * E, "logits (K/V un-expanded, kv_group 4: 8 KV heads)"),
        "finalize_gqa4": rl(prof, "finalize", H * (W * S * E + (S - W) * E), "finalize (kv_group 4)"),
        "topk_gqa4": rl(prof, "topk", H * ((S - W) * E + k_mean * 4), "topk (kv_group 4)"),
        "gather_gqa4": rl(prof, "gather", 4 * (k_mean + W) * D * E * H, "gather (kv_group 4: rows read from 8 KV heads)"),
    }
    alg_total = sum(r["algorithmic_bytes"] for r in rows.values() if r)
    return {"unexpanded_gqa_tokens_per_s": round(S * steps / ge, 1),
            "unexpanded_gqa_us_per_layer": round(ge / steps / NUM_LAYERS * 1e6, 2),
            "call_effective_frac_of_8TBps": round(alg_total / (ge / steps / NUM_LAYERS) / 1e9 / HBM_PEAK_GBS, 4),
            "note": "K/V handed over before repeat_kv (8 KV heads for 32 query heads); not the headline value"}, \
        {k_: v_ for k_, v_ in rows.items() if v_}


def _smi_sampler(samples, stop):
    """rocm-smi power / shader clock of GPU 0 every ~50 ms until stop[0] (what the H2O pair runs at: it sits at the board's power cap)."""
    import re
    while not stop[0]:
        try:
            r = subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--json"], capture_output=True, text=True, timeout=5)
            c = next(iter(json.loads(r.stdout).values()))
            pw = next((float(v) for k_, v in c.items() if "Power" in k_ and "W" in k_ and re.match(r"^[0-9.]+$", str(v))), None)
            m = re.search(r"(\d+)Mhz", str(next((v for k_, v in c.items() if k_.startswith("sclk")), "")))
            samples.append((pw, float(m.group(1)) if m else None))
        except Exception:       # noqa: BLE001 - no rocm-smi / another output format: the fields stay null
            samples.append((None, None))
        time.sleep(0.05)


def h2o_extra(P, N, dt, dev, S, H):
    """Extra (not `value`): BASELINE config 3's other policy - the H2O score of all S query rows (pyramidkv_utils.py:544-554),
    the one kernel pair of this path that is bound by the matrix + vector pipes instead of HBM: 2 * 2 * S^2 * D * H flop against
    the dense bf16 MFMA peak (2.5 PFLOP/s).  Device time of the two passes from events on the dispatches.  `roofline_issue`
    prices the same time against what actually bounds the pair (profiles/r04/h2o/h2o_account.md): a SIMD issues one vector
    instruction per 4 cycles and the port is blocked ~0.4 of an MFMA's duration, which puts the floor of the reference's
    rounding chain at ~34 (pass 1) / ~33 (pass 2) cycles per 64 elements; cycles here = pass time x the shader clock sampled
    with rocm-smi DURING the passes x 1024 SIMDs / (S^2 H / 64)."""
    import threading
    (q, k, _), = make_sets(1, H, S, dt, dev, 808, 1)
    for _ in range(2):
        P.ops.score_h2o(q, k, W)
    torch.cuda.synchronize()
    samples, stop = [], [False]
    th = threading.Thread(target=_smi_sampler, args=(samples, stop))
    th.start()
    N.prof_enable(True)
    N.prof_read(reset=True)
    iters = 0
    t0 = time.perf_counter()
    while iters < 5 or time.perf_counter() - t0 < 0.6:          # ~0.6 s: a dozen rocm-smi samples under load
        P.ops.score_h2o(q, k, W)
        torch.cuda.synchronize()
        iters += 1
    stop[0] = True
    th.join()
    prof = N.prof_read(reset=True)
    N.prof_enable(False)
    ms = {kk: prof[kk][0] / max(1, prof[kk][1]) for kk in ("h2o_stats", "h2o_colsum")}
    total = ms["h2o_stats"] + ms["h2o_colsum"]
    flop = 2.0 * 2.0 * S * S * D * H
    pw = [x[0] for x in samples[1:] if x[0]]
    sc = [x[1] for x in samples[1:] if x[1]]
    sclk = sum(sc) / len(sc) if sc else None
    groups = float(S) * S * H / 64.0 / 1024.0                   # 64-element groups per SIMD and pass
    issue = None
    if sclk:
        c1, c2 = (ms[kk] * 1e-3 * sclk * 1e6 / groups for kk in ("h2o_stats", "h2o_colsum"))
        issue = {"bound": "vector issue + blocked MFMA port", "unit": "cycles per 64 elements and SIMD",
                 "achieved": {"stats": round(c1, 1), "colsum": round(c2, 1)}, "floor": {"stats": 34.0, "colsum": 33.0},
                 "frac": round((34.0 + 33.0) / (c1 + c2), 4), "sclk_mhz_during_the_passes": round(sclk),
                 "power_w_mean": round(sum(pw) / len(pw), 1) if pw else None, "samples": len(sc)}
    return {"h2o_score_ms": round(total, 3), "stats_ms": round(ms["h2o_stats"], 3), "colsum_ms": round(ms["h2o_colsum"], 3),
            "roofline": {"bound": "mfma", "achieved": round(flop / (total * 1e-3) / 1e12, 1), "peak": 2500.0, "unit": "TFLOP/s",
                         "frac": round(flop / (total * 1e-3) / 1e12 / 2500.0, 4)},
            "roofline_issue": issue,
            "note": "[1,%d,%d,128] %s, N(0,1) inputs: the chip runs this pair at its power cap (profiles/r04/h2o/h2o_account.md); "
                    "round 5: pass 1 takes its exponentials relative to the first key tile's maximum (no key-norm scan; robust to "
                    "large-norm keys, profiles/r05/h2o_ab.txt)" % (H, S, str(dt).replace("torch.", ""))}


def two_stream_extra(P, dt, dev, S, H, ks, steps):
    """Extra (not `value`): the same 32 update_kv calls issued alternately on two streams.  One call is a bandwidth-bound K scan
    followed by a latency-bound tail (finalize, top-k, gather: ~22 us on a few CUs); in a real prefill that tail overlaps
    with the next kernels of the model - here with the next call's K scan.  Throughput, not single-call latency."""
    sets = make_sets(1, H, S, dt, dev, 977, 4)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]

    def step():
        for layer in range(NUM_LAYERS):
            q, k, v = sets[layer % len(sets)]
            with torch.cuda.stream(streams[layer & 1]):
                P.ops.compress(q, k, v, W, ks[layer], "maxpool", 7)
    for st in streams:
        st.wait_stream(torch.cuda.current_stream(dev))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def step_one():                     # the same calls on the same tensors, all on the current stream: the like-for-like figure
        for layer in range(NUM_LAYERS):
            q, k, v = sets[layer % len(sets)]
            P.ops.compress(q, k, v, W, ks[layer], "maxpool", 7)
    el1 = timed(step_one)
    el = timed(step)
    return {"tokens_per_s": round(S * steps / el, 1), "us_per_update_kv": round(el / steps / NUM_LAYERS * 1e6, 2),
            "one_stream_us_per_update_kv": round(el1 / steps / NUM_LAYERS * 1e6, 2),
            "note": "32 calls per step alternating between two streams (the tail of call i overlaps the K scan of call i+1); "
                    "`one_stream_us_per_update_kv` = the same calls on the same expanded tensors on one stream"}


def config2_extra(P, N, rl, alg_bytes, kernel_rows, a, dt, dev, H):
    """BASELINE config 2 (not `value`): Llama-3-8B shapes, PyramidKV budget 128 at S = 8192 (the reference runners' real
    LongBench length), all 32 layer budgets through 32 pre-built PyramidKVCluster.update_kv: wall time per call, host time to
    issue a call, device time per kernel, the K scan against the HBM roofline, and the parity of layers 0 and 31."""
    S, cap = 8192, 128
    ks = layer_budgets(P, "pyramidkv", cap, W, S)
    clusters = make_clusters(P, "pyramidkv", cap)
    sets = make_sets(1, H, S, dt, dev, 2222, 4)
    slots = [torch.empty(1, H, ks[layer], dtype=torch.int32, device=dev) for layer in range(NUM_LAYERS)]

    def step(keep=None):
        for layer in range(NUM_LAYERS):
            q, k, v = sets[layer % len(sets)]
            cl = clusters[layer]
            cl.index_out = slots[layer]
            kc, vc = cl.update_kv(k, q, v, None, 1)
            if keep is not None and layer in keep:
                keep[layer] = (kc, vc, slots[layer].clone())
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    steps = max(5, a.steps)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    N.prof_enable(True)
    N.prof_read(reset=True)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    prof = N.prof_read(reset=True)
    N.prof_enable(False)
    alg = alg_bytes(1, H, S, sum(ks) / NUM_LAYERS)
    rows = kernel_rows(prof, alg)
    call_us = el / steps / NUM_LAYERS * 1e6
    res = {"workload": "pyramidkv budget=128 window=8 maxpool7, 32 update_kv calls/step, [1,%d,%d,128] %s (expanded K/V)" % (H, S, a.dtype),
           "update_kv_us": round(call_us, 2), "host_us": round(host / steps / NUM_LAYERS * 1e6, 2),
           "tokens_per_s": round(S * steps / el, 1), "ms_per_step": round(el / steps * 1e3, 4),
           "kernels_us": {k_: r["avg_us"] for k_, r in rows.items()},
           "kernels_sum_us": round(sum(r["avg_us"] for r in rows.values()), 2),
           "roofline": rows.get("logits"),
           "call_effective_frac_of_8TBps": round(sum(alg.values()) / (call_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
    if not a.no_parity:
        keep = {0: None, NUM_LAYERS - 1: None}
        step(keep)
        torch.cuda.synchronize()
        res["parity"] = parity_block_for(keep, sets, ks, cap, "pyramidkv", a.dtype, S)
    del sets
    torch.cuda.empty_cache()
    return res


def config5_extra(P, N, a, dt, dev):
    """BASELINE config 5 (not `value`): Mistral-7B attention shapes (32 query heads, 8 KV heads, D = 128), K/V handed over
    UN-EXPANDED, S = 32768, Ada-SnapKV (floor 0.2, normalize, maxpool-7, window 8) at budget 128 and 2048 through
    AdaKVCluster.update_kv: wall time per call (the call holds the one host sync of the policy, :718), device time per kernel,
    what is left for host / sync, the call's algorithmic bytes against the HBM roofline, and a parity block against
    oracle.adakv_update_kv (the reference's op sequence on the repeat_kv-expanded tensors)."""
    from oracle import pkv_oracle as O
    Hq, Hkv, S = 32, 8, 32768
    g = Hq // Hkv
    sets = make_sets(1, Hq, S, dt, dev, 5150, 3, Hkv)
    res = {"workload": "Ada-SnapKV floor=0.2 normalize window=8 maxpool7, q [1,%d,%d,128] + un-expanded K/V [1,%d,%d,128] %s" % (Hq, S, Hkv, S, a.dtype)}
    for cap in (128, 2048):
        cl = P.AdaKVCluster(window_size=W, kernel_size=7, pooling="maxpool", max_capacity_prompt=cap, floor=0.2, normalize=True,
                            layer_idx=0, num_hidden_layers=NUM_LAYERS)
        for it in range(4):
            q, k, v = sets[it % len(sets)]
            cl.update_kv(k, q, v)
        torch.cuda.synchronize()
        iters = 30
        t0 = time.perf_counter()
        for it in range(iters):
            q, k, v = sets[it % len(sets)]
            kf, vf = cl.update_kv(k, q, v)
        torch.cuda.synchronize()
        call_us = (time.perf_counter() - t0) / iters * 1e6
        N.prof_enable(True)
        N.prof_read(reset=True)
        for it in range(iters):
            q, k, v = sets[it % len(sets)]
            cl.update_kv(k, q, v)
        torch.cuda.synchronize()
        prof = N.prof_read(reset=True)
        N.prof_enable(False)
        kus = {k_: round(v_[0] / v_[1] * 1e3 * (v_[1] / iters), 2) for k_, v_ in prof.items() if v_[1]}      # us per CALL (a kernel may run twice)
        ksum = sum(kus.values())
        klen = int(cl.klen_sum)
        # algorithmic bytes: K once per KV head + the w query rows of every query head (score), pooled scores read once by the
        # selection, the flat gather 2 tensors x klen_sum rows x D x e x (read + write)
        alg = Hkv * S * D * E + Hq * W * D * E + Hq * (S - W) * E + 4 * klen * D * E
        row = {"update_kv_us": round(call_us, 2), "kernels_us_per_call": kus, "kernels_sum_us": round(ksum, 2),
               "host_sync_remainder_us": round(call_us - ksum, 2), "klen_sum": klen, "max_seqlen_k": int(cl.max_seqlen_k),
               "list_len": int(cl.ada.prepared.m_use) if cl.ada.prepared is not None else None, "route": cl.ada.route.value, "repeated_calls": cl.ada.repeats,
               "tokens_per_s": round(S / call_us * 1e6, 0),
               "roofline": {"bound": "hbm", "achieved": round(alg / (call_us * 1e-6) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": round(alg / (call_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4), "traffic": None,
                            "algorithmic_bytes": int(alg), "what": "whole call (wall time incl. the host sync) over its algorithmic bytes"},
               "roofline_kernels_only": round(alg / (ksum * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
        if not a.no_parity:
            q, k, v = sets[0]
            kf, vf = cl.update_kv(k, q, v)
            torch.cuda.synchronize()
            qc = q.cpu()
            kx, vx = (t.cpu().repeat_interleave(g, dim=1) for t in (k, v))
            torch.set_num_threads(min(os.cpu_count() or 1, 32))
            with contextlib.redirect_stdout(io.StringIO()):
                kr, vr, meta = O.adakv_update_kv(kx, qc, vx, W, cap, 7, "maxpool", 0.2, True)
            lens, rl_ = cl.head_lens.cpu().tolist(), meta.head_lens.tolist()
            same_lens = lens == rl_
            heads_kv = 0.0
            if same_lens:
                cu = [0] + list(torch.tensor(lens).cumsum(0).tolist())
                kfc, vfc = kf.cpu(), vf.cpu()
                heads_kv = sum(bool(torch.equal(kfc[cu[h]:cu[h + 1]], kr[cu[h]:cu[h + 1]]) and torch.equal(vfc[cu[h]:cu[h + 1]], vr[cu[h]:cu[h + 1]]))
                               for h in range(Hq)) / Hq
            row["parity"] = {"checker": "oracle.adakv_update_kv on the host CPU (K/V expanded by repeat_kv), same tensors",
                             "head_budgets_identical": same_lens, "metadata_identical": same_lens and cl.cu_klen.cpu().tolist() == meta.cu_klen.tolist()
                             and int(cl.klen_sum) == int(meta.klen_sum) and int(cl.max_seqlen_k) == int(meta.max_seqlen_k),
                             "kv_bit_identical_heads": heads_kv,
                             "heads_with_other_budget": sum(x != y for x, y in zip(lens, rl_))}
        res["budget%d" % cap] = row
    del sets
    torch.cuda.empty_cache()
    return res


def merge_extra(P, dt, dev, H):
    """LOOK-M pivot merge (pyramidkv_utils.py:119-170; not `value`): SnapKVCluster(merge="pivot").update_kv next to the plain
    gather at S = 8192 / 32768, budget 128: wall time per call and the merge step's algorithmic bytes (every K row read once
    for the cosine pivots + the dropped K and V rows read once for the scatter-mean) against the HBM roofline."""
    res = {}
    for S in (8192, 32768):
        (q, k, v), = make_sets(1, H, S, dt, dev, 31 + S, 1)
        cap = 128
        plain = P.SnapKVCluster(window_size=W, max_capacity_prompt=cap, kernel_size=7, pooling="maxpool")
        merge = P.SnapKVCluster(window_size=W, max_capacity_prompt=cap, kernel_size=7, pooling="maxpool", merge="pivot")
        idx = P.ops.select(q, k, W, cap - W, "maxpool", 7)

        def timed(fn, iters=10):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters * 1e3
        t_plain = timed(lambda: plain.update_kv(k, q, v, None, 1))
        t_merge = timed(lambda: merge.update_kv(k, q, v, None, 1))
        t_only = timed(lambda: P.ops.merge_compact(k, v, idx, W))
        alg = H * S * D * E * 2                      # K rows (pivot search + merge) and V rows (merge), each read once
        res["S%d_budget%d" % (S, cap)] = {
            "update_kv_plain_us": round(t_plain, 2), "update_kv_merge_us": round(t_merge, 2), "merge_only_us": round(t_only, 2),
            "roofline": {"bound": "hbm", "achieved": round(alg / (t_only * 1e-6) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(alg / (t_only * 1e-6) / 1e9 / HBM_PEAK_GBS, 4), "traffic": None, "algorithmic_bytes": int(alg)}}
        del q, k, v
        torch.cuda.empty_cache()
    return res


def gpu_eager_baseline(dt, dev, S, H, cap):
    """Same-chip comparator: the reference's eager op sequence - the oracle restatement of
    pyramidkv_utils.py:306-347, ``tensor.topk`` as the reference calls it - executed by PyTorch-ROCm on this GPU on the
    same shapes, device time from events on the current stream.  A reported baseline like `cpu_baseline`, never the
    product path."""
    from oracle import pkv_oracle as O
    (q, k, v), = make_sets(1, H, S, dt, dev, 555, 1)
    res = {}
    for budget in (cap, 2048):
        def call():
            with contextlib.redirect_stdout(io.StringIO()):
                return O.snapkv_update_kv(k, q, v, W, budget, 7, "maxpool", topk_mode="reference")
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        iters = 5
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(iters):
            call()
        ev1.record()
        torch.cuda.synchronize()
        us = ev0.elapsed_time(ev1) / iters * 1e3
        res["snapkv_budget%d" % budget] = {"update_kv_us": round(us, 1), "tokens_per_s": round(S / us * 1e6, 0)}
    res["kind"] = "reference op sequence (oracle restatement) on torch %s, device %s" % (torch.__version__, torch.cuda.get_device_name(dev))
    res["workload"] = "[1,%d,%d,128] %s, window 8, maxpool7, one update_kv call" % (H, S, str(dt).replace("torch.", ""))
    return res


def first_contact(dist, backend, world, rank, dev, pdist, ks, B, Hl, a):
    """What the first real multi-GPU run must show before any of its numbers is believed (round-5 review item 8): one distinct
    device per rank (by PCI bus id, gathered over the process group), the RCCL communicator size == N, the node's xGMI
    topology as `rocm-smi --showtopo` prints it, and the all-gather's own latency in BOTH exchange modes (one collective per
    prefill / one per layer).  Raises on a rank / device mismatch: a run that silently shares a GPU is not a measurement."""
    info = {}
    try:
        bus = torch.cuda.get_device_properties(dev).pci_bus_id
    except Exception:       # noqa: BLE001 - older builds: no bus id on the properties object
        bus = None
    ident = "%s/%s/bus%s" % (socket.gethostname(), torch.cuda.get_device_name(dev), bus if bus is not None else "?%d" % dev.index)
    idents = [None] * world
    dist.all_gather_object(idents, (rank, dev.index, ident))
    info["ranks"] = [{"rank": r, "device_index": d, "device": i} for r, d, i in sorted(idents)]
    distinct = len({(d, i) for _, d, i in idents}) == world
    info["one_distinct_device_per_rank"] = distinct
    if backend == "nccl":
        assert dist.get_world_size() == a.gpus, "RCCL communicator has %d ranks, --gpus %d" % (dist.get_world_size(), a.gpus)
        # only a KNOWN clash is fatal: without bus ids (bus "?n") ranks that were each given one visible device all report index 0
        known = all("bus?" not in i for _, _, i in idents)
        assert distinct or not known, "two ranks share a device: %s" % (idents,)
        if not distinct:
            info["one_distinct_device_per_rank"] = "unknown (no PCI bus ids on this torch build)"
    # both exchange modes of the selected indices, alone on the device: the whole prefill's buffer once / one layer's indices
    def timed(fn, n=20):
        fn()
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6
    xch = pdist.PrefillIndexExchange(ks, B, Hl, dev, force=True)
    one = torch.zeros(B, Hl, ks[0], dtype=torch.int32, device=dev)
    info["allgather_us_by_mode"] = {"prefill (one collective, all 32 layers' indices)": round(timed(lambda: xch.views(xch.gather_async())), 1),
                                    "layer (one collective per layer, k = %d)" % ks[0]: round(timed(lambda: pdist.allgather_indices_async(one, force=True).wait()), 1)}
    if rank == 0:
        try:
            r = subprocess.run(["rocm-smi", "--showtopo"], capture_output=True, text=True, timeout=20)
            info["rocm_smi_showtopo"] = [ln for ln in r.stdout.splitlines() if ln.strip() and not ln.startswith("=")][:80]
        except Exception as e:      # noqa: BLE001
            info["rocm_smi_showtopo"] = "unavailable: %s" % e
    return {"first_contact": info}


def three_way_block(P, dev, S, H):
    """`parity.vs_device_reference` (round-5 review item 1): libpkv vs the reference's op sequence on the host CPU vs the SAME op
    sequence on PyTorch-ROCm eager on this GPU, on one seeded [1,H,S,128] set in bf16 and fp16, for the budgets of PyramidKV's
    first / last layer and SnapKV 128 / 2048 (tests/three_way.py; the full grid is profiles/r06/parity_three_way.json).  Per
    pair: fraction of heads with the identical index set / sequence / K,V bits; against the device reference libpkv runs with
    scale "rcp" + tie order "aten_rocm" (what ATen's HIP kernels do), against the CPU reference with its defaults."""
    import three_way as T3
    from inputs import make_qkv
    out = {"checker": "tests/three_way.py: oracle/pkv_oracle.py on CPU tensors (cpu) and on HIP tensors (eager = PyTorch-ROCm's own kernels)"}
    for dname in ("bf16", "fp16"):
        q, k, v = make_qkv(1, H, S, D, dname, "gauss", 6300)
        rep = T3.window_policy(P, q, k, v, W, {"pyramid_layer0_k234": 234, "pyramid_layer31_k17": 17, "snapkv_budget128": 120,
                                               "snapkv_budget2048": 2040}, dev=dev)
        out[dname] = T3.summarise(rep)
        b = rep["budgets"]["snapkv_budget2048"]
        out[dname]["budget2048_heads_in_another_order"] = {p_: b[p_]["heads"] - b[p_]["identical_sequence"]
                                                           for p_ in ("hip_vs_cpu", "hip_vs_eager", "eager_vs_cpu")}
    return out


def _call_us(fn, sets, iters=10, reps=3):
    """device time per call between two events around `iters` back-to-back calls, fastest of `reps` rounds (one host hiccup -
    a page fault, an allocator refill - inside a 10-call window otherwise shows up as milliseconds)"""
    for it in range(3):
        fn(*sets[it % len(sets)])
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for it in range(iters):
            fn(*sets[it % len(sets)])
        ev1.record()
        torch.cuda.synchronize()
        us = ev0.elapsed_time(ev1) / iters * 1e3
        best = us if best is None or us < best else best
    return best


def _kernel_us(N, fn, sets, iters=10):
    N.prof_enable(True)
    N.prof_read(reset=True)
    for it in range(iters):
        fn(*sets[it % len(sets)])
    torch.cuda.synchronize()
    prof = N.prof_read(reset=True)
    N.prof_enable(False)
    return {k_: round(v_[0] / v_[1] * 1e3, 2) for k_, v_ in prof.items() if v_[1]}


def _sel_parity(P, q, k, v, w, kk, pooling, ksz, idx, kc, vc):
    """heads with the oracle's index set / sequence / K,V bits for one dense selection (canonical tie order)."""
    from oracle import pkv_oracle as O
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    qc, kc_, vc_ = q[:1].cpu(), k[:1].cpu(), v[:1].cpu()
    with contextlib.redirect_stdout(io.StringIO()):
        s = O.pool_scores(O.window_scores(qc, kc_, w), pooling, ksz)
    ridx = O.topk_canonical(s, kk)
    kr, vr = O.gather_compact(kc_, vc_, ridx, w)
    ia = idx[:1].cpu().long()
    kth = torch.gather(s, -1, ridx[..., kk - 1:kk])
    return {"heads_identical_set": float((torch.sort(ia, -1).values == torch.sort(ridx, -1).values).all(-1).float().mean()),
            "heads_identical_sequence": float((ia == ridx).all(-1).float().mean()),
            "kv_bit_identical_heads": float(((kc[:1].cpu() == kr).flatten(2).all(-1) & (vc[:1].cpu() == vr).flatten(2).all(-1)).float().mean()),
            "ties_at_kth_value_mean": float((s == kth).sum(-1).float().mean())}


def robust_extra(P, N, dev, S, H, a):
    """Real-distribution leg (round-5 review item 5; not `value`): the same calls on `make_qkv(kind="sink")` inputs in fp16 -
    logits with std 6 and an attention-sink key every window query scores at +40, so that all but a few hundred pooled scores
    per head underflow to exactly 0 and the k-th largest value is tied tens of thousands of times (topk_kernel leaves its
    small-k prefilter for the general path, pkv_topk.hip "heavy ties") - next to the same calls on fp16 N(0,1) inputs: wall
    time per call, device time per kernel, the sink / gauss ratio, and a parity block against the CPU oracle.  H2O: both passes
    on sink data at S (pass 1 decides tracked vs frozen from a 16-key look, pkv_h2o.hip) and parity at S = 8192 on 4 heads."""
    from inputs import make_qkv
    from oracle import pkv_oracle as O
    res = {"inputs": "tests/inputs.py make_qkv(kind='sink'): fp16, [1,%d,%d,128], logit std 6, sink key at position 0 scored +40 by the last 64 queries" % (H, S)}
    legs = {}
    for kind in ("gauss", "sink"):
        q, k, v = (t.to(dev) for t in make_qkv(1, H, S, D, "fp16", kind, 6600))
        sets = [(q, k, v)]
        row = {}
        for cap in (128, 2048):
            kk = cap - W
            fn = lambda q_, k_, v_: P.ops.compress(q_, k_, v_, W, kk, "maxpool", 7)       # noqa: E731
            r = {"update_kv_us": round(_call_us(fn, sets), 2), "kernels_us": _kernel_us(N, fn, sets)}
            if kind == "sink" and not a.no_parity:
                kc, vc, idx = P.ops.compress(q, k, v, W, kk, "maxpool", 7, return_indices=True)
                r["parity"] = _sel_parity(P, q, k, v, W, kk, "maxpool", 7, idx, kc, vc)
            row["snapkv_budget%d" % cap] = r
        fn = lambda q_, k_, v_: P.ops.score_h2o(q_, k_, W)                                # noqa: E731
        ku = _kernel_us(N, fn, sets, iters=3)
        row["h2o_scores"] = {"stats_ms": round(ku.get("h2o_stats", 0) / 1e3, 3), "colsum_ms": round(ku.get("h2o_colsum", 0) / 1e3, 3)}
        legs[kind] = row
        del q, k, v, sets
        torch.cuda.empty_cache()
    res.update(legs)
    res["sink_over_gauss"] = {
        "snapkv_budget128": round(legs["sink"]["snapkv_budget128"]["update_kv_us"] / legs["gauss"]["snapkv_budget128"]["update_kv_us"], 3),
        "snapkv_budget2048": round(legs["sink"]["snapkv_budget2048"]["update_kv_us"] / legs["gauss"]["snapkv_budget2048"]["update_kv_us"], 3),
        "topk_kernel_budget2048": round(legs["sink"]["snapkv_budget2048"]["kernels_us"].get("topk", 0) / max(1e-9, legs["gauss"]["snapkv_budget2048"]["kernels_us"].get("topk", 0)), 3),
        "h2o_scores": round((legs["sink"]["h2o_scores"]["stats_ms"] + legs["sink"]["h2o_scores"]["colsum_ms"])
                            / max(1e-9, legs["gauss"]["h2o_scores"]["stats_ms"] + legs["gauss"]["h2o_scores"]["colsum_ms"]), 3)}
    if not a.no_parity:                      # H2O on sink data against the materialised S x S oracle: S = 8192, 4 heads
        q, k, v = make_qkv(1, 4, 8192, D, "fp16", "sink", 6601)
        torch.set_num_threads(min(os.cpu_count() or 1, 32))
        want = O.h2o_scores_blocked(q, k, W, block=512)
        got = P.ops.score_h2o(q.to(dev), k.to(dev), W).cpu()
        b_g, b_w = (t.view(torch.int16).int() & 0xffff for t in (got, want))
        d_ = (torch.where(b_g >= 0x8000, -(b_g & 0x7fff), b_g) - torch.where(b_w >= 0x8000, -(b_w & 0x7fff), b_w)).abs()
        kc, vc, idx = P.ops.compress(q.to(dev), k.to(dev), v.to(dev), W, 120, None, 1, h2o=True, return_indices=True)
        ridx = O.topk_canonical(want, 120)
        normal = want.float().abs() >= 2.0 ** -14           # below it fp16 is subnormal: one "ulp" is the absolute step 2^-24, and every
        #                                                        probability that flips between 0 and 2^-24 moves the column sum by one step
        res["h2o_parity_S8192_4heads"] = {"score_mismatch_frac": round(float((d_ > 0).float().mean()), 7), "score_max_ulp": int(d_.max()),
                                         "score_max_ulp_normal_range": int(d_[normal].max()) if bool(normal.any()) else 0,
                                         "scores_in_subnormal_range_frac": round(float((~normal).float().mean()), 4),
                                         "heads_identical_set_budget128": float((torch.sort(idx.cpu().long(), -1).values == torch.sort(ridx, -1).values).all(-1).float().mean())}
    return res


def baseline_grid_extra(P, N, rl, alg_bytes, kernel_rows, a, dev, S, H):
    """BASELINE.md section 3's grid rows the headline / `grid` / `sweep` do not carry (round-5 review item 6; not `value`): the
    fp16 twin of the headline step (every reference runner's dtype, run_longbench.py:388), the `init_*` default knobs
    (window 32, avgpool-5, pyramidkv_utils.py:885-890), budget 64 (BASELINE config 1's budget), and StreamingLLM - each as one
    timed workload with per-kernel device time and a parity block."""
    res = {}
    f16 = torch.float16
    # fp16 twin of the headline: 32 PyramidKV layer budgets, 4 rotating sets
    ks = layer_budgets(P, "pyramidkv", 128, W, S)
    clusters = make_clusters(P, "pyramidkv", 128)
    sets = make_sets(1, H, S, f16, dev, 4242, 4)
    slots = [torch.empty(1, H, ks[layer], dtype=torch.int32, device=dev) for layer in range(NUM_LAYERS)]

    def step(keep=None):
        for layer in range(NUM_LAYERS):
            q, k, v = sets[layer % len(sets)]
            cl = clusters[layer]
            cl.index_out = slots[layer]
            kc, vc = cl.update_kv(k, q, v, None, 1)
            if keep is not None and layer in keep:
                keep[layer] = (kc, vc, slots[layer].clone())
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    steps = max(5, a.steps)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    N.prof_enable(True)
    N.prof_read(reset=True)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    prof = N.prof_read(reset=True)
    N.prof_enable(False)
    rows = kernel_rows(prof, alg_bytes(1, H, S, sum(ks) / NUM_LAYERS))
    row = {"workload": "pyramidkv budget=128 window=8 maxpool7, 32 update_kv calls/step, [1,%d,%d,128] fp16" % (H, S),
           "ms_per_step": round(el / steps * 1e3, 4), "tokens_per_s": round(S * steps / el, 1),
           "kernels_us": {k_: r["avg_us"] for k_, r in rows.items()}, "roofline": rows.get("logits")}
    if not a.no_parity:
        keep = {0: None, NUM_LAYERS - 1: None}
        step(keep)
        torch.cuda.synchronize()
        row["parity"] = parity_block_for(keep, sets, ks, 128, "pyramidkv", "fp16", S)
    res["headline_fp16"] = row
    del sets, slots
    torch.cuda.empty_cache()

    # the init_* defaults (window 32, avgpool-5) and budget 64, bf16, one SnapKV call each; StreamingLLM (no scoring)
    bf = torch.bfloat16
    sets = make_sets(1, H, S, bf, dev, 4343, 2)
    for name, w_, cap, pool, ksz in (("init_defaults_window32_avgpool5_budget128", 32, 128, "avgpool", 5),
                                     ("init_defaults_window32_avgpool5_budget2048", 32, 2048, "avgpool", 5),
                                     ("budget64_window8_maxpool7", 8, 64, "maxpool", 7)):
        cl = P.SnapKVCluster(window_size=w_, max_capacity_prompt=cap, kernel_size=ksz, pooling=pool)
        fn = lambda q_, k_, v_: cl.update_kv(k_, q_, v_, None, 1)                        # noqa: E731
        us = _call_us(fn, sets)
        r = {"policy": "snapkv", "window": w_, "budget": cap, "pooling": "%s-%d" % (pool, ksz), "S": S, "dtype": "bf16",
             "update_kv_us": round(us, 2), "tokens_per_s": round(S / us * 1e6, 0), "kernels_us": _kernel_us(N, fn, sets)}
        if not a.no_parity:
            q, k, v = sets[0]
            kc, vc, idx = P.ops.compress(q, k, v, w_, cap - w_, pool, ksz, return_indices=True)
            r["parity"] = _sel_parity(P, q, k, v, w_, cap - w_, pool, ksz, idx, kc, vc)
        res[name] = r
    # PyramidKV budget 64: the 32 layer budgets 110 ... 17 of BASELINE config 1 at the headline length
    ks64 = layer_budgets(P, "pyramidkv", 64, W, S)
    cl64 = [P.PyramidKVCluster(num_hidden_layers=NUM_LAYERS, layer_idx=layer, window_size=W, max_capacity_prompt=64, kernel_size=7, pooling="maxpool")
            for layer in range(NUM_LAYERS)]

    def step64():
        for layer in range(NUM_LAYERS):
            q, k, v = sets[layer % len(sets)]
            cl64[layer].update_kv(k, q, v, None, 1)
    for _ in range(2):
        step64()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step64()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    res["pyramidkv_budget64"] = {"layer_budgets": "%d ... %d" % (ks64[0], ks64[-1]), "ms_per_step": round(el / steps * 1e3, 4),
                                 "tokens_per_s": round(S * steps / el, 1)}
    st = P.StreamingLLMKVCluster(window_size=124, max_capacity_prompt=128)              # the runners' w = cap - 4 (run_longbench.py:222-223)
    us = _call_us(lambda q_, k_, v_: st.update_kv(k_, q_, v_, None, 1), sets)
    res["streamingllm_budget128"] = {"update_kv_us": round(us, 2), "tokens_per_s": round(S / us * 1e6, 0)}
    del sets
    torch.cuda.empty_cache()
    return res


def e2e_prefill_extra(P, N, dev):
    """The metric's "prefill tokens/s" on a model with Llama-3-8B's dimensions (round-5 review item 4; not `value`): random-init
    LlamaForCausalLM, 32 layers, hidden 4096, 32 / 8 heads, D = 128, intermediate 14336, bf16, small vocabulary (no weights on
    disk), prefill of one sequence through `replace_llama("pyramidkv")` (budget 128, window 8, maxpool-7) at S = 8192 and
    32768: tokens/s with eviction OFF (the stock attention), ON in the reference's order (repeat_kv first, llama_model.py:158-168)
    and ON with K/V handed over before repeat_kv; `update_kv_share` = the 32 update_kv calls' kernel time / the prefill's wall
    time.  The attention itself is PyTorch SDPA: the model is the caller of this path, not part of it."""
    try:
        from transformers import LlamaConfig, LlamaForCausalLM, DynamicCache
    except Exception as e:      # noqa: BLE001
        return {"skipped": "transformers unavailable: %s" % e}
    from pyramidkv_amd import monkeypatch as mp
    cfg = LlamaConfig(vocab_size=1024, hidden_size=4096, intermediate_size=14336, num_hidden_layers=NUM_LAYERS, num_attention_heads=32,
                      num_key_value_heads=8, head_dim=128, max_position_embeddings=65536, rope_theta=500000.0)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        torch.manual_seed(0)
        with torch.device(dev):
            model = LlamaForCausalLM(cfg).eval()
    finally:
        torch.set_default_dtype(old)
    res = {"model": "random-init Llama, Llama-3-8B dimensions (32 layers, hidden 4096, 32/8 heads, D 128, MLP 14336), bf16, vocab 1024, SDPA attention",
           "policy": "pyramidkv budget=128 window=8 maxpool7"}

    def prefill(ids):
        with torch.no_grad():
            model(ids, past_key_values=DynamicCache(config=cfg), use_cache=True, logits_to_keep=1)

    def timed(ids, n=2):
        prefill(ids)
        torch.cuda.synchronize()
        best = None
        for _ in range(n):
            t0 = time.perf_counter()
            prefill(ids)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            best = t if best is None or t < best else best
        return best
    try:
        for S in (8192, 32768):
            ids = torch.randint(0, 1024, (1, S), device=dev)
            row = {}
            t_off = timed(ids)
            row["eviction_off"] = {"prefill_ms": round(t_off * 1e3, 2), "tokens_per_s": round(S / t_off, 0)}
            for label, skip in (("eviction_on_reference_order", False), ("eviction_on_skip_repeat_kv", True)):
                mp.replace_llama("pyramidkv")
                mp.skip_repeat_kv = skip
                for layer in model.model.layers:
                    c = layer.self_attn.config
                    c.window_size, c.max_capacity_prompt, c.kernel_size, c.pooling, c.merge = W, 128, 7, "maxpool", None
                t_on = timed(ids)
                N.prof_enable(True)
                N.prof_read(reset=True)
                prefill(ids)
                torch.cuda.synchronize()
                prof = N.prof_read(reset=True)
                N.prof_enable(False)
                kms = sum(v_[0] for v_ in prof.values())
                row[label] = {"prefill_ms": round(t_on * 1e3, 2), "tokens_per_s": round(S / t_on, 0),
                              "update_kv_kernels_ms_all_32_layers": round(kms, 3), "update_kv_share": round(kms / (t_on * 1e3), 5),
                              "vs_eviction_off": round(t_on / t_off, 4)}
                mp.restore()
            res["S%d" % S] = row
            del ids
    finally:
        mp.skip_repeat_kv = True
        mp.restore()
        del model
        torch.cuda.empty_cache()
    return res


_REF = {}


def reference_module():
    """pyramidkv/pyramidkv_utils.py of the real reference, imported when /root/reference exists on this box (the build
    container; never the GPU boxes) - BASELINE.md section 3: "imported when present, else the restatement"."""
    if "mod" not in _REF:
        mod = None
        ref = os.environ.get("PKV_REFERENCE_ROOT", "/root/reference")
        if os.path.exists(os.path.join(ref, "pyramidkv", "pyramidkv_utils.py")):
            try:
                sys.path.insert(0, ref)
                import importlib
                mod = importlib.import_module("pyramidkv.pyramidkv_utils")
            except Exception:       # noqa: BLE001 - an unusable checkout is the same as none
                mod = None
        _REF["mod"] = mod
    return _REF["mod"]


def _cpu_time(fn, seconds):
    """best and median of up to 5 timed calls after one warm-up, bounded by ~`seconds` of CPU work"""
    with contextlib.redirect_stdout(io.StringIO()):
        t0 = time.perf_counter()
        fn()
        first = time.perf_counter() - t0
        ts = []
        while len(ts) < 5 and (sum(ts) + first < seconds or len(ts) < 1):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[0], ts[len(ts) // 2], len(ts)


def cpu_baselines_more(P, dev, a):
    """Time-boxed host-core baselines for the BASELINE configurations other than the headline (round-5 review item 6): SnapKV
    budget 2048 at S = 32768, H2O at S = 4096 (the largest the unmodified reference runs: it materialises S x S) and Ada-SnapKV at
    S = 8192 - the reference's own update_kv when /root/reference is on this box (`kind: "reference"`), else the bit-pinned
    restatement (`"port"`) - each next to the same call through libpkv on this GPU."""
    from oracle import pkv_oracle as O
    from inputs import make_qkv
    ref = reference_module()
    ncpu = os.cpu_count() or 1
    nt = min(ncpu, 64)
    torch.set_num_threads(nt)
    kind = "reference" if ref is not None else "port"
    out = {"kind": kind, "cores": nt, "host_logical_cpus": ncpu,
           "what": ("pyramidkv/pyramidkv_utils.py imported from /root/reference" if ref is not None else
                    "oracle/pkv_oracle.py (== the reference bit for bit on the committed fixtures)") + ", torch.set_num_threads(%d), stdout suppressed" % nt}
    dname = a.dtype

    def gpu_us(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / 5 * 1e6
    # SnapKV budget 2048, S = 32768
    q, k, v = make_qkv(1, 32, 32768, D, dname, "gauss", 1234)
    if ref is not None:
        cl = ref.SnapKVCluster(window_size=W, max_capacity_prompt=2048, kernel_size=7, pooling="maxpool")
        f = lambda: cl.update_kv(k, q, v, None, 1)                                           # noqa: E731
    else:
        f = lambda: O.snapkv_update_kv(k, q, v, W, 2048, 7, "maxpool", topk_mode="reference")  # noqa: E731
    best, med, n = _cpu_time(f, a.cpu_seconds / 3)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    hcl = P.SnapKVCluster(window_size=W, max_capacity_prompt=2048, kernel_size=7, pooling="maxpool")
    out["snapkv_budget2048_S32768"] = {"cpu_ms": round(best * 1e3, 2), "cpu_ms_median": round(med * 1e3, 2), "calls": n, "cpu_tokens_per_s": round(32768 / best, 0),
                                       "libpkv_us": round(gpu_us(lambda: hcl.update_kv(kd, qd, vd, None, 1)), 2)}
    # H2O, S = 4096
    q, k, v = make_qkv(1, 32, 4096, D, dname, "gauss", 1235)
    if ref is not None:
        cl = ref.H2OKVCluster(window_size=W, max_capacity_prompt=128, kernel_size=7, pooling="maxpool")
        f = lambda: cl.update_kv(k, q, v, None, 1)                                           # noqa: E731
    else:
        f = lambda: O.h2o_update_kv(k, q, v, W, 128, topk_mode="reference")                  # noqa: E731
    best, med, n = _cpu_time(f, a.cpu_seconds / 3)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    hcl = P.H2OKVCluster(window_size=W, max_capacity_prompt=128, kernel_size=7, pooling="maxpool")
    out["h2o_budget128_S4096"] = {"cpu_ms": round(best * 1e3, 2), "cpu_ms_median": round(med * 1e3, 2), "calls": n, "cpu_tokens_per_s": round(4096 / best, 0),
                                  "libpkv_us": round(gpu_us(lambda: hcl.update_kv(kd, qd, vd, None, 1)), 2),
                                  "note": "the largest S the unmodified reference runs: it materialises [1,32,S,S] (:544,553)"}
    # Ada-SnapKV, S = 8192 (floor 0.2, normalize; K/V expanded as the reference receives them)
    q, k, v = make_qkv(1, 32, 8192, D, dname, "gauss", 1236)
    if ref is not None:
        cl = ref.AdaKVCluster(window_size=W, kernel_size=7, pooling="maxpool", max_capacity_prompt=128, floor=0.2, normalize=True,
                              layer_idx=0, num_hidden_layers=NUM_LAYERS)
        f = lambda: cl.update_kv(k, q, v)                                                    # noqa: E731
    else:
        f = lambda: O.adakv_update_kv(k, q, v, W, 128, 7, "maxpool", 0.2, True, sort_mode="reference")   # noqa: E731
    best, med, n = _cpu_time(f, a.cpu_seconds / 3)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    hcl = P.AdaKVCluster(window_size=W, kernel_size=7, pooling="maxpool", max_capacity_prompt=128, floor=0.2, normalize=True,
                         layer_idx=0, num_hidden_layers=NUM_LAYERS)
    out["adakv_budget128_S8192"] = {"cpu_ms": round(best * 1e3, 2), "cpu_ms_median": round(med * 1e3, 2), "calls": n, "cpu_tokens_per_s": round(8192 / best, 0),
                                    "libpkv_us": round(gpu_us(lambda: hcl.update_kv(kd, qd, vd)), 2)}
    return out



def cpu_baseline(qkv, ks, w, cap, a):
    """The reference's eager path (oracle restatement == pyramidkv_utils.py:197-283 executed by PyTorch CPU) on
    the host cores of this node, same tensors moved to the CPU.  Bounded sample: a few of the 32 layer-calls,
    thread count chosen by a one-call probe over {all cores, 64, 16} (the fastest is reported in `cores`)."""
    from oracle import pkv_oracle as O
    q, k, v = (t[:1].cpu() for t in qkv)        # one sequence, this rank's heads
    ncpu = os.cpu_count() or 1
    S = q.shape[2]
    n = max(1, min(a.cpu_layers, NUM_LAYERS))
    layers = [round(i * (NUM_LAYERS - 1) / max(1, n - 1)) for i in range(n)] if n > 1 else [0]

    ref = reference_module()           # the reference's own file when this box has it, else the restatement
    ref_clusters = None
    if ref is not None:
        ref_clusters = [ref.PyramidKVCluster(num_hidden_layers=NUM_LAYERS, layer_idx=layer, window_size=w, max_capacity_prompt=cap, kernel_size=7,
                                             pooling="maxpool") if a.policy == "pyramidkv" else
                        ref.SnapKVCluster(window_size=w, max_capacity_prompt=cap, kernel_size=7, pooling="maxpool") for layer in range(NUM_LAYERS)]

    def run(ls):
        t0 = time.perf_counter()
        for layer in ls:
            with contextlib.redirect_stdout(io.StringIO()):
                if ref_clusters is not None:
                    ref_clusters[layer].update_kv(k, q, v, None, 1)
                elif a.policy == "pyramidkv":
                    O.pyramidkv_update_kv(k, q, v, w, cap, 7, "maxpool", NUM_LAYERS, layer, topk_mode="reference")
                else:
                    O.snapkv_update_kv(k, q, v, w, cap, 7, "maxpool", topk_mode="reference")
        return time.perf_counter() - t0

    best_t, best_n = None, None
    for nt in sorted({ncpu, min(ncpu, 64), min(ncpu, 16)}, reverse=True):
        torch.set_num_threads(nt)
        run([0])                         # warm-up at this thread count
        t = run([0])
        if best_t is None or t < best_t:
            best_t, best_n = t, nt
    torch.set_num_threads(best_n)
    # bounded sample: whole passes over the chosen layer-calls until ~cpu_seconds of CPU work; the fastest pass counts
    # (the host is shared with the GPU driver threads, single passes scatter by 2x)
    t, spent, passes = None, 0.0, 0
    while spent < a.cpu_seconds or passes < 2:
        tp = run(layers)
        spent += tp
        passes += 1
        t = tp if t is None or tp < t else t
    model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    gold = os.path.join(ROOT, "tests", "golden", "index.json")
    nfix = len(json.load(open(gold)).get("cases", [])) if os.path.exists(gold) else 0
    return {"value": round(S * len(layers) / NUM_LAYERS / t, 1), "unit": "tokens/s", "cores": best_n, "kind": "reference" if ref is not None else "port",
            "reference_file": "/root/reference/pyramidkv/pyramidkv_utils.py (imported)" if ref is not None else "absent on this box: the bit-pinned restatement runs instead",
            "port_checked_against": "oracle/pkv_oracle.py == the real reference (pyramidkv/pyramidkv_utils.py, imported) bit-for-bit on "
                                    "%d committed fixtures (tests/golden/, tests/test_oracle_golden.py)" % nfix,
            "sample": "%d of the 32 layer-calls per pass (layers %s) of the same workload ([1,%d,%d,128] %s), %d passes = %.1f s "
                      "of CPU work, fastest pass %.2f s; host has %d logical CPUs, thread count picked by a 1-call probe"
                      % (len(layers), layers if len(layers) < NUM_LAYERS else "0..31", q.shape[1], S, a.dtype, passes, spent, t, ncpu),
            "ms_per_layer": round(t / len(layers) * 1e3, 3), "cpu": model}


if __name__ == "__main__":
    main()
