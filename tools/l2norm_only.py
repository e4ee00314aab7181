"""The kernels of one L2NormCluster.update_kv and of the window-score K scan on the same K tensor, for a profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/l2norm_only.py [g] [cap] [calls]

[1, 32, 32768, 128] bf16, K/V with 32 / g heads.  The kernel-stats table then holds l2norm_kernel, the top-k, idx_expand_kernel
(g > 1), gather_kernel and logits2_kernel `calls` + 3 times each."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pyramidkv_amd as P  # noqa: E402

g = int(sys.argv[1]) if len(sys.argv) > 1 else 1
cap = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 20
gen = torch.Generator(device="cuda").manual_seed(0)
q = torch.randn(1, 32, 32768, 128, device="cuda", generator=gen).to(torch.bfloat16)
k = torch.randn(1, 32 // g, 32768, 128, device="cuda", generator=gen).to(torch.bfloat16)
v = torch.randn(1, 32 // g, 32768, 128, device="cuda", generator=gen).to(torch.bfloat16)
cl = P.L2NormCluster(max_capacity_prompt=cap, layer_idx=2, skip_layers=[0, 1])
for _ in range(calls + 3):
    cl.update_kv(k, q, v, None, g)
    P.ops.score_window(q, k, 8, "maxpool", 7, "sum", kv_group=g)
torch.cuda.synchronize()
