"""Runs ON THE GPU BOX under rocprofv3 --kernel-trace --stats: kernel times of the wide streaming step (step_wide: wide_cast, wide_gemv x 2,
ln_relu_rows, stream_gates_head, wide_ant_hidden, wide_ant_head; csrc/stream_wide.hip), bf16, zero flow, 20 + 300 frames of n streams -
one (L, n) per run, so that the tool's per-kernel averages are not mixed; L = 0 is MiniROAD.  usage: python scripts/probes/step_wide_profile.py L n"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from prego_amd import weights as W
from prego_amd.config import anticipation_cfg, assembly101_cfg
from prego_amd.registry import build_model
import prego_amd.model  # noqa: F401
L, n = int(sys.argv[1]), int(sys.argv[2])
base = assembly101_cfg(compute_dtype="bf16", assume_zero_flow=True)
cfg = anticipation_cfg(base, L) if L else base
sd = W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0) if L else W.miniroad_state_dict(cfg, 20, head_gain=8.0)
m = build_model(cfg, "cuda:0")
m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
m.eval()
x = torch.randn(n, 2048, device="cuda").clamp_(min=0)
h = torch.zeros(n, 1024, device="cuda")
for _ in range(320):
    m.step_wide(x, None, h)
torch.cuda.synchronize()
m.check()
print(f"L={L} n={n}: done")
