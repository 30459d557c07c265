"""Runs ON THE GPU BOX under rocprofv3 --kernel-trace --stats: kernel times of MiniROADA streaming (MROADA.step: the streaming step's
launches plus stream_ant_hidden / stream_ant_head), bf16, zero flow, 20 + 300 frames of n streams at anticipation_length L - one (L, n)
per run, so that the tool's per-kernel averages are not mixed.  usage: python scripts/probes/ant_step_profile.py L n"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from prego_amd import weights as W
from prego_amd.config import anticipation_cfg, assembly101_cfg
from prego_amd.registry import build_model
import prego_amd.model  # noqa: F401
L, n = int(sys.argv[1]), int(sys.argv[2])
cfg = anticipation_cfg(assembly101_cfg(compute_dtype="bf16", assume_zero_flow=True), L)
m = build_model(cfg, "cuda:0")
m.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0).items()})
m.eval()
x = torch.randn(n, 2048, device="cuda").clamp_(min=0)
h = torch.zeros(n, 1024, device="cuda")
for _ in range(320):
    m.step(x, None, h)
torch.cuda.synchronize()
m.check()
print(f"L={L} n={n}: done")
