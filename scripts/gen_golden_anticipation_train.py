#!/usr/bin/env python3
"""Generate tests/golden/g13* (MiniROADA training) by importing the reference model, loss and trainer with the import stubs of
oracle/gen_golden.py.

Only data is written: weights and inputs are regenerated from seeds by prego_amd/weights.py; the fixtures hold the reference's outputs,
sampled like g4b (norm + 256 evenly spaced values per tensor) where a whole tensor would be large.

    python scripts/gen_golden_anticipation_train.py
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle.gen_golden import OUT, _load, _stub_modules, make_targets     # noqa: E402
from prego_amd import weights as W                                        # noqa: E402
from prego_amd.config import anticipation_cfg, assembly101_cfg           # noqa: E402

# (tag, hidden_dim, L, B, T, zero flow, actionness, loss): the batches of g13a..d (and g13e's, which is g13a's)
CASES = {"g13a": (1024, 4, 2, 8, False, True, "ant"), "g13b": (1024, 8, 16, 128, True, False, "ant"),
         "g13c": (512, 1, 2, 8, False, False, "ant"), "g13d": (512, 3, 2, 8, False, False, "dense")}


def case_cfg(tag):
    H, L, B, T, zf, act, _ = CASES[tag]
    return anticipation_cfg(assembly101_cfg(hidden_dim=H, dropout=0.0), L, actionness=act)


def case_batch(tag):
    """rgb, flow [B, T, 2048], target [B, T, C] (unused by OadAntLoss), ant_target [B, L, C] (one-hot), as numpy"""
    H, L, B, T, zf, act, _ = CASES[tag]
    rgb = W.tsn_features((B, T, 2048), 20, f"{tag}.rgb")
    flow = np.zeros_like(rgb) if zf else W.tsn_features((B, T, 2048), 20, f"{tag}.flow")
    return rgb, flow, make_targets(B, T, 86, 20, f"{tag}.tgt"), make_targets(B, L, 86, 20, f"{tag}.ant")


def dense_weights(tag):
    """g13d's loss weights: loss = sum(logits * wl) + sum(anticipation_logits * wa)"""
    H, L, B, T, zf, act, _ = CASES[tag]
    return W.normal((B, T, 86), 20, f"{tag}.wl"), W.normal((B, T, L, 86), 20, f"{tag}.wa")


def sample(a):
    """norm (fp64) + 256 evenly spaced flat indices and their values"""
    a = np.asarray(a, np.float32).reshape(-1)
    idx = np.linspace(0, a.size - 1, min(256, a.size)).astype(np.int64)
    return np.float64(np.linalg.norm(a.astype(np.float64))), idx, a[idx].copy()


def _put(save, name, a):
    save["norm." + name], save["idx." + name], save["val." + name] = sample(a)


def grad_cases():
    from criterions.loss import OadAntLoss
    from model import build_model
    for tag in CASES:
        cfg = case_cfg(tag)
        model = _load(build_model(cfg, "cpu"), W.miniroad_a_state_dict(cfg, 20)).train()
        rgb, flow, tgt, ant = case_batch(tag)
        out = model(torch.from_numpy(rgb), torch.from_numpy(flow))
        if CASES[tag][6] == "ant":
            loss = OadAntLoss(cfg)(out, torch.from_numpy(tgt), torch.from_numpy(ant))
        else:
            wl, wa = dense_weights(tag)
            loss = (out["logits"] * torch.from_numpy(wl)).sum() + (out["anticipation_logits"] * torch.from_numpy(wa)).sum()
        loss.backward()
        save = {"loss": np.float64(float(loss))}
        _put(save, "out.logits", out["logits"].detach().numpy())
        _put(save, "out.anticipation_logits", out["anticipation_logits"].detach().numpy())
        if tag == "g13b":
            save["last_ant"] = out["anticipation_logits"][:, -1].detach().numpy().astype(np.float32)
        no_grad = []
        for k, p in model.named_parameters():
            if p.grad is None:
                no_grad.append(k)
                continue
            _put(save, "grad." + k, p.grad.numpy())
        save["no_grad"] = np.array(no_grad)
        np.savez_compressed(os.path.join(OUT, f"{tag}_mroada_train.npz"), **save)
        print(tag, "loss", float(loss), "no grad:", no_grad)


def adamw_case():
    """g13e: 3 torch.optim.AdamW steps (lr 1e-4, wd 0.05, main.py:62-67) on g13a's batch"""
    from criterions.loss import OadAntLoss
    from model import build_model
    cfg = case_cfg("g13a")
    model = _load(build_model(cfg, "cpu"), W.miniroad_a_state_dict(cfg, 20)).train()
    opt = torch.optim.AdamW([{"params": model.parameters(), "initial_lr": 1e-4}], lr=1e-4, weight_decay=0.05)
    rgb, flow, tgt, ant = (torch.from_numpy(x) for x in case_batch("g13a"))
    losses = []
    for _ in range(3):
        loss = OadAntLoss(cfg)(model(rgb, flow), tgt, ant)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    save = {"losses": np.array(losses, np.float64)}
    for k, p in model.named_parameters():
        _put(save, "param." + k, p.detach().numpy())
    np.savez_compressed(os.path.join(OUT, "g13e_mroada_adamw.npz"), **save)
    print("g13e losses", losses)


def epoch_cfg(root):
    """g13f: make_tree's TVSeries anticipation layer (H 512, C 5, L 3, window 8, stride 4), dropout 0"""
    from scripts.gen_golden_anticipation import make_tree
    return dict(make_tree(root), dropout=0.0)


def epoch_case():
    """g13f: one epoch of the reference's ant_train_one_epoch (trainer/train.py:31-54) on make_tree's tree, shuffle off, window phase
    seeded (np.random.seed(0) in front of the dataset), `.cuda()` an identity in this process"""
    from criterions.loss import OadAntLoss
    from datasets.dataset import THUMOSDataset
    from model import build_model
    from trainer.train import ant_train_one_epoch
    cfg = epoch_cfg(tempfile.mkdtemp())
    np.random.seed(0)
    ds = THUMOSDataset(cfg, "train")
    loader = torch.utils.data.DataLoader(ds, batch_size=cfg["batch_size"], shuffle=False)
    model = _load(build_model(cfg, "cpu"), W.miniroad_a_state_dict(cfg, 20))
    opt = torch.optim.AdamW([{"params": model.parameters(), "initial_lr": cfg["lr"]}], lr=cfg["lr"], weight_decay=cfg["weight_decay"])
    orig = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        loss = ant_train_one_epoch(loader, model, OadAntLoss(cfg), opt, None, 1)
    finally:
        torch.Tensor.cuda = orig
    save = {"epoch_loss": np.float64(loss), "n_windows": np.int64(len(ds))}
    for k, p in model.named_parameters():
        _put(save, "param." + k, p.detach().numpy())
    np.savez_compressed(os.path.join(OUT, "g13f_mroada_epoch.npz"), **save)
    print("g13f epoch loss", loss, "windows", len(ds))


if __name__ == "__main__":
    _stub_modules()
    grad_cases()
    adamw_case()
    epoch_case()
