#!/usr/bin/env python3
"""Generate tests/golden/g12_* (MiniROADA) by importing the reference model, with the import stubs of oracle/gen_golden.py.

Only data is written: inputs and weights are regenerated from seeds by prego_amd/weights.py, the fixtures hold the reference's
outputs (sampled frames where a whole output would exceed ~1 MB), state_dict key lists / shapes and sampled initial weights.

    python scripts/gen_golden_anticipation.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle.gen_golden import OUT, _load, _stub_modules     # noqa: E402
from prego_amd import weights as W                           # noqa: E402
from prego_amd.config import anticipation_cfg, assembly101_cfg  # noqa: E402

# (tag, hidden_dim, L, head_gain, ant_gain)
CASES = [("plain", 1024, 1, 1.0, 1.0), ("plain", 1024, 4, 1.0, 1.0), ("plain", 1024, 8, 1.0, 1.0), ("plain", 512, 8, 1.0, 1.0),
         ("peaky", 1024, 1, 8.0, 4.0), ("peaky", 1024, 4, 8.0, 4.0), ("peaky", 1024, 8, 8.0, 4.0), ("peaky", 512, 8, 8.0, 4.0)]


def _margin(p):
    s = np.sort(p, -1)
    return (s[..., -1] - s[..., -2]).astype(np.float32)


def _eval(model, rgb):
    with torch.no_grad():
        o = model(torch.from_numpy(rgb), torch.from_numpy(np.zeros_like(rgb)))
    return o["logits"][0].numpy(), o["anticipation_logits"][0].numpy()


def eval_cases():
    from model import build_model
    for tag, H, L, hg, ag in CASES:
        cfg = anticipation_cfg(assembly101_cfg(hidden_dim=H), L)
        sd = W.miniroad_a_state_dict(cfg, 20, head_gain=hg, ant_gain=ag)
        model = _load(build_model(cfg, "cpu"), sd).eval()
        rgb = W.tsn_features((1, 256, 2048), 20, "g12.rgb")
        p, a = _eval(model, rgb)
        idx = np.linspace(0, 255, 48).astype(np.int64)
        np.savez_compressed(os.path.join(OUT, f"g12_mroada_eval_{tag}_h{H}_L{L}.npz"),
                            probs=p.astype(np.float32), argmax=p.argmax(-1).astype(np.int32),
                            ant_argmax=a.argmax(-1).astype(np.int16), ant_margin=_margin(a),
                            sample_idx=idx, ant_sample=a[idx].astype(np.float32),
                            head_gain=np.float32(hg), ant_gain=np.float32(ag))
        print("g12", tag, H, L, "min ant margin", float(_margin(a).min()))
        if tag == "peaky" and H == 1024 and L == 8:
            T = 4096
            rgbL = W.tsn_features((1, T, 2048), 20, f"g12.rgb.{T}")
            p, a = _eval(model, rgbL)
            idx = np.linspace(0, T - 1, 64).astype(np.int64)
            np.savez_compressed(os.path.join(OUT, f"g12_mroada_longT_{T}.npz"),
                                argmax=p.argmax(-1).astype(np.int16), ant_argmax=a.argmax(-1).astype(np.int16),
                                ant_margin=_margin(a), sample_idx=idx, sample_probs=p[idx].astype(np.float32),
                                ant_sample=a[idx].astype(np.float32))
            print("g12 longT done")


# ---- tiny on-disk tree for the data layers and the evaluator (regenerated from seeds by the tests) -------------------------------
TREE_VIDS = {"train": ["vid_a", "vid_b"], "test": ["vid_c", "vid_d", "vid_e"]}
TREE_LENS = {"vid_a": 40, "vid_b": 27, "vid_c": 45, "vid_d": 30, "vid_e": 22}
TREE_C, TREE_L = 5, 3


def tree_cfg(root: str, **over) -> dict:
    """a TVSeries-shaped anticipation cfg over the tree make_tree writes at `root` (1024-d features, 5 classes, L = 3)"""
    cfg = anticipation_cfg(assembly101_cfg(
        data_name="TVSERIES_ANTICIPATION", task="ANTICIPATION", loss="ANTICIPATION", root_path=root,
        rgb_type="rgb_kinetics_bninception", flow_type="flow_kinetics_bninception", annotation_type="target_perframe",
        video_list_path=os.path.join(root, "video_list.json"), window_size=8, stride=4, num_classes=TREE_C,
        hidden_dim=512, embedding_dim=512), TREE_L)
    cfg.update(over)
    return cfg


def make_tree(root: str) -> dict:
    os.makedirs(root, exist_ok=True)
    for sub in ("target_perframe", "rgb_kinetics_bninception", "flow_kinetics_bninception"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for vid, T in TREE_LENS.items():
        lab = (W.uniform01((T,), 7, f"tree.lab.{vid}") * TREE_C).astype(np.int64)
        np.save(os.path.join(root, "target_perframe", vid + ".npy"), np.eye(TREE_C, dtype=np.float32)[lab])
        np.save(os.path.join(root, "rgb_kinetics_bninception", vid + ".npy"), W.tsn_features((T, 1024), 7, f"tree.rgb.{vid}"))
        np.save(os.path.join(root, "flow_kinetics_bninception", vid + ".npy"), W.tsn_features((T, 1024), 7, f"tree.flow.{vid}"))
    with open(os.path.join(root, "video_list.json"), "w") as f:
        json.dump({"TVSERIES": {"train_session_set": TREE_VIDS["train"], "test_session_set": TREE_VIDS["test"],
                                "class_index": ["background"] + [f"step{i}" for i in range(1, TREE_C)]}}, f)
    return tree_cfg(root)


class StandIn(torch.nn.Module):
    """a fixed stand-in model for the evaluator: probabilities from the first feature channels (no weights)"""

    def __init__(self, C=TREE_C, L=TREE_L):
        super().__init__()
        self.C, self.L = C, L

    def forward(self, rgb, flow):
        B, T, _ = rgb.shape
        logits = 4.0 * rgb[..., :self.C] - 2.0 * flow[..., :self.C]
        ant = (4.0 * rgb[..., self.C:self.C * (self.L + 1)] - flow[..., :self.C * self.L]).reshape(B, T, self.L, self.C)
        return {"logits": torch.softmax(logits, -1), "anticipation_logits": torch.softmax(ant, -1)}


class _Log:
    def info(self, *a, **k):
        pass


def tree_cases():
    """feeder windows, ANT_Evaluate on the stand-in (AP, cAP) and on MROADA (AP), OadAntLoss value and gradient"""
    import tempfile
    from criterions.loss import OadAntLoss
    from datasets.dataset import THUMOSDataset
    from model import build_model
    from trainer.eval import ANT_Evaluate
    root = tempfile.mkdtemp()
    cfg = make_tree(root)
    np.random.seed(0)
    tr = THUMOSDataset(cfg, "train")
    te = THUMOSDataset(cfg, "test")
    feed = {"train_vid": np.array([TREE_VIDS["train"].index(x[0]) for x in tr.inputs], np.int32),
            "train_start": np.array([x[1] for x in tr.inputs], np.int32), "train_end": np.array([x[2] for x in tr.inputs], np.int32),
            "train_ant": np.stack([x[4] for x in tr.inputs]).astype(np.float32),
            "train_rgb_sum": np.array([float(tr[i][0].double().sum()) for i in range(len(tr))]),
            "test_end": np.array([x[2] for x in te.inputs], np.int32)}
    for i, x in enumerate(te.inputs):
        feed[f"test_ant_{i}"] = np.asarray(x[4], np.float32)
        feed[f"test_target_{i}"] = np.asarray(x[3], np.float32)
    np.savez_compressed(os.path.join(OUT, "g12_feeder_windows.npz"), **feed)
    # the reference evaluator pins "cuda:0"; on a CPU box its .to("cuda:0") is made a no-op
    orig_to = torch.Tensor.to
    torch.Tensor.to = lambda self, *a, **k: self if (a and a[0] == "cuda:0") else orig_to(self, *a, **k)
    try:
        res = {}
        loader = torch.utils.data.DataLoader(te, batch_size=1, shuffle=False)
        for metric in ("AP", "cAP"):
            ev = ANT_Evaluate(dict(cfg, metric=metric))
            mean = ev.eval(StandIn().eval(), loader, _Log())
            res[f"standin_{metric}"] = {"mean": float(mean), "steps": _steps(ev, StandIn().eval(), loader, metric, cfg)}
        sd = W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0)
        model = _load(build_model(cfg, "cpu"), sd).eval()
        ev = ANT_Evaluate(dict(cfg, metric="AP"))
        res["mroada_AP"] = {"mean": float(ev.eval(model, loader, _Log())), "steps": _steps(ev, model, loader, "AP", cfg)}
    finally:
        torch.Tensor.to = orig_to
    with open(os.path.join(OUT, "g12_ant_eval.json"), "w") as f:
        json.dump(res, f)
    # OadAntLoss (reduction 'sum') on fixed logits / multi-label targets, some rows all zero
    logits = torch.from_numpy(W.normal((3, 4, TREE_L, TREE_C), 7, "loss.logits")).requires_grad_(True)
    target = torch.from_numpy((W.uniform01((3, 4, TREE_C), 7, "loss.t") > 0.6).astype(np.float32))
    ant_t = torch.from_numpy((W.uniform01((3, TREE_L, TREE_C), 7, "loss.at") > 0.6).astype(np.float32))
    loss = OadAntLoss(cfg)({"anticipation_logits": logits}, target, ant_t)
    loss.backward()
    np.savez_compressed(os.path.join(OUT, "g12_ant_loss.npz"), loss=np.float32(loss.item()), grad=logits.grad.numpy().astype(np.float32))
    print("g12 tree cases:", json.dumps({k: v["mean"] for k, v in res.items()}), "loss", float(loss))


def _steps(ev, model, loader, metric, cfg):
    """per-step mAPs the reference's ANT_Evaluate logged (its return value is only their mean): recomputed with its own metric"""
    from utils.metrics import perframe_average_precision
    ps, ts = [], []
    with torch.no_grad():
        for rgb, flow, t, at in loader:
            ps.append(model(rgb, flow)["anticipation_logits"][0].numpy()); ts.append(at[0].numpy())
    p, t = np.concatenate(ps), np.concatenate(ts)
    return [float(perframe_average_precision(p[:, l], t[:, l], ev.all_class_names, None, metric)["mean_AP"]) for l in range(t.shape[1])]


def init_weights():
    """state_dict keys / shapes and sampled initial weights under torch.manual_seed(0), actionness on and off (hidden_dim 512, L 4)."""
    from model import build_model
    res = {}
    for act in (False, True):
        cfg = anticipation_cfg(assembly101_cfg(hidden_dim=512), 4, actionness=act)
        torch.manual_seed(0)
        m = build_model(cfg, "cpu")
        sd = m.state_dict()
        res[str(act)] = {"keys": list(sd.keys()), "shapes": [list(v.shape) for v in sd.values()],
                         "head": {k: v.flatten()[:8].tolist() for k, v in sd.items()},
                         "sum": {k: float(v.double().sum()) for k, v in sd.items()}}
    with open(os.path.join(OUT, "g12_mroada_init.json"), "w") as f:
        json.dump(res, f)
    print("g12 init done")


if __name__ == "__main__":
    _stub_modules()
    eval_cases()
    init_weights()
    tree_cases()
