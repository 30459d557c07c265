"""A tiny THUMOS-shaped tree for the evaluators' THUMOS post-processing tests: 22 classes, class 21 = "ambiguous" (one-hot rows
there are the frames the post-processing removes), regenerated from seeds."""
import json
import os

import numpy as np

from prego_amd import weights as W
from prego_amd.config import anticipation_cfg, assembly101_cfg

C, AMB, L = 22, 21, 2
VIDS = {"train": ["th_a"], "test": ["th_b", "th_c", "th_d"]}
LENS = {"th_a": 30, "th_b": 47, "th_c": 32, "th_d": 24}
NAMES = ["background"] + [f"action{i}" for i in range(1, AMB)] + ["ambiguous"]


def targets(T, tag):
    """one-hot rows [T, 22]: runs of 1-5 frames of the classes 0 .. 20; every seventh run is ambiguous; the first video frame too"""
    u = W.uniform01((2 * T,), 11, f"thumos.tree.{tag}")
    ids, k = [], 0
    while len(ids) < T:
        m = 1 + int(u[2 * k] * 5)
        c = AMB if k % 7 == 3 else int(u[2 * k + 1] * AMB)
        ids += [c] * m
        k += 1
    ids = np.array(ids[:T], np.int64)
    ids[0] = AMB
    return np.eye(C, dtype=np.float32)[ids]


def make_thumos_tree(root: str, **over) -> dict:
    """writes the tree and returns a THUMOS_ANTICIPATION cfg over it (1024-d features, hidden_dim 512, L = 2)"""
    os.makedirs(root, exist_ok=True)
    for sub in ("target_perframe", "rgb_kinetics_bninception", "flow_kinetics_bninception"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for vid, T in LENS.items():
        np.save(os.path.join(root, "target_perframe", vid + ".npy"), targets(T, vid))
        np.save(os.path.join(root, "rgb_kinetics_bninception", vid + ".npy"), W.tsn_features((T, 1024), 11, f"thumos.rgb.{vid}"))
        np.save(os.path.join(root, "flow_kinetics_bninception", vid + ".npy"), W.tsn_features((T, 1024), 11, f"thumos.flow.{vid}"))
    with open(os.path.join(root, "video_list.json"), "w") as f:
        json.dump({"THUMOS": {"train_session_set": VIDS["train"], "test_session_set": VIDS["test"], "class_index": NAMES}}, f)
    cfg = anticipation_cfg(assembly101_cfg(
        data_name="THUMOS_ANTICIPATION", task="ANTICIPATION", loss="ANTICIPATION", root_path=root,
        rgb_type="rgb_kinetics_bninception", flow_type="flow_kinetics_bninception", annotation_type="target_perframe",
        video_list_path=os.path.join(root, "video_list.json"), window_size=8, stride=4, num_classes=C,
        hidden_dim=512, embedding_dim=512), L)
    cfg.update(over)
    return cfg
