"""Feature trees on disk for the train-cache tests (tests/test_train_cache_cpu.py, tests/test_gpu_train_cache.py): four videos of 300,
157, 5 and 1 frames - longer than a window, shorter than one, a single frame - with 12 classes, written from seeds."""
import json
import os

import numpy as np

from prego_amd import weights as W
from prego_amd.config import anticipation_cfg, assembly101_cfg, epic_tent_cfg

LENS = {"v300": 300, "v157": 157, "v5": 5, "v1": 1}
N_CLASSES = 12


def targets(T, kind, k):
    """'onehot': one class per frame, every 17th row all-zero (4 bytes per frame suffice); 'multi': also rows with two classes and a
    row whose single entry is 0.5 (only dense rows reproduce them)"""
    t = np.zeros((T, N_CLASSES), np.float32)
    rows = np.arange(T)
    t[rows, (rows // 29 + k) % N_CLASSES] = 1.0
    t[rows % 17 == 3] = 0.0
    if kind == "multi":
        two = rows[rows % 11 == 5]
        t[two, (two + 3) % N_CLASSES] = 1.0
        if T > 2:
            t[2] = 0.0
            t[2, 7] = 0.5
    return t


def _save(path, arr):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.save(path, arr)


def oad_tree(root, d_rgb=2048, flow="zero", kind="onehot", **over):
    """an EPIC-TENT-O tree; flow 'zero': the shipped config (flow_anet_resnet50, overwritten with zeros), 'disk': 1024-d flow files"""
    flow_type = "flow_anet_resnet50" if flow == "zero" else "flow_kinetics_bninception"
    for k, (vid, T) in enumerate(LENS.items()):
        _save(os.path.join(root, "rgb_anet_resnet50", vid + ".npy"), W.tsn_features((T, d_rgb), 31, f"tc.rgb.{vid}"))
        _save(os.path.join(root, "target_perframe", vid + ".npy"), targets(T, kind, k))
        if flow == "disk":
            _save(os.path.join(root, flow_type, "assembly_optical_flow_BNInception", vid, "assembling.npy"),
                  W.tsn_features((T, 1024), 31, f"tc.flow.{vid}"))
    vl = os.path.join(root, "video_list.json")
    json.dump({"EPIC-TENT-O": {"train_session_set": list(LENS), "test_session_set": ["v157", "v5"],
                               "class_index": [f"c{i}" for i in range(N_CLASSES)]}}, open(vl, "w"))
    cfg = epic_tent_cfg(root_path=root, video_list_path=vl, flow_type=flow_type, num_workers=0, batch_size=16)
    cfg.update(over)
    return cfg


def ant_tree(root, d=1024, L=3, kind="onehot", **over):
    """a TVSeries-shaped anticipation tree (rgb and flow of `d` values)"""
    for k, (vid, T) in enumerate(LENS.items()):
        _save(os.path.join(root, "rgb_kinetics_bninception", vid + ".npy"), W.tsn_features((T, d), 32, f"tc.rgb.{vid}"))
        _save(os.path.join(root, "flow_kinetics_bninception", vid + ".npy"), W.tsn_features((T, d), 32, f"tc.flow.{vid}"))
        _save(os.path.join(root, "target_perframe", vid + ".npy"), targets(T, kind, k))
    vl = os.path.join(root, "video_list.json")
    json.dump({"TVSERIES": {"train_session_set": list(LENS), "test_session_set": ["v157", "v300"],
                            "class_index": ["background"] + [f"step{i}" for i in range(1, N_CLASSES)]}}, open(vl, "w"))
    cfg = anticipation_cfg(assembly101_cfg(
        data_name="TVSERIES_ANTICIPATION", task="ANTICIPATION", loss="ANTICIPATION", root_path=root, rgb_type="rgb_kinetics_bninception",
        flow_type="flow_kinetics_bninception", annotation_type="target_perframe", video_list_path=vl, window_size=8, stride=4,
        num_classes=N_CLASSES, num_workers=0, batch_size=16), L)
    cfg.update(over)
    return cfg


def same_batch(got, want):
    """a train-cache batch against the loader's: tensors bit for bit, vids / starts / ends equal"""
    import torch
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        if isinstance(b, torch.Tensor):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b), k
        else:
            assert list(a) == list(b), k
