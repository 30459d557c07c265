"""GPU: the training set in device memory (cfg['train_cache_device'], prego_amd/train_cache.py) and its kernel (prego_gather_windows,
csrc/train_cache.hip).  Everything here is exact: a cached batch is the loader's batch bit for bit, so a cached epoch is the loader-fed
epoch bit for bit - same epoch loss, same weights - and a cached main.py run saves the loader-fed run's checkpoint."""
import ctypes as C
import glob
import logging

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from torch.utils.data import DataLoader                   # noqa: E402

from prego_amd import train_cache as TC                   # noqa: E402
from prego_amd import weights as W                        # noqa: E402
from prego_amd.data import build_data_loader              # noqa: E402
from tests.helpers import train_cache_tree as T           # noqa: E402

DEV = "cuda:0"
LOG = logging.getLogger("tc.gpu")


# ---- 1. batches --------------------------------------------------------------------------------------------------------------------
# d_rgb 2052: 513 vectors of 16 bytes, a third, partial trip of the 256 lanes over a row; 12: fewer vectors than lanes.  window 128 and 8
# against videos of 300, 157, 5 and 1 frames; 12 classes: a target row is three vectors, a 16-window batch of window 8 is 1536 target
# elements (two chunks of 1024, the second partial).
_CONFIGS = {
    "zero-flow": lambda r: T.oad_tree(r, d_rgb=2048, flow="zero", kind="onehot", window_size=128),
    "disk-flow": lambda r: T.oad_tree(r, d_rgb=2052, flow="disk", kind="onehot", window_size=8),
    "dense-targets": lambda r: T.oad_tree(r, d_rgb=12, flow="disk", kind="multi", window_size=128),
    "anticipation": lambda r: T.ant_tree(r, d=1024, L=3, kind="onehot", window_size=8),
    "anticipation-dense": lambda r: T.ant_tree(r, d=12, L=3, kind="multi", window_size=128),
    "pad-entries": lambda r: T.oad_tree(r, d_rgb=2048, flow="zero", kind="onehot", window_size=8),
    "pad-entries-anticipation": lambda r: T.ant_tree(r, d=1024, L=3, kind="onehot", window_size=8),
}


@pytest.mark.parametrize("name", sorted(_CONFIGS))
def test_every_batch_of_an_epoch_is_the_loaders(tmp_path, name):
    cfg = _CONFIGS[name](str(tmp_path))
    np.random.seed(11)
    loader = build_data_loader(cfg, "train")
    ds = loader.dataset
    if name.startswith("pad-entries"):                  # a sampler that names PAD entries (index + len), as EpochWindowSampler does
        n = len(ds)
        ds._init_features = lambda: None
        loader = DataLoader(ds, batch_size=16, sampler=torch.randperm(n, generator=torch.Generator().manual_seed(1)).tolist() + [n + 2, n, 2 * n - 1])
    dl = TC.device_loader(loader, DEV, cfg, LOG)
    assert isinstance(dl, TC.DeviceWindowLoader) and dl.dataset is ds and len(dl) == len(loader)
    info = dl.cache_info()
    assert info["state"] == "filled" and info["frames"] == 463 and info["videos"] == 4
    assert info["targets"] == ("dense" if "dense" in name else "labels")
    for epoch in range(2):
        torch.manual_seed(epoch)
        want = list(loader)
        torch.manual_seed(epoch)
        got = list(dl)
        assert len(got) == len(want) > 4
        for g, w in zip(got, want):
            assert all(t.is_cuda for t in g[:len(g) if "anticipation" in name else 3])
            T.same_batch(g, w)
        ds._init_features()
    if name == "zero-flow":
        assert got[0][1].data_ptr() == got[1][1].data_ptr() and got[-1][1].shape[0] == got[-1][0].shape[0] < 16      # one zero tensor, its first rows
        assert got[0][0].data_ptr() != got[1][0].data_ptr()                                                          # fresh tensors otherwise
    dl.drop_cache()
    assert dl.cache_info()["state"] == "empty" and dl.cache_info()["bytes"] == 0
    torch.manual_seed(5)
    want = list(loader)
    torch.manual_seed(5)
    for g, w in zip(dl, want):                         # the next epoch uploads the set again
        T.same_batch(g, w)
    assert dl.cache_info()["state"] == "filled"


# ---- 2. the C entry ----------------------------------------------------------------------------------------------------------------
def _entry_args():
    """a tiny valid call: 2 videos of 5 and 3 frames, d 8, 3 classes, W 2, L 1, three windows, a batch of two"""
    g = torch.Generator().manual_seed(2)
    t = dict(rgb=torch.randn(8, 8, generator=g), flow=torch.randn(8, 8, generator=g), labels=torch.tensor([0, 1, 2, -1, 1, 2, 0, 1], dtype=torch.int32),
             row0=torch.tensor([0, 5]), vlen=torch.tensor([5, 3], dtype=torch.int32), table=torch.tensor([[0, 0], [1, 1], [0, 3]], dtype=torch.int32),
             order=torch.tensor([2, 0, 1], dtype=torch.int32))
    t = {k: v.to(DEV) for k, v in t.items()}
    t["dense"] = torch.nn.functional.one_hot(t["labels"].clamp(min=0).long(), 3).float() * (t["labels"] >= 0)[:, None]
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)      # noqa: E731
    t.update(rgb_out=nan(2, 2, 8), flow_out=nan(2, 2, 8), target_out=nan(2, 2, 3), ant_out=nan(2, 1, 3))
    return t


def _call(lib, t, **over):
    p = {k: (None if v is None else v.data_ptr()) for k, v in t.items()}
    k = dict(p, n_rows=8, d_rgb=8, d_flow=8, dense=None, n_videos=2, n_windows=3, n_order=3, first=1, n=2, W=2, C=3, L=1)
    k.update(over)
    return lib.prego_gather_windows(k["rgb"], k["flow"], k["n_rows"], k["d_rgb"], k["d_flow"], k["labels"], k["dense"], k["row0"], k["vlen"],
                                    k["n_videos"], k["table"], k["n_windows"], k["order"], k["n_order"], k["first"], k["n"], k["W"], k["C"], k["L"],
                                    k["rgb_out"], k["flow_out"], k["target_out"], k["ant_out"], torch.cuda.current_stream().cuda_stream)


def test_refusals_launch_nothing_and_a_call_neither_allocates_nor_waits():
    from prego_amd import _lib
    dbg = _lib.load_debug()
    t = _entry_args()
    outs = [t[k] for k in ("rgb_out", "flow_out", "target_out", "ant_out")]
    a = t["rgb"].data_ptr()
    cases = {"d_rgb % 4": dict(d_rgb=6), "d_flow % 4": dict(d_flow=2), "misaligned rows": dict(rgb=a + 4), "misaligned out": dict(target_out=t["target_out"].data_ptr() + 4),
             "n < 1": dict(n=0), "both targets": dict(dense=t["dense"].data_ptr()), "no targets": dict(labels=None), "W < 1": dict(W=0),
             "L < 0": dict(L=-1), "ant out without L": dict(L=0)}
    for what, over in cases.items():
        assert _call(dbg, t, **over) == -1, what
        assert b"gather_windows" in dbg.prego_last_error(), what
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)

    def counts():
        m, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(m), C.byref(w)) == 0
        return m.value, w.value
    n0 = counts()
    assert _call(dbg, t) == 0, dbg.prego_last_error()
    assert counts() == n0                                       # no device allocation and no host wait inside the call
    torch.cuda.synchronize()
    # order[1:3] = windows 0 and 1: (video 0, start 0) = pad row + frame 0, ant = frame 1; (video 1, start 1) = frames 0, 1 of video 1,
    # ant = its frame 2
    rgb, lab = t["rgb"], [0, 1, 2, -1, 1, 2, 0, 1]
    hot = lambda i: [float(lab[i] == c) for c in range(3)]      # noqa: E731
    assert torch.equal(t["rgb_out"], torch.stack([torch.stack([torch.zeros(8, device=DEV), rgb[0]]), rgb[5:7]]))
    assert torch.equal(t["flow_out"], torch.stack([torch.stack([torch.zeros(8, device=DEV), t["flow"][0]]), t["flow"][5:7]]))
    assert t["target_out"].tolist() == [[[0.0] * 3, hot(0)], [hot(5), hot(6)]]
    assert t["ant_out"].tolist() == [[hot(1)], [hot(7)]]
    # dense rows instead of class ids: the same targets; nullable outputs are left alone
    t2 = _entry_args()
    assert _call(dbg, t2, labels=None, dense=t2["dense"].data_ptr(), rgb_out=None, flow_out=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(t2["target_out"], t["target_out"]) and torch.equal(t2["ant_out"], t["ant_out"]) and bool(torch.isnan(t2["rgb_out"]).all())
    # tables that point outside give zeros, never a read: a window index, a video index, a start and a row0 out of range
    t3 = _entry_args()
    t3["order"] = torch.tensor([7, -1, 1, 0], dtype=torch.int32, device=DEV)
    t3["table"] = torch.tensor([[5, 0], [1, 2 ** 31 - 1], [0, 3]], dtype=torch.int32, device=DEV)
    assert _call(dbg, t3, n_order=4, first=0, n=2) == 0
    torch.cuda.synchronize()
    assert not t3["rgb_out"].any() and not t3["target_out"].any()
    assert _call(dbg, t3, n_order=4, first=2, n=2) == 0
    t4 = _entry_args()
    t4["row0"] = torch.tensor([10 ** 12, 6], device=DEV)         # video 1 now claims rows 6, 7 and 8 of 8
    t5 = _entry_args()
    t5["row0"] = torch.tensor([-1, -4], device=DEV)
    assert _call(dbg, t4) == 0 and _call(dbg, t5) == 0
    torch.cuda.synchronize()
    for o in (t3["rgb_out"], t3["target_out"], t3["ant_out"], t4["rgb_out"][0], t4["target_out"][0], t4["ant_out"], t5["rgb_out"][1], t5["ant_out"][1]):
        assert not o.any()
    assert torch.equal(t4["rgb_out"][1], rgb[6:8]) and t4["target_out"][1].tolist() == [hot(6), hot(7)]
    assert torch.equal(t5["rgb_out"][0], torch.zeros(2, 8, device=DEV)) and t5["ant_out"][0].tolist() == [hot(0)]      # rows -1 (refused) and 0


# ---- 3. a cached epoch is the loader-fed epoch --------------------------------------------------------------------------------------
def _epoch_pair(cfg, build, trainer_key, call):
    """one epoch loader-fed and one cached, from the same state_dict and seeds: (epoch loss, weights) of both"""
    import prego_amd.loss, prego_amd.model, prego_amd.trainer, prego_amd.transformer  # noqa: F401
    from prego_amd.optim import FusedAdamW
    from prego_amd.registry import TRAINER, build_criterion
    res = {}
    for leg in ("loader", "cached"):
        np.random.seed(3)
        torch.manual_seed(3)
        loader = build_data_loader(cfg, "train")
        if leg == "cached":
            loader = TC.device_loader(loader, DEV, cfg, LOG)
            assert isinstance(loader, TC.DeviceWindowLoader)
        model = build()
        crit = build_criterion(cfg, DEV)
        opt = FusedAdamW([{"params": list(model.parameters()), "initial_lr": 1e-3}], lr=1e-3, weight_decay=0.05, model=model)
        loss = call(TRAINER[trainer_key], loader, model, crit, opt)
        assert len(loader) > 4
        res[leg] = (loss, {k: p.detach().clone() for k, p in model.named_parameters()})
    assert np.isfinite(res["loader"][0]) and res["loader"][0] == res["cached"][0], (res["loader"][0], res["cached"][0])
    for k, p in res["loader"][1].items():
        assert torch.equal(p, res["cached"][1][k]), k
    return res


def _load(cfg, sd):
    from prego_amd.registry import build_model
    m = build_model(cfg, DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.train()


def test_a_cached_oad_epoch_equals_the_loader_fed_epoch(tmp_path):
    """MiniROAD, bf16, dropout 0.2, FusedAdamW, the guarded loop"""
    import prego_amd.trainer as TR
    cfg = T.oad_tree(str(tmp_path), window_size=128, dropout=0.2, compute_dtype="bf16", assume_zero_flow=True)
    sd = W.miniroad_state_dict(cfg, 20)
    assert TR.GUARDED_LOOP
    res = _epoch_pair(cfg, lambda: _load(cfg, sd), "OAD", lambda tr, loader, m, crit, opt: tr(loader, m, crit, opt, None, 1, DEV, None, scheduler=None))
    assert any(not np.array_equal(res["loader"][1][k].cpu().numpy(), sd[k]) for k in sd)          # the epoch did train


def test_a_cached_anticipation_epoch_equals_the_loader_fed_epoch(tmp_path):
    cfg = T.ant_tree(str(tmp_path), d=1024, L=2, window_size=8, hidden_dim=512, embedding_dim=512, dropout=0.2, compute_dtype="bf16")
    sd = W.miniroad_a_state_dict(cfg, 20)
    _epoch_pair(cfg, lambda: _load(cfg, sd), "ANTICIPATION", lambda tr, loader, m, crit, opt: tr(loader, m, crit, opt, None, 1, device=DEV))


def test_a_cached_transformer_epoch_equals_the_loader_fed_epoch(tmp_path):
    """the `Transformer` entry, one layer, window 32, with its dropout on"""
    cfg = T.oad_tree(str(tmp_path), model="Transformer", window_size=32, patch_dim=1, num_heads=8, attn_dropout_rate=0.1, dropout=0.1,
                     num_layers=1, compute_dtype="bf16")
    sd = W.vit_state_dict(cfg, 20)
    _epoch_pair(cfg, lambda: _load(cfg, sd), "OAD", lambda tr, loader, m, crit, opt: tr(loader, m, crit, opt, None, 1, DEV, None, scheduler=None))


# ---- 4. main.py --------------------------------------------------------------------------------------------------------------------
def test_main_with_the_switch_saves_the_loader_fed_checkpoint(tmp_path, monkeypatch):
    from prego_amd import main as M
    base = T.oad_tree(str(tmp_path / "data"), num_epoch=2)
    for k in ("eval", "amp", "tensorboard", "lr_scheduler", "no_rgb", "no_flow", "config"):
        base.pop(k, None)                              # argparse supplies these (main.py:16-24)
    monkeypatch.chdir(tmp_path)
    runs = {}
    for name, extra in {"loader": {}, "cached": {"train_cache_device": True},
                        "fallback": {"train_cache_device": True, "train_cache_max_bytes": 1}}.items():
        cfg = dict(base, output_path=str(tmp_path / name), **extra)
        ypath = tmp_path / f"{name}.yaml"
        yaml.safe_dump(cfg, open(ypath, "w"))
        best = M.main(["--config", str(ypath)])
        ck = glob.glob(str(tmp_path / name / "*" / "ckpts" / "best_*.pth"))
        assert len(ck) == 1, (name, ck)
        runs[name] = (best, torch.load(ck[0], map_location="cpu"))
        if name == "cached":
            info = TC.cache_info()
            assert info["state"] == "filled" and info["frames"] == 463 and info["bytes"] == 463 * 2048 * 4 + 463 * 4 + 12 * 4
        if name == "fallback":
            assert TC.cache_info()["state"] == "disabled" and "budget" in TC.cache_info()["reason"]
    for name in ("cached", "fallback"):
        assert runs[name][0] == runs["loader"][0] and 0.0 < runs[name][0] <= 1.0, (name, runs[name][0], runs["loader"][0])
        assert set(runs[name][1]) == set(runs["loader"][1])
        for k, v in runs["loader"][1].items():
            assert torch.equal(v, runs[name][1][k]), (name, k)
