"""GPU tests of MiniROADA training against the reference itself (tests/golden/g13*, scripts/gen_golden_anticipation_train.py): losses,
outputs and gradients (g13a-d), three AdamW steps (g13e), one epoch of the reference's ant_train_one_epoch (g13f); and the contracts
around the step: the AdamW launches are no-ops while the timeout word is set, the anticipation gradients travel in sub-bucket 0 of the
data-parallel bucket, and main.main trains, checkpoints and re-evaluates a MiniROADA model."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prego_amd import weights as W                                   # noqa: E402
from scripts.gen_golden_anticipation_train import (CASES, case_batch, case_cfg, dense_weights,   # noqa: E402
                                                   epoch_cfg)

G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
LOSS_TOL = {"fp32": 1e-4, "bf16": 2e-2}          # G4b's tiers: loss relative, samples relative to the tensor's norm
GRAD_TOL = {"fp32": 2e-3, "bf16": 6e-2}


def _model(cfg, dtype):
    import prego_amd.model  # noqa: F401
    from prego_amd.registry import build_model
    m = build_model(dict(cfg, compute_dtype=dtype), DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_a_state_dict(cfg, 20).items()})
    return m.train()


def _close(ref, name, got, tol):
    norm, idx, val = float(ref["norm." + name]), ref["idx." + name], ref["val." + name]
    g = got.detach().reshape(-1).double().cpu().numpy()
    err = float(np.abs(g[idx] - val).max())
    assert err <= tol * norm, f"{name}: max |d| {err:.3e} > {tol} x norm {norm:.3e}"
    assert abs(np.linalg.norm(g) - norm) <= tol * norm, f"{name}: norm {np.linalg.norm(g):.6e} vs {norm:.6e}"


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tag", sorted(CASES))
def test_gradients_match_the_reference(tag, dtype):
    from prego_amd.loss import OadAntLoss
    ref = np.load(os.path.join(G, f"{tag}_mroada_train.npz"))
    cfg = case_cfg(tag)
    m = _model(cfg, dtype)
    rgb, flow, tgt, ant = (torch.from_numpy(x).to(DEV) for x in case_batch(tag))
    out = m(rgb, flow)
    if CASES[tag][6] == "ant":
        loss = OadAntLoss(cfg)(out, tgt, ant)
    else:
        wl, wa = (torch.from_numpy(x).to(DEV) for x in dense_weights(tag))
        loss = (out["logits"] * wl).sum() + (out["anticipation_logits"] * wa).sum()
    loss.backward()
    lr = float(ref["loss"])
    assert abs(float(loss.detach()) - lr) <= LOSS_TOL[dtype] * max(1.0, abs(lr)), (float(loss.detach()), lr)
    tol = GRAD_TOL[dtype]
    _close(ref, "out.logits", out["logits"], tol)
    _close(ref, "out.anticipation_logits", out["anticipation_logits"], tol)
    if "last_ant" in ref:
        last = out["anticipation_logits"][:, -1].detach().cpu().numpy()
        assert np.abs(last - ref["last_ant"]).max() <= tol * np.linalg.norm(ref["last_ant"])
    no_grad = set(ref["no_grad"].tolist())
    for k, p in m.named_parameters():
        if k in no_grad:
            assert p.grad is None, k
        else:
            _close(ref, "grad." + k, p.grad, tol)
    if tag == "g13a":
        assert no_grad == {"f_actionness.0.weight", "f_actionness.0.bias"}


def _deltas_agree(ref, model, init, lr, what):
    """parameter moves against the reference's: an Adam step moves an element by about lr whatever its gradient's size, so elements whose
    gradient is ~0 may legitimately move the other way; at most 2 % of the sampled elements may differ by more than 5 % of lr"""
    bad = tot = 0
    for k, p in model.named_parameters():
        idx, val = ref["idx.param." + k], ref["val.param." + k]
        d_got = p.detach().reshape(-1).double().cpu().numpy()[idx] - init[k].reshape(-1)[idx]
        d_ref = val.astype(np.float64) - init[k].reshape(-1)[idx]
        bad += int(np.sum(np.abs(d_got - d_ref) > 0.05 * lr))
        tot += idx.size
    assert bad <= 0.02 * tot, f"{what}: {bad} of {tot} sampled elements moved differently from the reference"


def test_three_fused_adamw_steps_match_the_reference():
    from prego_amd.loss import OadAntLoss
    from prego_amd.optim import FusedAdamW
    ref = np.load(os.path.join(G, "g13e_mroada_adamw.npz"))
    cfg = case_cfg("g13a")
    init = W.miniroad_a_state_dict(cfg, 20)
    m = _model(cfg, "fp32")
    opt = FusedAdamW([{"params": list(m.parameters()), "initial_lr": 1e-4}], lr=1e-4, weight_decay=0.05, model=m)
    assert opt.is_guarded_for(m)
    rgb, flow, tgt, ant = (torch.from_numpy(x).to(DEV) for x in case_batch("g13a"))
    losses = []
    for _ in range(3):
        loss = OadAntLoss(cfg)(m(rgb, flow), tgt, ant)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    np.testing.assert_allclose(losses, ref["losses"], rtol=1e-4)
    _deltas_agree(ref, m, init, 1e-4, "g13e")
    assert torch.equal(m.f_actionness[0].weight.detach().cpu(), torch.from_numpy(init["f_actionness.0.weight"]))


def test_one_epoch_matches_the_reference_trainer(tmp_path):
    import prego_amd.data  # noqa: F401
    import prego_amd.trainer  # noqa: F401
    from prego_amd.loss import OadAntLoss
    from prego_amd.optim import FusedAdamW
    from prego_amd.registry import DATA_LAYERS, TRAINER
    ref = np.load(os.path.join(G, "g13f_mroada_epoch.npz"))
    cfg = epoch_cfg(str(tmp_path))
    np.random.seed(0)
    ds = DATA_LAYERS[cfg["data_name"]](cfg, "train")
    assert len(ds) == int(ref["n_windows"])
    loader = torch.utils.data.DataLoader(ds, batch_size=cfg["batch_size"], shuffle=False, pin_memory=True)
    init = W.miniroad_a_state_dict(cfg, 20)
    m = _model(cfg, "fp32")
    opt = FusedAdamW([{"params": list(m.parameters()), "initial_lr": cfg["lr"]}], lr=cfg["lr"], weight_decay=cfg["weight_decay"], model=m)
    loss = TRAINER["ANTICIPATION"](loader, m, OadAntLoss(cfg), opt, None, 1)
    assert abs(loss - float(ref["epoch_loss"])) <= 1e-4 * abs(float(ref["epoch_loss"])), (loss, float(ref["epoch_loss"]))
    _deltas_agree(ref, m, init, cfg["lr"], "g13f")


def test_anticipation_adamw_step_is_a_no_op_while_the_timeout_word_is_set():
    from prego_amd import _lib
    from prego_amd._lib import PregoError, ptr_array
    from prego_amd.engine import ANT_KEYS, MiniRoadEngine
    dbg = _lib.load_debug()
    cfg = case_cfg("g13c")
    sd = {k: torch.from_numpy(v).to(DEV) for k, v in W.miniroad_a_state_dict(cfg, 20).items()}
    eng = MiniRoadEngine(2048, 2048, 2048, 512, 86, DEV, "bf16", lib=dbg)
    eng.set_weights(sd)
    eng.set_anticipation(sd[ANT_KEYS[0]], sd[ANT_KEYS[1]], 1)
    params = [sd[k].clone() for k in ANT_KEYS]
    g = torch.Generator(device=DEV).manual_seed(3)
    grads = [torch.randn(p.shape, device=DEV, generator=g) * 1e-2 for p in params]
    m1, m2 = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def step():
        rc = dbg.prego_miniroad_adamw_step_anticipation(eng.h, ptr_array([p.data_ptr() for p in params]), ptr_array([x.data_ptr() for x in grads]),
                                                        ptr_array([x.data_ptr() for x in m1]), ptr_array([x.data_ptr() for x in m2]),
                                                        1, 1e-3, 0.9, 0.999, 1e-8, 0.05, s)
        assert rc == 0, dbg.prego_last_error()
    rgb = [torch.from_numpy(W.tsn_features((40, 2048), 20, "abort.rgb")).to(DEV)]
    fwd = lambda: eng.forward_ragged(rgb, None, softmax=False, want_ant=True)[3][0].clone()
    before = [p.clone() for p in params]
    out0 = fwd()
    assert dbg.prego_debug_set_abort(eng.h, 1, s) == 0
    step()
    torch.cuda.synchronize()
    assert all(torch.equal(p, b) for p, b in zip(params, before))
    assert not any(x.any() for x in m1 + m2)
    with pytest.raises(PregoError):
        eng.check()                                   # reports the timeout and clears the word
    eng.check()
    assert torch.equal(fwd(), out0)                   # the W_a operand copy was not touched either
    step()
    torch.cuda.synchronize()
    assert not any(torch.equal(p, b) for p, b in zip(params, before))
    assert not torch.equal(fwd(), out0)               # ... and follows the update now
    eng.check()


def test_anticipation_gradients_travel_in_sub_bucket_0(monkeypatch):
    """the data-parallel bucket path on one GPU with a stand-in collective (a world of 2 whose all_reduce doubles the tensor): the
    anticipation tensors sit in sub-bucket 0 with f_classification, the guard slot stays at the end of the last sub-bucket, and the
    reduced step equals the plain one"""
    import torch.distributed as dist
    from prego_amd.engine import ANT_KEYS
    from prego_amd.loss import OadAntLoss
    from prego_amd.trainer import _allreduce_grads
    cfg = case_cfg("g13a")
    rgb, flow, tgt, ant = (torch.from_numpy(x).to(DEV) for x in case_batch("g13a"))

    def grads(model):
        OadAntLoss(cfg)(model(rgb, flow), tgt, ant).backward()
        _allreduce_grads(model)
        torch.cuda.synchronize()
        model.engine(train=True).check()
        return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}

    ref = grads(_model(cfg, "bf16"))
    calls = []
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a, **k: 0)
    monkeypatch.setattr(dist, "all_reduce", lambda t, op=None, **k: (calls.append(t.numel()), t.mul_(2))[1])
    m2 = _model(cfg, "bf16")
    got = grads(m2)
    eng = m2.engine(train=True)
    lo, hi = eng._grad_bounds[0]
    for k in ANT_KEYS + ("f_classification.0.weight", "f_classification.0.bias"):
        o, n = eng._grad_offsets[k]
        assert lo <= o and o + n <= hi, k
    assert eng._grad_bounds[2][1] == eng._guard_off + 64           # the guard slot ends the last sub-bucket
    assert len(calls) == 3 and sum(calls) == eng._grad_flat.numel()
    for k in ref:
        assert torch.equal(got[k], ref[k]), k                      # x 2 / 2 is exact


def test_main_trains_checkpoints_and_reevaluates_miniroada(tmp_path, monkeypatch):
    import yaml
    from prego_amd import main as M
    cfg = epoch_cfg(str(tmp_path / "data"))
    cfg.update(output_path=str(tmp_path / "out"), num_epoch=1, num_workers=0, batch_size=4)
    for k in ("eval", "amp", "tensorboard", "lr_scheduler", "no_rgb", "no_flow", "config", "compute_dtype"):
        cfg.pop(k, None)                              # argparse supplies these (main.py:16-24); --compute_dtype defaults to fp16
    ypath = tmp_path / "cfg.yaml"
    yaml.safe_dump(cfg, open(ypath, "w"))
    monkeypatch.chdir(tmp_path)
    best = M.main(["--config", str(ypath)])
    assert 0.0 < best <= 1.0
    ck = glob.glob(str(tmp_path / "out" / "*" / "ckpts" / "best_*.pth"))
    assert len(ck) == 1, ck
    sd = torch.load(ck[0], map_location="cpu")
    assert set(sd) == {"layer1.0.weight", "layer1.0.bias", "layer1.1.weight", "layer1.1.bias", "gru.weight_ih_l0", "gru.weight_hh_l0",
                       "gru.bias_ih_l0", "gru.bias_hh_l0", "f_classification.0.weight", "f_classification.0.bias",
                       "anticipation_layer.0.weight", "anticipation_layer.0.bias"}
    mAP = M.main(["--config", str(ypath), "--eval", ck[0]])
    assert abs(mAP - best) < 1e-6                     # the checkpoint reproduces the epoch's eval
