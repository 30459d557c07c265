"""GPU tests of MiniROADA training (model/rnn/rnn.py:113-130 in training mode, criterions/loss.py:40-79, trainer/train.py:31-54): the KEEP
forward of the anticipation head, its backward (csrc/ant_head_bwd.hip) through prego_miniroad_set_anticipation_grads, the fused AdamW
step of anticipation_layer and TRAINER["ANTICIPATION"].  The oracle is a torch fp32 restatement of the reference model (nn.GRU, nn.Linear,
LayerNorm) with the same weights, differentiated by torch autograd."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from prego_amd import weights as W                               # noqa: E402
from prego_amd.config import anticipation_cfg, assembly101_cfg  # noqa: E402

DEV = "cuda:0"
# G4b's tiers: loss relative, gradient max |diff| relative to the reference gradient's norm
LOSS_TOL = {"fp32": 1e-4, "bf16": 2e-2}
GRAD_TOL = {"fp32": 2e-3, "bf16": 6e-2}


def _cfg(hid, L, actionness=False, dtype="fp32"):
    return anticipation_cfg(assembly101_cfg(hidden_dim=hid, dropout=0.0, compute_dtype=dtype), L, actionness=actionness)


def _model(cfg, sd):
    import prego_amd.model  # noqa: F401
    from prego_amd.registry import build_model
    m = build_model(cfg, DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.train()


def _inputs(B, T, seed=5, zero_flow=False):
    rgb = torch.from_numpy(W.tsn_features((B, T, 2048), seed, "rgb")).to(DEV)
    flow = torch.zeros_like(rgb) if zero_flow else torch.from_numpy(W.tsn_features((B, T, 2048), seed, "flow")).to(DEV)
    return rgb, flow


def _ant_target(B, L, C, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.one_hot(torch.randint(0, C, (B, L), generator=g), C).float().to(DEV)


class _Ref(torch.nn.Module):
    """rnn.py:113-130 in training mode, fp32 torch"""

    def __init__(self, sd, hid, L, C):
        super().__init__()
        self.layer1 = torch.nn.Sequential(torch.nn.Linear(4096, 2048), torch.nn.LayerNorm(2048), torch.nn.ReLU())
        self.gru = torch.nn.GRU(2048, hid, 1, batch_first=True)
        self.f_classification = torch.nn.Sequential(torch.nn.Linear(hid, C))
        self.anticipation_layer = torch.nn.Sequential(torch.nn.Linear(hid, L * hid))
        self.L, self.H = L, hid
        self.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if not k.startswith("f_actionness")})
        self.to(DEV)

    def forward(self, rgb, flow):
        x = self.layer1(torch.cat((rgb, flow), 2))
        h, _ = self.gru(x, torch.zeros(1, x.shape[0], self.H, device=x.device))
        h = torch.relu(h)
        B, T = h.shape[0], h.shape[1]
        a = torch.relu(self.anticipation_layer(h)).view(B, T, self.L, self.H)
        return {"logits": self.f_classification(h), "anticipation_logits": self.f_classification(a)}


def _ant_loss_torch(out, ant_target):          # OadAntLoss, reduction 'sum' (loss.py:40-79)
    C = ant_target.shape[-1]
    last = out["anticipation_logits"][:, -1].reshape(-1, C)
    return torch.sum(-torch.nn.functional.normalize(ant_target.reshape(-1, C)) * torch.log_softmax(last, -1))


def _dense_weights(out):
    g = torch.Generator().manual_seed(11)
    return {k: torch.randn(v.shape, generator=g).to(DEV) for k, v in out.items()}


def _dense_loss(out, wts):
    return (out["logits"] * wts["logits"]).sum() + (out["anticipation_logits"] * wts["anticipation_logits"]).sum()


def _grads(model):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}


def _check_grads(got, ref, tol, what):
    for k, r in ref.items():
        g = got[k]
        assert g is not None, f"{what}: {k} has no gradient"
        err = float((g - r).abs().max())
        scale = float(r.norm())
        assert err <= tol * max(scale, 1e-12), f"{what}: {k} max |dg| {err:.3e} > {tol} x |g| {scale:.3e}"


@pytest.mark.parametrize("dtype,hid,L,B,T,loss_kind,zero_flow,actionness", [
    ("fp32", 1024, 4, 2, 8, "ant", False, True),
    ("bf16", 1024, 4, 2, 8, "ant", False, True),
    ("fp32", 512, 1, 3, 8, "ant", False, False),
    ("bf16", 512, 1, 3, 8, "ant", False, False),
    ("fp32", 512, 3, 2, 8, "dense", False, False),
    ("bf16", 512, 3, 2, 8, "dense", False, False),
    ("bf16", 1024, 8, 16, 128, "ant", True, False),
])
def test_training_step_matches_torch(dtype, hid, L, B, T, loss_kind, zero_flow, actionness):
    from prego_amd.loss import OadAntLoss
    cfg = _cfg(hid, L, actionness, dtype)
    sd = W.miniroad_a_state_dict(cfg, seed=21)
    m = _model(cfg, sd)
    ref = _Ref(sd, hid, L, 86)
    rgb, flow = _inputs(B, T, zero_flow=zero_flow)
    tgt = torch.zeros(B, T, 86, device=DEV)
    ant_t = _ant_target(B, L, 86)
    out = m(rgb, flow)
    assert out["logits"].shape == (B, T, 86) and out["anticipation_logits"].shape == (B, T, L, 86)
    out_r = ref(rgb, flow)
    if loss_kind == "ant":
        loss = OadAntLoss(cfg)(out, tgt, ant_t)
        loss_r = _ant_loss_torch(out_r, ant_t)
    else:
        wts = _dense_weights(out_r)
        loss, loss_r = _dense_loss(out, wts), _dense_loss(out_r, wts)
    loss.backward()
    loss_r.backward()
    lv, lr = float(loss), float(loss_r)
    assert abs(lv - lr) <= LOSS_TOL[dtype] * max(1.0, abs(lr)), f"loss {lv} vs {lr}"
    got = _grads(m)
    _check_grads(got, _grads(ref), GRAD_TOL[dtype], f"{dtype} {loss_kind} H{hid} L{L}")
    if actionness:
        assert got["f_actionness.0.weight"] is None and got["f_actionness.0.bias"] is None


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_training_logits_equal_miniroad_and_ant_logits_match_inference(dtype):
    import prego_amd.model  # noqa: F401
    from prego_amd.registry import build_model
    cfg = _cfg(1024, 4, dtype=dtype)
    sd = W.miniroad_a_state_dict(cfg, seed=22)
    m = _model(cfg, sd)
    trunk = build_model(assembly101_cfg(dropout=0.0, compute_dtype=dtype), DEV)
    trunk.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if not k.startswith("anticipation")})
    trunk.train()
    rgb, flow = _inputs(3, 16)
    with torch.no_grad():
        out = m(rgb, flow)
        base = trunk(rgb, flow)["logits"]
    assert torch.equal(out["logits"], base)
    m.eval()
    _, _, _, ant, _ = m.engine().forward_ragged([rgb[b] for b in range(3)], [flow[b] for b in range(3)], softmax=False, want_ant=True)
    err = float((out["anticipation_logits"] - torch.stack(ant, 0)).abs().max())
    assert err < {"fp32": 1e-3, "bf16": 1e-2}[dtype], err


def test_logits_only_loss_leaves_the_trunk_bits_of_miniroad():
    import prego_amd.model  # noqa: F401
    from prego_amd.registry import build_model
    cfg = _cfg(1024, 4, dtype="bf16")
    sd = W.miniroad_a_state_dict(cfg, seed=23)
    m = _model(cfg, sd)
    trunk = build_model(assembly101_cfg(dropout=0.0, compute_dtype="bf16"), DEV)
    trunk.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if not k.startswith("anticipation")})
    trunk.train()
    rgb, flow = _inputs(4, 16)
    wl = torch.randn(4, 16, 86, generator=torch.Generator().manual_seed(1)).to(DEV)
    (m(rgb, flow)["logits"] * wl).sum().backward()
    (trunk(rgb, flow)["logits"] * wl).sum().backward()
    ga, gb = _grads(m), _grads(trunk)
    for k, g in gb.items():
        assert torch.equal(ga[k], g), k
    assert not ga["anticipation_layer.0.weight"].any() and not ga["anticipation_layer.0.bias"].any()


def test_backward_without_anticipation_grads_is_refused():
    from prego_amd._lib import PregoError
    from prego_amd.engine import MiniRoadEngine
    cfg = _cfg(512, 2, dtype="bf16")
    sd = {k: torch.from_numpy(v) for k, v in W.miniroad_a_state_dict(cfg, seed=24).items()}
    e = MiniRoadEngine(2048, 2048, 2048, 512, 86, DEV, "bf16")
    e.set_weights(sd)
    e.set_anticipation(sd["anticipation_layer.0.weight"], sd["anticipation_layer.0.bias"], 2)
    rgb, flow = _inputs(2, 8)
    e.forward_train(rgb, flow, want_ant=True)
    e._train_ant = False                     # as if the caller forgot the anticipation gradients
    with pytest.raises(PregoError, match="set_anticipation_grads"):
        e.backward(torch.zeros(2, 8, 86, device=DEV))


@pytest.mark.parametrize("pattern", ["last", "middle", "first"])
def test_span_equals_full_range(pattern):
    from prego_amd import _lib
    from prego_amd.engine import ANT_KEYS, MiniRoadEngine
    dbg = _lib.load_debug()
    cfg = _cfg(1024, 8, dtype="bf16")
    sd = {k: torch.from_numpy(v) for k, v in W.miniroad_a_state_dict(cfg, seed=25).items()}
    e = MiniRoadEngine(2048, 2048, 2048, 1024, 86, DEV, "bf16", lib=dbg)
    e.set_weights(sd)
    e.set_anticipation(sd[ANT_KEYS[0]], sd[ANT_KEYS[1]], 8)
    B, T = 16, 128
    rgb, flow = _inputs(B, T)
    g = torch.Generator().manual_seed(3)
    d_ant = torch.zeros(B, T, 8, 86)
    t = {"last": T - 1, "middle": T // 2, "first": 0}[pattern]
    d_ant[:, t] = torch.randn(B, 8, 86, generator=g)
    d_ant = d_ant.to(DEV)
    dl = torch.randn(B, T, 86, generator=g).to(DEV)
    res = []
    try:
        for full in (0, 1):
            dbg.prego_debug_ant_full_span(full)
            e.forward_train(rgb, flow, want_ant=True)
            res.append({k: v.clone() for k, v in e.backward(dl, d_ant).items()})
    finally:
        dbg.prego_debug_ant_full_span(0)
    torch.cuda.synchronize()
    for k, a in res[0].items():
        b = res[1][k]
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()), k
    assert res[0][ANT_KEYS[0]].abs().max() > 0


def test_fused_adamw_matches_torch_adamw_and_refreshes_the_eval_head():
    import prego_amd.model  # noqa: F401
    from prego_amd.loss import OadAntLoss
    from prego_amd.optim import FusedAdamW
    from prego_amd.registry import build_model
    cfg = _cfg(512, 3, actionness=True, dtype="fp32")
    sd = W.miniroad_a_state_dict(cfg, seed=26)
    ma, mb = _model(cfg, sd), _model(cfg, sd)
    oa = FusedAdamW(ma.parameters(), lr=1e-4, weight_decay=0.05, model=ma)
    ob = torch.optim.AdamW(mb.parameters(), lr=1e-4, weight_decay=0.05)
    assert oa.is_guarded_for(ma)
    crit = OadAntLoss(cfg)
    rgb, flow = _inputs(2, 8)
    tgt, ant_t = torch.zeros(2, 8, 86, device=DEV), _ant_target(2, 3, 86)
    for _ in range(3):
        for m, o in ((ma, oa), (mb, ob)):
            o.zero_grad(set_to_none=True)
            crit(m(rgb, flow), tgt, ant_t).backward()
            o.step()
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    for k in pb:
        err = float((pa[k] - pb[k]).abs().max())
        assert err <= 1e-6 + 1e-4 * float(pb[k].abs().max()), (k, err)
    assert torch.equal(pa["f_actionness.0.weight"].cpu(), torch.from_numpy(sd["f_actionness.0.weight"]))
    # the eval engine picks up the new anticipation weights: same bits as a fresh model loaded with the trained state_dict
    fresh = build_model(cfg, DEV)
    fresh.load_state_dict(ma.state_dict())
    ma.eval(); fresh.eval()
    with torch.no_grad():
        a, b = ma(rgb, flow), fresh(rgb, flow)
    assert torch.equal(a["anticipation_logits"], b["anticipation_logits"]) and torch.equal(a["logits"], b["logits"])


def test_is_guarded_for_with_and_without_actionness():
    from prego_amd.optim import FusedAdamW
    for act in (False, True):
        cfg = _cfg(512, 2, actionness=act, dtype="bf16")
        m = _model(cfg, W.miniroad_a_state_dict(cfg, seed=27))
        assert FusedAdamW(m.parameters(), lr=1e-4, model=m).is_guarded_for(m)


def _loader(B=4, T=8, L=3, n=5):
    out = []
    for i in range(n):
        rgb = torch.from_numpy(W.tsn_features((B, T, 2048), 40 + i, "rgb"))
        flow = torch.from_numpy(W.tsn_features((B, T, 2048), 40 + i, "flow"))
        g = torch.Generator().manual_seed(i)
        tgt = torch.nn.functional.one_hot(torch.randint(0, 86, (B, T), generator=g), 86).float()
        ant = torch.nn.functional.one_hot(torch.randint(0, 86, (B, L), generator=g), 86).float()
        out.append((rgb.pin_memory(), flow.pin_memory(), tgt.pin_memory(), ant.pin_memory()))
    return out


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_trainer_guarded_and_per_step_loops_agree(dtype):
    import prego_amd.trainer as TR
    from prego_amd.loss import OadAntLoss
    from prego_amd.optim import FusedAdamW
    from prego_amd.registry import TRAINER
    cfg = _cfg(512, 3, dtype=dtype)
    sd = W.miniroad_a_state_dict(cfg, seed=28)
    batches = _loader()
    res = []
    for guarded in (True, False):
        m = _model(cfg, sd)
        opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.05, model=m)
        old = TR.GUARDED_LOOP
        TR.GUARDED_LOOP = guarded
        try:
            loss = TRAINER["ANTICIPATION"](batches, m, OadAntLoss(cfg), opt, None, 1)
        finally:
            TR.GUARDED_LOOP = old
        res.append((loss, {k: v.detach().clone() for k, v in m.state_dict().items()}))
    assert res[0][0] == res[1][0] and np.isfinite(res[0][0]) and res[0][0] > 0
    for k, v in res[0][1].items():
        assert torch.equal(v, res[1][1][k]), k


def test_trainer_amp_runs_the_grad_scaler_protocol():
    from prego_amd.loss import OadAntLoss
    from prego_amd.optim import FusedAdamW
    from prego_amd.registry import TRAINER
    cfg = _cfg(512, 3, dtype="bf16")
    m = _model(cfg, W.miniroad_a_state_dict(cfg, seed=29))
    before = m.anticipation_layer[0].weight.detach().clone()
    opt = FusedAdamW(m.parameters(), lr=1e-3, model=m)
    loss = TRAINER["ANTICIPATION"](_loader(n=3), m, OadAntLoss(cfg), opt, torch.amp.GradScaler("cuda"), 1, device=DEV)
    assert np.isfinite(loss) and loss > 0
    assert not torch.equal(before, m.anticipation_layer[0].weight.detach())


def test_forward_and_backward_allocate_nothing_after_warm_up():
    """no device allocation in a warm MiniROADA step, and no host wait beyond MiniROAD's own (the pointer-table fence of stage_tables:
    run-ahead one call deep)"""
    from prego_amd import _lib
    from prego_amd.engine import ANT_KEYS, MiniRoadEngine
    dbg = _lib.load_debug()                  # the counters count the debug library's own host code: run the engine there
    cfg = _cfg(1024, 4, dtype="bf16")
    sd = {k: torch.from_numpy(v) for k, v in W.miniroad_a_state_dict(cfg, seed=30).items()}
    e = MiniRoadEngine(2048, 2048, 2048, 1024, 86, DEV, "bf16", lib=dbg)
    e.set_weights(sd)
    e.set_anticipation(sd[ANT_KEYS[0]], sd[ANT_KEYS[1]], 4)
    rgb, flow = _inputs(4, 32)
    d_ant = torch.randn(4, 32, 4, 86, device=DEV)
    dl = torch.randn(4, 32, 86, device=DEV)

    def counted(want_ant):
        torch.cuda.synchronize()
        a0, w0 = C.c_int64(), C.c_int64()
        dbg.prego_debug_alloc_count(C.byref(a0), C.byref(w0))
        e.forward_train(rgb, flow, want_ant=want_ant)
        e.backward(dl, d_ant if want_ant else None)
        a1, w1 = C.c_int64(), C.c_int64()
        dbg.prego_debug_alloc_count(C.byref(a1), C.byref(w1))
        torch.cuda.synchronize()
        return a1.value - a0.value, w1.value - w0.value

    for want in (True, False, True, False):       # warm-up: workspaces, plan tables, kernels
        counted(want)
    mallocs_a, waits_a = counted(True)
    mallocs_t, waits_t = counted(False)
    assert mallocs_a == 0 and mallocs_t == 0
    assert waits_a == waits_t
