"""CPU tests of MiniROADA training's host side: TRAINER["ANTICIPATION"] (trainer/train.py:31-54) and the PAD entries of the anticipation
data layer that a data-parallel epoch's short last batch needs."""
import inspect

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def test_anticipation_trainer_resolves_with_the_reference_parameter_order():
    import prego_amd.trainer  # noqa: F401
    from prego_amd.registry import TRAINER, build_trainer
    fn = TRAINER["ANTICIPATION"]
    assert fn.__name__ == "ant_train_one_epoch" and build_trainer({"task": "ANTICIPATION"}) is fn
    params = list(inspect.signature(fn).parameters.values())
    # train.py:31: ant_train_one_epoch(trainloader, model, criterion, optimizer, scaler, epoch, writer=None, scheduler=None)
    assert [p.name for p in params[:8]] == ["trainloader", "model", "criterion", "optimizer", "scaler", "epoch", "writer", "scheduler"]
    assert params[8].name == "device" and params[8].kind is inspect.Parameter.KEYWORD_ONLY and params[8].default is None


def test_pad_entries_yield_zero_targets(tmp_path):
    from scripts.gen_golden_anticipation import make_tree
    import prego_amd.data  # noqa: F401
    from prego_amd.registry import DATA_LAYERS
    cfg = make_tree(str(tmp_path))
    ds = DATA_LAYERS[cfg["data_name"]](cfg, "train")
    n = len(ds)
    assert n > 0
    for i in (0, n - 1):
        rgb, flow, tgt, ant = ds[i]
        prgb, pflow, ptgt, pant = ds[i + n]
        assert torch.equal(rgb, prgb) and torch.equal(flow, pflow)
        assert ptgt.shape == tgt.shape and pant.shape == ant.shape
        assert not ptgt.any() and not pant.any()
    with pytest.raises(IndexError):
        ds[2 * n]


class _Stub(torch.nn.Module):
    """CPU stand-in for MROADA's training forward: a linear map of the input to logits and anticipation logits"""

    def __init__(self, d, L, C):
        super().__init__()
        self.f = torch.nn.Linear(d, C)
        self.a = torch.nn.Linear(d, L * C)
        self.L, self.C = L, C

    def forward(self, rgb, flow):
        x = torch.cat((rgb, flow), -1)
        B, T = x.shape[:2]
        return {"logits": self.f(x), "anticipation_logits": self.a(x).view(B, T, self.L, self.C)}


class _AntLossTorch(torch.nn.Module):          # OadAntLoss restated in torch (the shipped one runs on the GPU only)
    reduction = "sum"

    def forward(self, out, target, ant_target):
        C = ant_target.shape[-1]
        last = out["anticipation_logits"][:, -1].reshape(-1, C)
        return torch.sum(-torch.nn.functional.normalize(ant_target.reshape(-1, C)) * torch.log_softmax(last, -1))


def test_single_process_epoch_is_the_sum_of_step_losses():
    from prego_amd.registry import TRAINER
    import prego_amd.trainer  # noqa: F401
    torch.manual_seed(0)
    m = _Stub(6, 2, 5)
    g = torch.Generator().manual_seed(1)
    batches = [(torch.randn(3, 4, 3, generator=g), torch.randn(3, 4, 3, generator=g),
                torch.zeros(3, 4, 5), torch.nn.functional.one_hot(torch.randint(0, 5, (3, 2), generator=g), 5).float()) for _ in range(2)]
    ref = _Stub(6, 2, 5)
    ref.load_state_dict(m.state_dict())
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    ropt = torch.optim.SGD(ref.parameters(), lr=0.1)
    loss = TRAINER["ANTICIPATION"](batches, m, _AntLossTorch(), opt, None, 1, device="cpu")
    want = 0.0
    for rgb, flow, tgt, ant in batches:
        ropt.zero_grad()
        lv = _AntLossTorch()(ref(rgb, flow), tgt, ant)
        lv.backward()
        ropt.step()
        want += lv.item()
    assert abs(loss - want) < 1e-5
    for k, v in ref.state_dict().items():
        assert torch.allclose(m.state_dict()[k], v, atol=1e-6), k
    assert np.isfinite(loss)


def _ant_batches():
    g = torch.Generator().manual_seed(5)
    B, T, L, C = 6, 4, 2, 5
    rgb, flow = torch.randn(B, T, 3, generator=g), torch.randn(B, T, 3, generator=g)
    tgt = torch.zeros(B, T, C)
    ant = torch.nn.functional.one_hot(torch.randint(0, C, (B, L), generator=g), C).float()
    ant[1] = 0.0                                      # a PAD-like window: zero loss, zero gradient
    return rgb, flow, tgt, ant


def _ant_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from prego_amd import distributed as D
    from prego_amd.registry import TRAINER
    import prego_amd.trainer  # noqa: F401
    if world > 1:
        D.init_from_env("gloo")
    rgb, flow, tgt, ant = _ant_batches()
    per = rgb.shape[0] // world
    sl = slice(rank * per, (rank + 1) * per)          # every rank its own windows
    torch.manual_seed(0)
    model = _Stub(6, 2, 5)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    loss = TRAINER["ANTICIPATION"]([(rgb[sl], flow[sl], tgt[sl], ant[sl])], model, _AntLossTorch(), opt, None, 1, device="cpu")
    q.put((rank, float(loss), [p.detach().numpy().tolist() for p in model.parameters()]))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_reach_the_single_process_global_step_and_loss():
    """gloo world 2, different local batches, OadAntLoss restated with reduction 'sum': the weights after the step equal the
    single-process step over the global batch (the all-reduced mean scaled by the world size), and every rank returns the global loss"""
    import socket
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    res = {}
    for world in (1, 2):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        q = ctx.Queue()
        procs = [ctx.Process(target=_ant_worker, args=(r, world, port, q)) for r in range(world)]
        for p in procs:
            p.start()
        res[world] = sorted(q.get(timeout=300) for _ in range(world))
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    (_, loss1, w1), = res[1]
    for rank, loss2, w2 in res[2]:
        assert abs(loss2 - loss1) <= 1e-5 * abs(loss1), (rank, loss2, loss1)
        for a, b in zip(w1, w2):
            assert torch.allclose(torch.tensor(a), torch.tensor(b), atol=1e-6)
    torch.manual_seed(0)
    assert not torch.allclose(torch.tensor(w1[2]), _Stub(6, 2, 5).a.weight)        # the step moved the anticipation weights


def test_a_criterion_without_reduction_keeps_the_oad_step_weight(monkeypatch):
    import prego_amd.trainer as TR
    seen = {}
    monkeypatch.setattr(TR, "_epoch", lambda *a, **k: seen.update(k) or 0.0)
    TR.ant_train_one_epoch([], torch.nn.Linear(1, 1), lambda *a: None, None, None, 1, device="cpu")
    assert seen.get("grad_weight") is None
