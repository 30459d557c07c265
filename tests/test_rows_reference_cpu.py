"""CPU tests of tests/helpers/rows_exact.py, the references and input families tests/test_gpu_rows.py holds the row-wise training kernels
to: (1) the fp64 references agree with torch (float64, CPU) and its autograd; (2) every "exact" family really is exact - the fp32
evaluation in two summation orders, with and without an emulated fused multiply-add, equals the fp64 result bit for bit; (3) the very
assertions the GPU tests use (rows_exact.assert_exact / assert_within) reject subtly wrong kernels, modelled as numpy mutants of the
references."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import rows_exact as rx

SEED, ROW0 = 0x5EED, 7


def _gen(k=0):
    return np.random.default_rng(1234 + k)


def _t64(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.float64)


# ---- (1) references against torch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [0, 1])
def test_layernorm_relu_reference_and_its_backward_agree_with_torch_autograd(relu):
    g = _gen(relu)
    R, E = 5, 768
    Y, gamma, beta = rx.ln_inputs(R, E, g)
    out, mu, rstd = rx.ln_relu_ref(Y, gamma, beta, 1e-5, relu, 0.0, 0, 0)
    y = _t64(Y).requires_grad_(True)
    gm, bt = _t64(gamma).requires_grad_(True), _t64(beta).requires_grad_(True)
    o = F.layer_norm(y, (E,), gm, bt, float(np.float32(1e-5)))
    o = F.relu(o) if relu else o
    assert np.allclose(out, o.detach().numpy(), rtol=1e-12, atol=1e-12)
    dE = g.standard_normal((R, E))
    o.backward(_t64(dE))
    a = dict(Y=Y, dE=dE, gamma=gamma, beta=beta, stats=np.stack([mu, rstd], 1), prior=np.zeros((R, E)))
    dY, dgam, dbet, _ = rx.ln_bwd_ref(a, relu, 0.0, 0, 0, 0)
    assert np.allclose(dY, y.grad.numpy(), rtol=1e-10, atol=1e-12)
    assert np.allclose(dgam, gm.grad.numpy(), rtol=1e-10, atol=1e-12) and np.allclose(dbet, bt.grad.numpy(), rtol=1e-10, atol=1e-12)


def test_gelu_derivative_reference_agrees_with_torch_autograd():
    u = np.concatenate([np.geomspace(1e-4, 12, 200), -np.geomspace(1e-4, 12, 200)])
    df = _gen().standard_normal(u.size)
    x = _t64(u).requires_grad_(True)
    torch.nn.GELU()(x).backward(_t64(df))
    assert np.allclose(rx.gelu_bwd_ref(df, u, 0.0, 0), x.grad.numpy(), rtol=1e-11, atol=1e-300)


def test_gru_step_reference_agrees_with_grucell_autograd():
    """one reverse step: gate order r, z, n; carry_z is the direct path dh z, dGI / dGH the gradients of the two pre-activation terms"""
    g = _gen()
    B, H, I = 3, 8, 5
    cell = torch.nn.GRUCell(I, H).double()
    x, hprev = _t64(g.standard_normal((B, I))), _t64(g.standard_normal((B, H))).requires_grad_(True)
    gi = (x @ cell.weight_ih.T + cell.bias_ih).detach().requires_grad_(True)
    gh = (hprev @ cell.weight_hh.T + cell.bias_hh).detach().requires_grad_(True)
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    hp = hprev.detach().requires_grad_(True)
    h = (1 - z) * n + z * hp
    assert torch.allclose(h, cell(x, hprev), rtol=1e-12, atol=1e-12)
    dh = g.standard_normal((B, H))
    h.backward(_t64(dh))
    a = dict(r=r.detach().numpy(), z=z.detach().numpy(), n=n.detach().numpy(), ghn=gh.detach().numpy()[:, 2 * H:], hprev=hp.detach().numpy(),
             dHout=dh, carry=np.zeros((B, H)), dhpart=np.zeros((B, H)))
    carry, dgi, dgh = rx.gru_bwd_ref(a, 0, 1)
    assert np.allclose(dgi, gi.grad.numpy(), rtol=1e-10, atol=1e-13) and np.allclose(dgh, gh.grad.numpy(), rtol=1e-10, atol=1e-13)
    # dL/dh_{t-1} = carry_z + dGH W_hh
    assert np.allclose(carry + dgh @ cell.weight_hh.detach().numpy(), hp.grad.numpy() + (_t64(dgh) @ cell.weight_hh.detach()).numpy(), rtol=1e-10)
    assert np.allclose(carry, hp.grad.numpy(), rtol=1e-10, atol=1e-13)
    # na_next: rows below it add carry_z_in + dhpart, rows at and above it do not
    a2 = dict(a, carry=np.ones((B, H)), dhpart=np.ones((B, H)))
    c2, _, _ = rx.gru_bwd_ref(a2, 2, 1)
    assert np.allclose(c2[:2], (dh[:2] + 2) * a["z"][:2]) and np.allclose(c2[2:], carry[2:])
    # t = 0: hprev is zero whatever the array holds
    c0, gi0, _ = rx.gru_bwd_ref(a, 0, 0)
    assert np.allclose(gi0[:, H:2 * H], dh * (0 - a["n"]) * a["z"] * (1 - a["z"]))


def test_adamw_reference_agrees_with_torch_for_two_steps():
    g = _gen()
    hp = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.05)
    f = lambda x: float(np.float32(x))      # noqa: E731  (the reference takes the fp32-valued hyper-parameters)
    p0 = g.standard_normal(50)
    pt = _t64(p0.copy()).requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=f(hp["lr"]), betas=(f(hp["b1"]), f(hp["b2"])), eps=f(hp["eps"]), weight_decay=f(hp["wd"]))
    p, m, v = p0, np.zeros(50), np.zeros(50)
    for step in (1, 2):
        gr = g.standard_normal(50)
        pt.grad = _t64(gr)
        opt.step()
        p, m, v, *_ = rx.adamw_ref(p, gr, m, v, step, **hp)
        assert np.allclose(p, pt.detach().numpy(), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_loss_reference_agrees_with_torch(reduction):
    g = _gen()
    n, C = 6, 22
    l = g.standard_normal((n, C)) * 3
    tg = (g.random((n, C)) < 0.15).astype(np.float64)
    tg[2] = 0
    lt = _t64(l).requires_grad_(True)
    per = (-F.normalize(_t64(tg), dim=1) * F.log_softmax(lt, dim=1)).sum(1)
    loss = per.mean() if reduction == "mean" else per.sum()
    (loss * 128).backward()
    ref, dl, d_loss, d_dl = rx.oad_loss_ref(l, tg, 128.0, reduction)
    assert np.isclose(ref, float(loss.detach()), rtol=1e-12) and np.allclose(dl, lt.grad.numpy(), rtol=1e-10, atol=1e-13)
    assert d_loss > 0 and (d_dl >= 0).all() and (d_dl[2] == 0).all() and d_loss < 1e-4 * max(1.0, abs(ref))      # row 2: y = 0, dlogits exactly 0


def test_conversion_reference_is_round_to_nearest_even_and_saturates():
    x = rx.finite_values(4096, _gen(), rx.TBF)
    fin = np.isfinite(x)
    got = rx.convert(torch.from_numpy(x), rx.TBF).view(torch.int16).numpy().view(np.uint16)
    assert (got[fin] == rx.bf16_rne_bits(x[fin])).all()
    h = rx.convert(torch.from_numpy(rx.edge_values(rx.TF16)), rx.TF16).to(torch.float64).numpy()
    assert np.isfinite(h).all() and np.abs(h).max() == 65504.0
    e = rx.edge_values(rx.TF16)
    assert float(rx.convert(torch.tensor([e[0]]), rx.TF16)) == 1.0 and float(rx.convert(torch.tensor([e[1]]), rx.TF16)) == 1 + 2.0 ** -9      # ties to even
    # the keep mask: the threshold of p = 0.1 is taken from the fp32 value of p, as on the device
    assert rx.keep_mask(SEED, 3, 100, 0.1).tolist() == rx.keep_mask(SEED, 0, 103, 0.1)[3:].tolist()
    assert float(rx.drop_scale(0.2)) == 1.25


def test_plan_rows_is_the_packed_time_major_layout():
    rowoff, order, rows = rx.plan_rows([3, 5, 1])
    assert rowoff.tolist() == [0, 3, 5, 7, 8, 9] and order.tolist() == [1, 0, 2]
    assert rows[:3] == [(0, 1), (0, 0), (0, 2)] and rows[-1] == (4, 1)
    H = torch.arange(9, dtype=torch.float32)[:, None].repeat(1, 2)
    hp = rx.build_hprev_ref(H, [3, 5, 1], rx.T32)
    assert hp[:3].abs().sum() == 0 and hp[3, 0] == 0 and hp[4, 0] == 1 and hp[8, 0] == 7


# ---- (2) the exactness claims ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [256, 512, 1024, 2048, 4096])
@pytest.mark.parametrize("relu,p,acc", [(1, 0.0, 0), (1, 0.2, 1), (0, 0.2, 0)])
def test_ln_bwd_family_is_exact_in_fp32_in_any_order_with_and_without_fma(E, relu, p, acc):
    a = rx.ln_bwd_inputs(6, E, _gen(E))
    assert rx.ln_bwd_is_exact(a, relu, p, SEED, ROW0, acc)
    want = rx.ln_bwd_ref(a, relu, p, SEED, ROW0, acc)
    assert (want[3] == 0).any(), "the family must put pre-activations exactly on zero (ReLU's gradient there is zero)"
    for order in (1, -1):
        for fma in (False, True):
            got = rx.ln_bwd_ref(a, relu, p, SEED, ROW0, acc, fp=np.float32, order=order, fma=fma)
            for w, gt in zip(want[:3], got[:3]):
                assert gt.dtype == np.float32 and (gt.astype(np.float64) == w).all()


def test_ln_bwd_bound_covers_the_fp32_evaluation_where_the_means_do_not_divide():
    for E in (768, 2304):
        a = rx.ln_bwd_inputs(5, E, _gen(E))
        want, bound = rx.ln_bwd_ref(a, 1, 0.2, SEED, ROW0, 1)[0], rx.ln_bwd_dy_bound(a, 1, 0.2, SEED, ROW0, 1)
        for fma in (False, True):
            got = rx.ln_bwd_ref(a, 1, 0.2, SEED, ROW0, 1, fp=np.float32, order=-1, fma=fma)[0]
            assert rx.assert_within(got, want, bound, f"E {E}") > 0      # inexact indeed, inside the bound


@pytest.mark.parametrize("H,na,na_next,t", [(64, 3, 2, 1), (512, 3, 3, 0), (64, 1, 0, 2)])
def test_gru_bwd_family_is_exact_in_fp32_with_and_without_fma(H, na, na_next, t):
    a = rx.gru_bwd_inputs(na, H, _gen(H + na))
    assert rx.gru_bwd_product_bits(a, na_next, t) <= rx.GRU_PRODUCT_BITS
    want = rx.gru_bwd_ref(a, na_next, t)
    for fma in (False, True):
        got = rx.gru_bwd_ref(a, na_next, t, fp=np.float32, fma=fma)
        assert all((gt.astype(np.float64) == w).all() for w, gt in zip(want, got))
    assert all(rx.exact32(w) for w in want)


def test_integer_sums_are_exact_in_any_order():
    src = rx.int_matrix(1030, 65, _gen())
    assert rx.sum_is_exact(src, 1.0, 0)
    s32 = src.astype(np.float32)
    fwd = np.add.accumulate(s32, 0, dtype=np.float32)[-1]
    rev = np.add.accumulate(s32[::-1], 0, dtype=np.float32)[-1]
    assert (fwd.astype(np.float64) == rx.colsum_ref(src)).all() and (rev == fwd).all()
    assert (rx.t32(src).to(torch.bfloat16).to(torch.float64).numpy() == src).all()       # exact in bf16 too


# ---- (3) the GPU tests' assertions reject subtly wrong kernels ---------------------------------------------------------------------------------------
def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()


@pytest.mark.parametrize("mutant", ["drop_dgamma_col", "skip_last_block", "relu_ge", "drop_shift", "no_row0", "mean_nrows"])
def test_ln_bwd_mutants_are_rejected(mutant):
    R, E = 5, 256          # nrows % 4 = 1: a last partial row block
    a = rx.ln_bwd_inputs(R, E, _gen(3))
    want = rx.ln_bwd_ref(a, 1, 0.2, SEED, ROW0, 0)
    bad = rx.ln_bwd_ref(a, 1, 0.2, SEED, ROW0, 0, mutant=mutant)
    names = ("dY", "dgamma", "dbeta")
    rx.assert_exact(rx.t32(want[0]), rx.t32(want[0]), "dY")           # the assertion passes on the reference itself
    hit = [n for n, w, b in zip(names, want, bad) if not (w == b).all()]
    assert hit, f"{mutant} changes nothing on this instance"
    for n, w, b in zip(names, want, bad):
        if n in hit:
            _rejected(lambda: rx.assert_exact(rx.t32(b), rx.t32(w), n))


@pytest.mark.parametrize("mutant", ["drop_shift", "no_row0"])
def test_ln_forward_dropout_mutants_are_rejected_by_the_zero_pattern_check(mutant):
    Y, gamma, beta = rx.ln_inputs(3, 512, _gen())
    want = rx.ln_relu_ref(Y, gamma, beta, 1e-5, 0, 0.2, SEED, ROW0)[0]
    bad = rx.ln_relu_ref(Y, gamma, beta, 1e-5, 0, 0.2, SEED, ROW0, mutant=mutant)[0]
    bound = rx.ln_forward_bounds(Y, gamma, beta, 1e-5, 512 // 64 + 6, float(rx.drop_scale(0.2)))[0]
    bound = np.where(want == 0, 0.0, bound)          # a dropped element is an exact zero
    rx.assert_within(want, want, bound, "reference")
    _rejected(lambda: rx.assert_within(bad, want, bound, mutant))


def test_colsum_and_transpose_and_conversion_mutants_are_rejected():
    src = rx.int_matrix(70, 33, _gen())
    _rejected(lambda: rx.assert_exact(rx.t32(rx.colsum_ref(src, "skip_last_block")), rx.t32(rx.colsum_ref(src)), "colsum"))
    x = torch.from_numpy(rx.finite_values(70 * 40, _gen(), rx.TBF)).view(70, 40)
    want = rx.transpose_ref(x, 70, 33, 128, rx.TBF)
    _rejected(lambda: rx.assert_exact(rx.transpose_ref(x, 70, 33, 128, rx.TBF, "pad_unwritten"), want, "pad rows"))
    _rejected(lambda: rx.assert_exact(rx.transpose_ref(x, 70, 33, 128, rx.TBF, "truncate"), want, "truncation"))
    e = torch.from_numpy(rx.edge_values(rx.TBF))
    _rejected(lambda: rx.assert_exact(rx.convert(e, rx.TBF, "truncate"), rx.convert(e, rx.TBF), "f32_to_bf16"))


@pytest.mark.parametrize("mutant,which", [("carry_1mz", 0), ("no_r_dgh", 2)])
def test_gru_bwd_mutants_are_rejected(mutant, which):
    a = rx.gru_bwd_inputs(3, 64, _gen())
    want, bad = rx.gru_bwd_ref(a, 2, 1), rx.gru_bwd_ref(a, 2, 1, mutant=mutant)
    _rejected(lambda: rx.assert_exact(rx.t32(bad[which]), rx.t32(want[which]), mutant))
    _rejected(lambda: rx.assert_exact(rx.convert(rx.t32(bad[which]), rx.TBF), rx.convert(rx.t32(want[which]), rx.TBF), mutant + " (bf16 copy)"))


@pytest.mark.parametrize("mutant,step", [("wd_after", 1), ("bc_step1", 2)])
def test_adamw_mutants_are_rejected(mutant, step):
    g = _gen()
    n = 4097
    f32 = lambda x: x.astype(np.float32).astype(np.float64)      # noqa: E731
    p, gr = f32(g.standard_normal(n)), f32(g.standard_normal(n))
    m, v = (np.zeros(n), np.zeros(n)) if step == 1 else (f32(0.1 * g.standard_normal(n)), f32(0.001 * g.random(n)))
    hp = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.05)
    want = rx.adamw_ref(p, gr, m, v, step, **hp)
    bad = rx.adamw_ref(p, gr, m, v, step, mutant=mutant, **hp)
    rx.assert_within(want[0].astype(np.float32), want[0], want[3], "fp32 rounding of the reference")
    _rejected(lambda: rx.assert_within(bad[0], want[0], want[3], mutant))


def test_bounds_are_tight_enough_to_mean_something():
    """a relative error of 1e-4 anywhere must not fit a bound of this module at the test shapes"""
    g = _gen()
    Y, gamma, beta = rx.ln_inputs(4, 4096, g)
    out = rx.ln_relu_ref(Y, gamma, beta, 1e-5, 0, 0.0, 0, 0)[0]
    b = rx.ln_forward_bounds(Y, gamma, beta, 1e-5, 4096 // 64 + 6)[0]
    assert np.median(b / np.maximum(np.abs(out), 1e-3)) < 1e-4
    a = rx.head_inputs(5, 2, 1536, 22, g)
    lg, bl = rx.head_ref(a)
    y = rx.ln_relu_ref(a["x"][:, 0, :], a["lnw"], a["lnb"], 1e-5, 0, 0.0, 0, 0)[0]
    assert (bl < 1e-4 * (np.abs(y) @ np.abs(a["hw"]).T)).all()      # relative to the dot product's terms: the logits themselves cancel
    u = np.geomspace(1e-4, 12, 64)
    assert (rx.gelu_bwd_bound(np.ones(64), u, 0.0, 0) < 3e-5 * np.maximum(np.abs(rx.gelu_bwd_ref(np.ones(64), u, 0.0, 0)), 1e-3) * 10).all()
