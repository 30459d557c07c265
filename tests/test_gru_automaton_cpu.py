"""The saturated-gate automaton (tests/helpers/gru_automaton.py) held to the real GRU on the CPU: it IS nn.GRU's arithmetic on its state
dict (fp64 oracle, 1e-9; rounded: equal), the kernels' fp32 formulas reproduce it bit for bit, every run of tests/test_gpu_automaton.py
stays inside conditions(), one flipped state element shows in the same frame's logits, and the derived bounds of the gate functions
hold for a numpy-fp32 emulation of them."""
import numpy as np
import pytest
import torch

from oracle import oracle_np as O
from tests.helpers import gru_automaton as A

AMP32 = np.float32(A.AMP)
SMALL = {
    "l1": (A.Case(d_rgb=512, d_flow=0, emb=512, hid=512, n_classes=12, seed=101), [5, 31, 17, 48]),
    "l1-flow": (A.Case(d_rgb=256, d_flow=256, emb=512, hid=512, n_classes=22, seed=102), [9, 40, 1, 23]),
    "l2": (A.Case(d_rgb=512, d_flow=0, emb=512, hid=512, n_classes=12, num_layers=2, seed=103), [12, 33, 20]),
    "ant": (A.Case(d_rgb=512, d_flow=0, emb=512, hid=512, n_classes=12, ant_len=3, seed=104), [25, 7, 36]),
}


def _np(sd):
    return {k: v.numpy() for k, v in sd.items() if not k.startswith("anticipation")}


@pytest.mark.parametrize("name", sorted(SMALL))
@pytest.mark.parametrize("with_h0", [False, True], ids=["h0_zero", "h0_hostile"])
def test_automaton_equals_the_fp64_gru(name, with_h0):
    case, lens = SMALL[name]
    sd, meta = A.build_state_dict(case)
    feats = A.build_features(case, lens, 3)
    h0 = A.hostile_h0(case, len(lens), 3) if with_h0 else None
    res = A.run(sd, meta, case, feats, h0=h0)
    A.conditions(sd, case, res, want_ties=False)
    for i, (r, f) in enumerate(feats):
        h0i = None if h0 is None else h0[..., i:i + 1, :].numpy()
        ref = O.miniroad_forward(_np(sd), r.numpy()[None], None if f is None else f.numpy()[None], training=True, h0=h0i, keep=True)
        h = res.clip(res.h[-1], i).numpy().astype(np.float64)
        assert np.abs(ref["h"][0] - h).max() < 1e-9 and np.array_equal(np.rint(ref["h"][0]), h)
        lg = res.clip(res.logits, i).numpy()
        assert np.abs(ref["raw_logits"][0] - lg).max() < 1e-9 and np.array_equal(np.rint(ref["raw_logits"][0]), lg)
        hl = ref["h_last"][:, 0] if case.num_layers == 2 else ref["h_last"][0]
        assert np.array_equal(np.rint(hl), res.h_last[..., i, :].numpy())
        if case.ant_len:                       # MROADA.forward on the fp64 states: relu(anticipation_layer(relu(h))) viewed [T, L, H], then the SAME classifier
            wa, ba = sd["anticipation_layer.0.weight"].numpy().astype(np.float64), sd["anticipation_layer.0.bias"].numpy().astype(np.float64)
            wc, bc = sd["f_classification.0.weight"].numpy().astype(np.float64), sd["f_classification.0.bias"].numpy().astype(np.float64)
            a = np.maximum(np.maximum(ref["h"][0], 0) @ wa.T + ba, 0).reshape(lens[i], case.ant_len, case.hid)
            al = a @ wc.T + bc
            got = res.clip(res.ant_logits, i).numpy()
            assert np.abs(al - got).max() < 1e-8 and np.array_equal(np.rint(al), got)
            assert np.array_equal(res.clip(res.ant_argmax, i).numpy(), np.argmax(got, axis=-1))      # np.argmax: first maximum


def test_layernorm_makes_c_of_a_one_bit():
    case, lens = SMALL["l1-flow"]
    sd, meta = A.build_state_dict(case)
    r, f = A.build_features(case, [40], 4)[0]
    x = np.concatenate([r.numpy(), f.numpy()], axis=1).astype(np.float64)
    y = x[:, meta["sigma"]]
    assert np.array_equal(y, x @ sd["layer1.0.weight"].numpy().astype(np.float64).T)
    e = np.maximum(O.layernorm(y, 1.0, 0.0), 0.0)
    p = y.mean(axis=1, keepdims=True)
    c = (1 - p) / np.sqrt(p * (1 - p) + A.LN_EPS)
    assert np.abs(e - c * y).max() < 1e-12


@pytest.mark.parametrize("hid", [512, 1024, 2048])
def test_fp32_formulas_reproduce_the_automaton_bit_for_bit(hid):
    """sigmoidf_ / tanhf_ / (1 - z) n + z h in numpy fp32 (exp rounded to fp32, IEEE division for rcp), gi from a fp32 LayerNorm:
    300 steps of 32 clips give the automaton's states exactly"""
    case = A.Case(d_rgb=512, d_flow=0, emb=512, hid=hid, seed=110 + hid)
    sd, meta = A.build_state_dict(case)
    feats = A.build_features(case, [300] * 32, 5)
    res = A.run(sd, meta, case, feats)
    A.conditions(sd, case, res, want_ties=False)
    x = torch.stack([r for r, _ in feats]).numpy()                       # [32, 300, 512]
    y = x[:, :, meta["sigma"]]
    mu = y.mean(axis=-1, keepdims=True, dtype=np.float32)
    var = ((y - mu) ** 2).mean(axis=-1, keepdims=True, dtype=np.float32)
    e = np.maximum((y - mu) / np.sqrt(var + np.float32(A.LN_EPS)), np.float32(0)).astype(np.float32)
    w_ih, b_ih = sd["gru.weight_ih_l0"].numpy(), sd["gru.bias_ih_l0"].numpy()
    gi = (AMP32 * e[:, :, meta["pi"][0]] + b_ih).astype(np.float32)
    assert np.array_equal(np.nonzero(w_ih)[1], meta["pi"][0])
    w_hh, b_hh = sd["gru.weight_hh_l0"].numpy(), sd["gru.bias_hh_l0"].numpy()
    h = np.zeros((32, hid), np.float32)
    want = res.h[0].view(32, 300, hid).numpy()
    for t in range(300):
        h = A.gru_step_f32(gi[:, t], h, w_hh, b_hh)
        assert np.array_equal(h, want[:, t].astype(np.float32)), t


def _cond_param(rid):
    r = A.RUNS[rid]
    return pytest.param(rid, marks=[pytest.mark.slow] if r.get("big") else [])


@pytest.mark.parametrize("rid", [_cond_param(r) for r in A.RUNS])
def test_every_gpu_run_stays_inside_its_conditions(rid):
    """the runs of tests/test_gpu_automaton.py, on the CPU: the same feature bits, except for the large runs (marked slow), whose bits
    the GPU file draws with the device's generator: for those this proves the construction, not the very inputs, and the GPU file checks
    conditions() again on what it drew before it looks at a kernel's output"""
    st = A.reference(rid)[-1].stats
    print(rid, {k: v for k, v in st.items() if k != "flips"})


def test_one_flipped_unit_shows_in_the_same_frames_logits():
    case = A.Case(seed=120)
    sd, meta = A.build_state_dict(case)
    feats = A.build_features(case, [12] * 40, 6)
    base = A.run(sd, meta, case, feats)
    rng = np.random.default_rng(1)
    h0 = base.h[0].view(40, 12, case.hid)[:, 3].to(torch.float32).clone()           # restart every clip from its state after frame 3 ...
    tail = [(r[4:].contiguous(), None) for r, _ in feats]
    same = A.run(sd, meta, case, tail, h0=h0)
    assert torch.equal(same.logits.view(40, 8, -1), base.logits.view(40, 12, -1)[:, 4:])
    unit = np.asarray([rng.choice(np.flatnonzero(row)) for row in h0.numpy()])       # a unit that has been written (+-1; a 0 has no sign)
    h0[torch.arange(40), torch.as_tensor(unit)] *= -1                                # ... with ONE unit flipped per clip
    flip = A.run(sd, meta, case, tail, h0=h0)
    # the classifier sees relu(h) of every unit with a nonzero weight in every class row: flipping the unit at frame 3 changes frame 3's
    # own logits in every class, whatever the dynamics do with it afterwards
    wc, bc = sd["f_classification.0.weight"].to(torch.float64), sd["f_classification.0.bias"].to(torch.float64)
    l3 = h0.clamp(min=0).to(torch.float64) @ wc.t() + bc                             # frame 3's logits of the flipped state
    assert bool((l3 != base.logits.view(40, 12, -1)[:, 3]).all())                    # every class of every trial
    differ = (flip.h[0].view(40, 8, -1) != same.h[0].view(40, 8, -1)).sum(dim=2)     # units that differ, frames 4 .. 11
    print("differing units 8 steps after one flip: median", int(differ[:, -1].median()), "died out:", int((differ[:, -1] == 0).sum()), "of 40")
    assert int(differ[:, -1].median()) > 50


def test_gate_function_bounds_hold_for_the_fp32_emulation():
    x = A.gate_points()
    x64 = x.astype(np.float64)
    with np.errstate(over="ignore"):
        s64 = 1.0 / (1.0 + np.exp(-x64))
    s = A.sigmoid_f32(x)
    t = A.tanh_f32(x)
    assert not np.isnan(s).any() and not np.isnan(t).any()
    assert np.abs(s - s64).max() <= A.SIGMOID_ABS_BOUND
    assert np.abs(t - np.tanh(x64)).max() <= A.TANH_ABS_BOUND
    one_minus = (np.float32(1) - s).astype(np.float32)
    assert np.abs(one_minus - (1.0 - s64)).max() <= A.ONE_MINUS_SIGMOID_ABS_BOUND
    ts = A.tanh_f32(s)
    assert np.abs(ts - np.tanh(s64)).max() <= A.TANH_OF_SIGMOID_ABS_BOUND
    assert (s[x >= 18] == 1).all() and (s[x <= -89] == 0).all() and (t[x >= 9.5] == 1).all() and (t[x <= -9.5] == -1).all()
    print("fp32 emulation: sigmoid", np.abs(s - s64).max() / A.U, "tanh", np.abs(t - np.tanh(x64)).max() / A.U, "units of 2^-24")
