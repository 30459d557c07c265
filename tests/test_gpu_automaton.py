"""The recurrence, the split pass, the streaming step and the two heads against the saturated-gate automaton (tests/helpers/gru_automaton.py):
weights under which the model has ONE right answer in every compute dtype and every pass, so EVERY frame of EVERY clip is compared with
torch.equal - logits, argmax (exact ties for the maximum included: the first maximal class wins), h_last, the state after every streamed
frame.  One state not reset at a clip boundary, one stale element of the exchange buffer, one row of the (clip, frame) map off by one
changes a +-1 somewhere, and the classifier (every weight nonzero) shows it in that very frame.

Every run checks conditions() on its reference before it looks at a kernel's output.  The only comparisons that are not equalities are the
probabilities and the gate functions; their bounds are derived in the helper, and the largest deviation measured is printed."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd.engine import MiniRoadEngine                 # noqa: E402
from tests.helpers import gru_automaton as A                # noqa: E402

DEV = "cuda:0"
A_KEYS = ("anticipation_layer.0.weight", "anticipation_layer.0.bias")
_REF = {}
_BIG = [None, None]             # one large reference at a time (gigabytes of feature bits)


def _ref(rid):
    if A.RUNS[rid].get("big"):
        if _BIG[0] != rid:
            _BIG[:] = [None, None]
            _BIG[:] = [rid, A.reference(rid, DEV)]
        return _BIG[1]
    if rid not in _REF:
        _REF[rid] = A.reference(rid, DEV)
    return _REF[rid]


def _engine(case, sd, dtype, env=None):
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:                                                    # the library reads its switches when the handle is created
        e = MiniRoadEngine(case.d_rgb, case.d_flow, case.emb, case.hid, case.n_classes, DEV, dtype, num_layers=case.num_layers)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    e.set_weights({k: v.to(DEV) for k, v in sd.items()})
    if case.ant_len:
        e.set_anticipation(sd[A_KEYS[0]].to(DEV), sd[A_KEYS[1]].to(DEV), case.ant_len)
    return e


def _io(case, feats, dt=None):
    cv = (lambda t: t) if dt is None else (lambda t: t.to(dt))
    return [cv(r) for r, _ in feats] if case.d_rgb else None, [cv(f) for _, f in feats] if case.d_flow else None


def _same(got_list, want, what):
    """every row of every clip; on a mismatch name the first clip and frame"""
    got = torch.cat([g.reshape(g.shape[0], -1) for g in got_list]).to(want.dtype)
    want = want.reshape(want.shape[0], -1)
    if torch.equal(got, want):
        return
    bad = (got != want).any(dim=1).nonzero()[:, 0]
    raise AssertionError(f"{what}: {len(bad)} of {len(want)} frames differ, first at packed frame {int(bad[0])}: got {got[bad[0]].tolist()[:8]} "
                         f"want {want[bad[0]].tolist()[:8]}")


def _forward_equals(e, case, feats, res, what, dt=None, h_last=False):
    rgb, flow = _io(case, feats, dt)
    o, a, _ = e.forward_ragged(rgb, flow, softmax=False, want_out=True, want_argmax=True)
    e.check()
    _same(o, res.logits, f"{what}: logits")
    _same(a, res.argmax, f"{what}: argmax")
    if h_last:
        _, a, hl = e.forward_ragged(rgb, flow, softmax=True, want_out=False, want_argmax=True, want_h_last=True)
        e.check()
        _same(a, res.argmax, f"{what}: argmax (with h_last)")
        assert torch.equal(hl, res.h_last.to(DEV)), f"{what}: h_last"


DTYPES_OF = {"h1024": ["fp16", "bf16", "fp32", "fp16x2"], "h512": ["fp16", "bf16", "fp32"], "h2048": ["fp16", "bf16"],
             "l2": ["fp16", "bf16", "fp32"]}
SIZE_RUNS = [(rid, dt) for rid in A.RUNS if rid.split("-")[0] in DTYPES_OF for dt in DTYPES_OF[rid.split("-")[0]]]


@pytest.mark.parametrize("rid,dtype", SIZE_RUNS, ids=[f"{r}-{d}" for r, d in SIZE_RUNS])
def test_every_dtype_and_hidden_size(rid, dtype):
    """40 ragged clips of 3..40 frames and one of 300, with and without a flow half, one and two GRU layers"""
    case, sd, _, feats, _, res = _ref(rid)
    e = _engine(case, sd, dtype)
    _forward_equals(e, case, feats, res, f"{rid} {dtype}", h_last=True)


@pytest.mark.parametrize("n", [40, 200, 400, 700])
def test_clip_counts_and_chunk_sizes(n):
    """tile counts 1 / 2 / 4, continuous batching (more clips than slots: slots run clips back to back) and restarts of the recurrence on
    launch boundaries: rows_per_chunk = n_clips (the smallest the library takes, rounded up to its 128-row quantum: one to three steps per launch, the
    per-chunk head), 1000 (many launches) and the default.  The library takes the chunk size from the SIZE of the workspace it is handed and the engine only ever
    grows its workspace, so every setting starts from no workspace, and the sizes are asserted to differ: the setting took."""
    case, sd, _, feats, _, res = _ref(f"clips{n}")
    n_clips = len(res.lens)
    for dtype in ("fp16", "bf16", "fp32"):
        e = _engine(case, sd, dtype)
        sizes = []
        for rpc in (n_clips, 1000, e.rows_per_chunk):
            e.rows_per_chunk = rpc
            e._ws = None
            _forward_equals(e, case, feats, res, f"{n} clips {dtype} rows_per_chunk {rpc}")
            sizes.append(e._ws.numel())
        assert (sizes[0] < sizes[1] if n_clips < 1000 else True) and sizes[1] <= sizes[2], (dtype, sizes)
        if sum(res.lens) > 1024:
            assert sizes[1] < sizes[2], (dtype, sizes)


@pytest.mark.parametrize("rid,dtype", [("chain", "fp16"), ("chain", "bf16"), ("chain", "fp32"), ("chain", "fp16x2"), ("chain-l2", "fp16"),
                                       ("chain-l2", "fp32")])
def test_h0_h_last_chaining(rid, dtype):
    """a hostile h0 of {-1, 0, 1}; two halves chained through h_last equal one call and equal the automaton"""
    case, sd, _, feats, h0, res = _ref(rid)
    e = _engine(case, sd, dtype)
    rgb, _ = _io(case, feats)
    h0 = h0.to(DEV)
    o, a, hl = e.forward_ragged(rgb, None, softmax=False, want_argmax=True, h0=h0, want_h_last=True)
    e.check()
    _same(o, res.logits, "one call: logits")
    _same(a, res.argmax, "one call: argmax")
    assert torch.equal(hl, res.h_last.to(DEV))
    cut = [T // 2 for T in res.lens]
    o1, a1, h1 = e.forward_ragged([r[:c] for r, c in zip(rgb, cut)], None, softmax=False, want_argmax=True, h0=h0, want_h_last=True)
    o2, a2, h2 = e.forward_ragged([r[c:] for r, c in zip(rgb, cut)], None, softmax=False, want_argmax=True, h0=h1, want_h_last=True)
    e.check()
    mid = torch.stack([res.clip(res.h[l], i)[c - 1] for l in range(case.num_layers) for i, c in enumerate(cut)]).to(torch.float32)
    assert torch.equal(h1.reshape(-1, case.hid), mid), "h_last of the first half"
    _same([torch.cat(p) for p in zip(o1, o2)], res.logits, "two halves: logits")
    _same([torch.cat(p) for p in zip(a1, a2)], res.argmax, "two halves: argmax")
    assert torch.equal(h2, res.h_last.to(DEV))


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_one_long_clip(dtype):
    """31 114 frames (the longest Epic-tent video): one flipped unit in 31 114 x 1 024 fails it"""
    case, sd, _, feats, _, res = _ref("long31114")
    e = _engine(case, sd, dtype)
    _forward_equals(e, case, feats, res, f"31114 frames {dtype}")


def _split_run(rid, dtype, in16=False):
    case, sd, _, feats, _, res = _ref(rid)
    assert sum(res.lens) >= 262144 and sum(res.lens) % 256 != 0
    dt = None if not in16 else {"fp16": torch.float16, "bf16": torch.bfloat16}[dtype]
    e3 = _engine(case, sd, dtype, {"PREGO_SPLIT_PASS": "3"})
    _forward_equals(e3, case, feats, res, f"{rid} {dtype}: first call", dt)
    assert e3.pass_info()["mode"] == 0, "a handle's first call is chunked"
    for k in range(2):
        _forward_equals(e3, case, feats, res, f"{rid} {dtype}: split pass {k}", dt)
        info = e3.pass_info()
        assert info["mode"] == 3 and info["slots"] == 48, info
    del e3
    e0 = _engine(case, sd, dtype, {"PREGO_SPLIT_PASS": "0"})
    _forward_equals(e0, case, feats, res, f"{rid} {dtype}: chunked handle", dt)
    assert e0.pass_info()["mode"] == 0


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_split_pass_64_ragged_clips(dtype):
    _split_run("split64", dtype)


def test_split_pass_50_clips_on_48_slots_16bit_features_with_flow():
    _split_run("split50-flow", "fp16", in16=True)


def test_split_pass_other_feature_and_embedding_size():
    _split_run("split52-e1024", "bf16")


@pytest.mark.parametrize("switch", ["PREGO_GRU_NO_LOCAL", "PREGO_GRU_NO_MT"])
def test_ab_switches_of_the_product_library(switch):
    runs = [("h1024-rgb", ["fp16", "bf16", "fp32"]), ("clips400", ["fp16"])]
    if switch == "PREGO_GRU_NO_LOCAL":      # the fp16x2 kernel's unpaired hand-off, and the 16-workgroup rendezvous of hidden size 512, off the verified placement
        runs += [("h1024-rgb", ["fp16x2"]), ("h512-rgb", ["bf16"])]
    for rid, dtypes in runs:
        case, sd, _, feats, _, res = _ref(rid)
        for dtype in dtypes:
            _forward_equals(_engine(case, sd, dtype, {switch: "1"}), case, feats, res, f"{switch} {rid} {dtype}")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 16])
def test_streaming_step(n, dtype):
    """n streams, 50 frames: logits, argmax and the state after EVERY frame"""
    case, sd, _, feats, _, res = _ref("stream16")
    e = _engine(case, sd, dtype)
    h = torch.zeros((n, case.hid), device=DEV)
    x = torch.stack([feats[i][0] for i in range(n)])                     # [n, 50, d_rgb]
    want_l, want_a, want_h = (t.view(16, 50, -1)[:n] for t in (res.logits, res.argmax, res.h[0]))
    for t in range(50):
        lg, am = e.step(x[:, t].contiguous(), None, h, softmax=False)
        assert torch.equal(lg.to(torch.float64), want_l[:, t]), f"frame {t}: logits"
        assert torch.equal(am, want_a[:, t, 0]), f"frame {t}: argmax"
        assert torch.equal(h, want_h[:, t].to(torch.float32)), f"frame {t}: state"
    e.check()


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("L", [1, 4, 8])
def test_miniroada_anticipation_head(L, dtype):
    case, sd, _, feats, _, res = _ref(f"ant{L}")
    e = _engine(case, sd, dtype)
    rgb, _ = _io(case, feats)
    o, a, _, ao, aa = e.forward_ragged(rgb, None, softmax=False, want_argmax=True, want_ant=True)
    e.check()
    _same(o, res.logits, "logits")
    _same(a, res.argmax, "argmax")
    _same(ao, res.ant_logits, "anticipation logits")
    _same(aa, res.ant_argmax, "anticipation argmax")
    assert int(((res.ant_logits == res.ant_logits.max(dim=-1, keepdim=True).values).sum(dim=-1) > 1).sum()) > 0, "no tie in the reference"


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_training_forward_and_head_gradients(dtype):
    """PREGO_FWD_KEEP, dropout 0, B 16 x T 128 with balanced feature rows (p = 1/2): exact logits; after a backward with dyadic dlogits
    exact f_classification gradients; every trunk gradient at most sigmoid(-64) * F (saturated gates pass no gradient;
    helpers/gru_automaton.py::trunk_grad_factor)"""
    case, sd, _, feats, _, res = _ref("train")
    e = _engine(case, sd, dtype)
    e.set_dropout(0.0, 0)
    B, T, C = 16, 128, case.n_classes
    rgb = torch.stack([r for r, _ in feats])
    logits = e.forward_train(rgb, None)
    e.check()
    assert torch.equal(logits.to(torch.float64), res.logits.view(B, T, C))
    g = torch.Generator().manual_seed(5)
    dl = (torch.randint(-16, 17, (B, T, C), generator=g).to(torch.float64) / 16).to(DEV)
    grads = e.backward(dl.to(torch.float32))
    e.check()
    hr = res.h[0].clamp(min=0).to(torch.float64)
    assert torch.equal(grads["f_classification.0.weight"].to(torch.float64), dl.view(-1, C).t() @ hr)
    assert torch.equal(grads["f_classification.0.bias"].to(torch.float64), dl.view(-1, C).sum(dim=0))
    F = A.trunk_grad_factor(sd, case, dl, B * T)
    cap = A.sigmoid64(-64.0) * F
    assert F < 1e13
    worst = {k: float(v.abs().max()) for k, v in grads.items() if not k.startswith("f_classification")}
    print(f"trunk gradients {dtype}: F = {F:.3g}, cap = {cap:.3g}, largest = {max(worst.values()):.3g}")
    assert len(worst) == 8
    for k, v in worst.items():
        assert v <= cap, (k, v, cap)                        # NaN fails too


def _probs_within_bound(got_list, logits64, what):
    got = torch.cat([g.reshape(-1, g.shape[-1]) for g in got_list]).to(torch.float64)
    p, bound = A.softmax_bound(logits64.reshape(-1, logits64.shape[-1]))
    assert float(p.min()) > 2.0 ** -126, "a subnormal probability"
    ratio = float(((got - p).abs() / bound).max())
    print(f"{what}: largest |p - p64| = {float((got - p).abs().max()):.3g}, {ratio:.3f} of its bound")
    assert ratio <= 1.0, what                               # NaN fails too


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32", "fp16x2"])
def test_probabilities(dtype):
    """softmax of exact logits (multiples of 1/32, spread <= 60) against fp64, bound derived in helpers/gru_automaton.py::softmax_bound"""
    case, sd, _, feats, _, res = _ref("prob")
    e = _engine(case, sd, dtype)
    rgb, _ = _io(case, feats)
    o, a, _ = e.forward_ragged(rgb, None, softmax=True, want_argmax=True)
    e.check()
    _same(a, res.argmax, "argmax")
    _probs_within_bound(o, res.logits, f"probabilities {dtype}")


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
def test_anticipation_probabilities(dtype):
    case, sd, _, feats, _, res = _ref("prob-ant4")
    e = _engine(case, sd, dtype)
    rgb, _ = _io(case, feats)
    o, a, _, ao, aa = e.forward_ragged(rgb, None, softmax=True, want_argmax=True, want_ant=True)
    e.check()
    _same(a, res.argmax, "argmax")
    _same(aa, res.ant_argmax, "anticipation argmax")
    _probs_within_bound(o, res.logits, f"probabilities {dtype}")
    _probs_within_bound(ao, res.ant_logits, f"anticipation probabilities {dtype}")


# ---- the gate functions themselves (csrc/common.h: sigmoidf_, tanhf_), through the public ABI ----------------------------------------
def _gate_sweep(which):
    """W_ih = 0, T = 1, h0 = 0: h_1 is a function of the biases alone (fp32 handle, h_last); 1 024 arguments per set of weights"""
    case = A.Case(d_rgb=512, d_flow=0, emb=512, hid=1024, seed=77)
    sd, meta = A.build_state_dict(case)
    H = case.hid
    sd["gru.weight_ih_l0"] = torch.zeros_like(sd["gru.weight_ih_l0"])
    rgb = [A.build_features(case, [1], 1, DEV)[0][0]]
    e = MiniRoadEngine(case.d_rgb, 0, case.emb, H, case.n_classes, DEV, "fp32")
    pts = A.gate_points()
    pts = np.concatenate([pts, np.zeros(-len(pts) % H, np.float32)])
    out = []
    for s in range(0, len(pts), H):
        x = torch.from_numpy(pts[s:s + H])
        b_ih, b_hh = torch.zeros(3 * H), torch.zeros(3 * H)
        if which == "tanh":                    # z = sigmoidf_(-128) = 0 exactly, b_hn = 0: h_1 = tanhf_(b_n)
            b_ih[H:2 * H], b_ih[2 * H:] = -128.0, x
        elif which == "sigmoid":               # n = tanhf_(64) = 1 exactly: h_1 = 1 - sigmoidf_(b_z)
            b_ih[H:2 * H], b_ih[2 * H:] = x, 64.0
        else:                                  # b_hn = 1, b_in = 0, z = 0: h_1 = tanhf_(sigmoidf_(b_r))
            b_ih[:H], b_ih[H:2 * H], b_hh[2 * H:] = x, -128.0, 1.0
        sd["gru.bias_ih_l0"], sd["gru.bias_hh_l0"] = b_ih, b_hh
        e.set_weights({k: v.to(DEV) for k, v in sd.items()})
        _, _, hl = e.forward_ragged(rgb, None, want_out=False, want_h_last=True)
        e.check()
        out.append(hl[0].cpu().numpy())
    return pts, np.concatenate(out)


def _s64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x.astype(np.float64)))


def test_tanh_of_the_recurrence():
    x, h = _gate_sweep("tanh")
    assert not np.isnan(h).any()
    err = np.abs(h - np.tanh(x.astype(np.float64))).max()
    print(f"tanhf_: largest error {err / A.U:.3f} * 2^-24 (bound {A.TANH_ABS_BOUND / A.U})")
    assert err <= A.TANH_ABS_BOUND
    assert (h[x >= 9.5] == 1).all() and (h[x <= -9.5] == -1).all()


def test_sigmoid_of_the_recurrence():
    x, h = _gate_sweep("sigmoid")
    assert not np.isnan(h).any()
    err = np.abs(h - (1.0 - _s64(x))).max()
    print(f"1 - sigmoidf_: largest error {err / A.U:.3f} * 2^-24 (bound {A.ONE_MINUS_SIGMOID_ABS_BOUND / A.U})")
    assert err <= A.ONE_MINUS_SIGMOID_ABS_BOUND
    assert (h[x >= 18] == 0).all() and (h[x <= -89] == 1).all()


def test_tanh_of_sigmoid_of_the_recurrence():
    x, h = _gate_sweep("composite")
    assert not np.isnan(h).any()
    err = np.abs(h - np.tanh(_s64(x))).max()
    print(f"tanhf_(sigmoidf_): largest error {err / A.U:.3f} * 2^-24 (bound {A.TANH_OF_SIGMOID_ABS_BOUND / A.U})")
    assert err <= A.TANH_OF_SIGMOID_ABS_BOUND
