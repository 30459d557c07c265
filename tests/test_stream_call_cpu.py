"""prego_amd/_stream_call.py without a device: its check function against the "... on cpu" texts of tests/golden/stream_refusals.json (recorded
from the nine entries before they shared it) for three entries of different wording - `step`, `StreamPool.push_frames` and
`TransformerStreamPool.push_bursts` -, the counts policies one by one, and the small steps around them."""
import json
import os

import pytest

torch = pytest.importorskip("torch")

from prego_amd import _stream_call as SC                      # noqa: E402
from prego_amd._lib import PregoError                         # noqa: E402
from prego_amd.config import FEATURE_SIZES, assembly101_cfg   # noqa: E402
from tests.helpers import stream_refusal_cases as R           # noqa: E402

GOLDEN = {cid: (kind, msg) for cid, kind, msg in json.load(open(os.path.join(os.path.dirname(__file__), "golden", "stream_refusals.json")))}
N, K, L = R.N, R.K, R.ANT_LEN
DEFAULT = "{what} as contiguous {dt} cuda {shape}"
_VIT = assembly101_cfg()
VIT_DIMS = (FEATURE_SIZES[_VIT["rgb_type"]], FEATURE_SIZES[_VIT["flow_type"]], _VIT["num_classes"])


def _dims(kind):
    return R.KINDS[kind][0], R.KINDS[kind][1], R.NCLS


# (case id, who, row shape, (d_rgb, d_flow, n_classes), anticipation_length, tensor name, the entry's wording)
WORDINGS = (
    [(f"step/{'flow' if name == 'flow' else 'ant'}/{name}-device", "step", (N,), _dims("flow" if name == "flow" else "ant"), L, name, fmt)
     for name, fmt in (("rgb", "contiguous fp32 cuda {shape}"), ("flow", "contiguous fp32 cuda {shape}"),
                       ("h", "the GRU state as contiguous fp32 cuda {shape}"), ("ant_out", "a contiguous {dt} cuda {shape} anticipation buffer"),
                       ("ant_argmax", "a contiguous {dt} cuda {shape} anticipation buffer"))]
    + [(f"push_frames/{'flow' if name == 'flow' else 'ant'}/{name}-device", "stream pool push_frames", (N, K),
        _dims("flow" if name == "flow" else "ant"), L, name, DEFAULT) for name in ("rgb", "flow", "out", "argmax", "ant_out", "ant_argmax")]
    + [(f"vit_push_bursts/flow/{name}-device", "transformer stream pool push_bursts", (N * K,), VIT_DIMS, 0, name,
        DEFAULT + f" (sum(counts) = {N * K} packed rows)") for name in ("rgb", "flow", "out", "argmax")])


@pytest.mark.parametrize("cid,who,rows,dims,ant_len,name,fmt", WORDINGS, ids=[w[0] for w in WORDINGS])
def test_check_words_a_cpu_tensor_as_the_entry_did(cid, who, rows, dims, ant_len, name, fmt):
    d_rgb, d_flow, ncls = dims
    kind, want = GOLDEN[cid]
    assert kind == "PregoError" and want.endswith(" on cpu")
    if name in ("rgb", "flow"):
        t = torch.zeros(rows + (d_rgb if name == "rgb" else d_flow,))
        specs = SC.in_specs(rows, d_rgb, d_flow, t if name == "rgb" else None, t if name == "flow" else None)
    elif name == "h":
        specs = [(torch.zeros((N, R.HID)), (N, R.HID), SC.F32, "GRU state" if who != "step" else None)]
    else:
        outs, specs = SC.outputs("cpu", rows, ncls, ant_len, None, None, None, None)
        assert len(outs) == (4 if ant_len else 2) and all(o is s[0] for o, s in zip(outs, specs))
        specs = [s for s in specs if s[3] == {"out": "out", "argmax": "argmax", "ant_out": "anticipation out", "ant_argmax": "anticipation argmax"}[name]]
    assert len([s for s in specs if s[0] is not None]) == 1
    with pytest.raises(PregoError) as e:
        SC.check(who, specs, fmt)
    assert str(e.value) == want


def test_outputs_keeps_the_callers_buffers_and_allocates_the_rest():
    mine = torch.empty((N, K), dtype=torch.int32)
    outs, specs = SC.outputs("cpu", (N, K), 12, L, None, mine, None, None)
    assert outs[1] is mine and [tuple(o.shape) for o in outs] == [(N, K, 12), (N, K), (N, K, L, 12), (N, K, L)]
    assert [o.dtype for o in outs] == [torch.float32, torch.int32, torch.float32, torch.int32]
    assert [s[1:] for s in specs] == [((N, K, 12), SC.F32, "out"), ((N, K), SC.I32, "argmax"), ((N, K, L, 12), SC.F32, "anticipation out"),
                                      ((N, K, L), SC.I32, "anticipation argmax")]
    theirs = torch.empty(3)
    outs, specs = SC.outputs("cpu", (N,), 12, 0, None, None, theirs, theirs)      # no head: the anticipation buffers are not looked at
    assert len(outs) == 2 and len(specs) == 2


# ---- the counts policies, one by one -------------------------------------------------------------------------------------------------
def test_counts_a_sequence_or_a_cpu_tensor_becomes_ints():
    assert SC.counts_list("w", (2, 3)) == [2, 3]
    assert SC.counts_list("w", torch.tensor([2, 3])) == [2, 3]
    assert SC.counts_list("w", [2.0, True], 2) == [2, 1]


def test_counts_length_is_checked_where_the_entry_knows_it():
    for cid, who in (("push_ragged/ant/counts-length", "stream pool push_ragged"), ("vit_push_bursts/flow/counts-length", "transformer stream pool push_bursts")):
        with pytest.raises(PregoError) as e:
            SC.counts_list(who, [K, K, K], N)
        assert ("PregoError", str(e.value)) == GOLDEN[cid]
    assert SC.counts_list("step_ragged", [K, K, K]) == [K, K, K]                 # step_ragged: n is the length of counts


def test_counts_tensor_policy_refuse_cuda():
    """step_ragged refuses a tensor that is CUDA, floating point or not 1-d (the golden text is the CUDA one: same sentence); the pools'
    entries take what .tolist() gives"""
    want = GOLDEN["step_ragged/ant/counts-cuda"][1]
    for bad in (torch.tensor([2.0, 2.0]), torch.tensor([[2, 2]])):
        with pytest.raises(PregoError) as e:
            SC.counts_list("step_ragged", bad, refuse_cuda=True)
        assert str(e.value) == want.split(", got ")[0] + f", got {tuple(bad.shape)} {bad.dtype} on cpu"
    assert SC.counts_list("stream pool push_ragged", torch.tensor([2.0, 2.0]), 2) == [2, 2]
    assert GOLDEN["push_ragged/ant/counts-cuda"][0] == "ok" and GOLDEN["vit_push_bursts/flow/counts-cuda"][0] == "ok"


def test_counts_one_int_policy():
    """push_bursts takes one number for every slot; the others let the TypeError out, as recorded"""
    assert SC.counts_list("w", 3, 2, one_int=True) == [3, 3]
    assert SC.counts_list("w", torch.tensor(3), 2, one_int=True) == [3, 3]
    for cid in ("step_ragged/ant/counts-one-int", "push_ragged/ant/counts-one-int"):
        with pytest.raises(TypeError) as e:
            SC.counts_list("w", K, N)
        assert ("TypeError", str(e.value)) == GOLDEN[cid]
    assert GOLDEN["vit_push_bursts/flow/counts-one-int"][0] == "ok"


def test_counts_int32_clamp_is_step_raggeds_alone():
    assert SC.clamp_i32([2 ** 40, -(2 ** 40), 5]) == [2 ** 31 - 1, -(2 ** 31), 5]
    assert SC.counts_list("w", [2 ** 40]) == [2 ** 40]                           # not clamped on the way in: R is the caller's sum


# ---- the small steps ---------------------------------------------------------------------------------------------------------------------
def test_resolve_ant_frame_source_and_refuse_general_word_the_recorded_refusals():
    assert SC.resolve_ant("w", None, 0) is False and SC.resolve_ant("w", None, 4) is True and SC.resolve_ant("w", False, 4) is False
    for cid, who in (("step/flow/want-ant-no-head", "step"), ("push/flow/want-ant-no-head", "stream pool push")):
        with pytest.raises(PregoError) as e:
            SC.resolve_ant(who, True, 0)
        assert str(e.value) == GOLDEN[cid][1]
    x = torch.zeros(1)
    assert SC.frame_source("w", 8, x, None) is x and SC.frame_source("w", 0, None, x) is x
    for cid, who, d_rgb, frames in (("step/ant/rgb-none", "step", 2048, "frame"), ("step_frames/no_rgb/flow-none", "step_frames", 0, "frames"),
                                    ("push/no_rgb/flow-none", "stream pool push", 0, "frame"),
                                    ("vit_push_bursts/no_rgb/flow-none", "transformer stream pool push_bursts", 0, "frames")):
        with pytest.raises(PregoError) as e:
            SC.frame_source(who, d_rgb, None, None, frames)
        assert str(e.value) == GOLDEN[cid][1]
    SC.refuse_general("w", "bf16", 1024, 1, "-")
    for cid, who, advice in (("step_frames/fp32/not-built-for", "step_frames", "use forward() with h0 / h_last"),
                             ("push/fp32/not-built-for", "stream pool push", "run the general forward and feed its ids to vote()")):
        with pytest.raises(PregoError) as e:
            SC.refuse_general(who, "fp32", 1024, 1, advice)
        assert str(e.value) == GOLDEN[cid][1]
    for args in (("fp16x2", 1024, 1), ("bf16", 512, 1), ("fp16", 1024, 2)):
        with pytest.raises(PregoError, match="the streaming kernels are built for"):
            SC.refuse_general("w", *args, "-")


def test_workspace_grows_and_a_zero_size_still_reaches_the_call():
    ws = SC.Workspace()
    assert ws.fit(0, "cpu", none_if_zero=True) is None and ws.t is None          # the engine's entries: no workspace, the C call refuses
    assert ws.fit(0, "cpu").numel() == 0                                         # the pools': the tensor they hold
    a = ws.fit(512, "cpu")
    assert a.numel() == 512 and a.dtype == torch.uint8 and ws.fit(100, "cpu") is a and ws.fit(0, "cpu") is a
    assert ws.fit(513, "cpu").numel() == 513
    assert SC.ptr(None) is None and SC.ptr(a).value == a.data_ptr()
