"""GPU: a clip's result does not depend on how Evaluate packs a call.  One seeded set of 18 ragged videos runs through every way the
evaluator can launch it - link-fed, copy-then-forward, the by-length two-part split (it needs 16 unpinned videos), and several batches
per pass, where the host half of batch k - 1 (the ids' wait, the cut of the device-made JSON text) runs behind the launch of batch k.
Output file, mAP and every video's device argmax must be the same bits in all of them."""
import json
import logging
import os
from collections import namedtuple

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import weights as W                        # noqa: E402
from prego_amd.config import epic_tent_cfg                # noqa: E402

LENS = [1, 37, 400, 123, 64, 257, 123, 310, 5, 199, 88, 350, 17, 275, 150, 33, 222, 391]      # 18 videos, 3045 frames, two of 123
D, NCLS = 2048, 12
BUDGET = 640                # eval_frames_per_batch: batches of 6, 5, 3 and 4 videos, the last one closed by the last video
METRICS = dict(eval_perstage=True, eval_segmental=True, eval_segmental_window=16)
CONFIGS = {                 # name -> (pinned features, cfg)
    "a": (True, {}),
    "b": (True, dict(eval_link_fed=False)),
    "c": (False, {}),
    "d": (False, dict(eval_split_by_length=False)),
    "e": (False, dict(eval_split_fraction=0.5)),
    "f": (True, dict(eval_frames_per_batch=BUDGET)),
    "g": (False, dict(eval_frames_per_batch=BUDGET)),
    "h": (True, dict(eval_frames_per_batch=BUDGET, **METRICS)),
    "h1": (True, dict(METRICS)),                          # the one-batch run (h) is compared with
}
Run = namedtuple("Run", "mAP text argmax forwards phases perstage segmental")


def _batches(lens, budget):
    """the batches of the pass loop: a batch is launched by the video that fills the frame budget; what is left goes behind the loop"""
    out, cur, frames = [], [], 0
    for i, T in enumerate(lens):
        cur.append(i)
        frames += T
        if frames >= budget:
            out.append(cur)
            cur, frames = [], 0
    return out, cur


def _items(pinned, two_positives_in=None):
    pin = (lambda t: t.pin_memory()) if pinned else (lambda t: t)
    items = []
    for i, T in enumerate(LENS):
        rgb = torch.from_numpy(W.tsn_features((T, D), 31, f"eb.rgb.{i}"))[None]
        tgt = torch.zeros(1, T, NCLS)
        tgt[0, torch.arange(T), (torch.arange(T) // 29 + i) % NCLS] = 1
        if i == two_positives_in:
            tgt[0, T // 2, :2] = 1
        items.append((pin(rgb), torch.zeros(1, 1, D).expand(1, T, D), pin(tgt), (f"v{i}",), torch.tensor([0]), torch.tensor([T])))
    assert all(it[0].is_pinned() == pinned and it[0].dtype == torch.float32 for it in items)
    return items


def _evaluator(tmp, name, **extra):
    from prego_amd.registry import build_eval
    import prego_amd.evaluate  # noqa: F401
    vl = os.path.join(tmp, "video_list.json")
    if not os.path.exists(vl):
        json.dump({"EPIC-TENT-O": {"class_index": [f"c{i}" for i in range(NCLS)]}}, open(vl, "w"))
    cfg = epic_tent_cfg(eval="dummy.pth", video_list_path=vl, compute_dtype="fp16", eval_output_dir=os.path.join(tmp, name), **extra)
    return build_eval(cfg), os.path.join(tmp, name, "output_miniROAD.json")


@pytest.fixture(scope="module")
def model():
    from prego_amd.registry import build_model
    import prego_amd.model  # noqa: F401
    cfg = epic_tent_cfg(compute_dtype="fp16")
    m = build_model(cfg, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_state_dict(cfg, 20, head_gain=8.0).items()})
    return m


@pytest.fixture(scope="module")
def runs(model, tmp_path_factory):
    """every configuration once, on the same model"""
    tmp = str(tmp_path_factory.mktemp("batching"))
    sets = {True: _items(True), False: _items(False)}
    res = {}
    for name, (pinned, extra) in CONFIGS.items():
        ev, out = _evaluator(tmp, name, **extra)
        forwards = []
        orig = model.forward_clips
        model.forward_clips = lambda *a, _o=orig, **k: (forwards.append(len(a[0])), _o(*a, **k))[1]
        try:
            mAP = float(ev(model, sets[pinned], logging.getLogger("t"), "cuda:0"))
        finally:
            del model.forward_clips
        res[name] = Run(mAP, open(out, "rb").read(), dict(ev.last_device_argmax), forwards, [p for p, _ in ev.phase_log], ev.last_perstage,
                        ev.last_segmental)
    return res


def test_the_budget_makes_four_batches_and_the_last_video_closes_the_last():
    done, left = _batches(LENS, BUDGET)
    assert [len(b) for b in done] == [6, 5, 3, 4] and left == []


@pytest.mark.parametrize("name", [n for n in CONFIGS if n != "a"])
def test_results_do_not_depend_on_the_packing(runs, name):
    ref, got = runs["a"], runs[name]
    assert json.loads(got.text) == json.loads(ref.text)
    assert got.mAP == ref.mAP
    assert list(got.argmax) == list(ref.argmax) == [f"v{i}" for i in range(len(LENS))]
    for vid, a in ref.argmax.items():
        assert torch.equal(got.argmax[vid], a), vid
    js = json.loads(got.text)
    assert [len(js[f"v{i}"]["pred"]) for i in range(len(LENS))] == LENS == [len(js[f"v{i}"]["gt"]) for i in range(len(LENS))]


def test_the_by_length_split_runs_exactly_when_it_should(runs):
    assert runs["a"].forwards == [18] and runs["d"].forwards == [18]
    # fp32 features: half of the frames at most in the first part, the longest videos first - 400 + 391 + 350 + 310 of 3045
    assert runs["c"].forwards == [4, 14] and runs["e"].forwards == [4, 14]
    assert runs["b"].forwards == [4, 14]                  # pinned features that are not link-fed are copied then forwarded, split as any


@pytest.mark.parametrize("name", ["f", "g", "h"])
def test_every_batch_is_launched_once_and_collected_one_batch_behind(runs, name):
    done, left = _batches(LENS, BUDGET)
    r = runs[name]
    assert r.forwards == [len(b) for b in done] and len(done) >= 4 and not left
    assert r.phases.count("launch") == len(done) + 1
    assert r.phases[:3 * len(done)] == ["loader", "launch", "collect"] * len(done)
    assert r.phases[3 * len(done):3 * len(done) + 6] == ["loader", "launch", "collect", "collect_last", "check", "json_written"]


def test_the_metrics_of_a_pass_do_not_depend_on_its_batches(runs):
    h, one = runs["h"], runs["h1"]
    assert h.perstage is not None and h.segmental is not None and one.forwards == [18]
    assert repr(h.perstage) == repr(one.perstage)         # floats print round-trip exact; a stage without positives is nan in both
    assert h.segmental == one.segmental
    assert runs["a"].perstage is None and runs["a"].segmental is None


def test_perstage_refuses_a_video_that_is_not_one_hot(model, tmp_path):
    from prego_amd._lib import PregoError
    ev, _ = _evaluator(str(tmp_path), "o", eval_perstage=True)
    with pytest.raises(PregoError, match="eval_perstage"):
        ev(model, _items(True, two_positives_in=7), logging.getLogger("t"), "cuda:0")
    model.check()
