"""CPU tests of MiniROADA (model/rnn/rnn.py:73-136): registry name, state_dict keys / shapes and seeded initial weights against the
reference's (tests/golden/g12_mroada_init.json, written by scripts/gen_golden_anticipation.py)."""
import json
import os

import numpy as np
import pytest
import torch

from prego_amd import weights as W
from prego_amd.config import anticipation_cfg, assembly101_cfg

G = os.path.join(os.path.dirname(__file__), "golden")


def test_registry_resolves_miniroad_a():
    import prego_amd.model  # noqa: F401
    from prego_amd.registry import META_ARCHITECTURES
    from prego_amd.model import MROADA
    for name in ("MiniROAD", "MiniROADA"):
        assert name in META_ARCHITECTURES
    assert META_ARCHITECTURES["MiniROADA"] is MROADA


@pytest.mark.parametrize("actionness", [False, True])
def test_state_dict_keys_shapes_and_seeded_init_match_the_reference(actionness):
    import prego_amd.model  # noqa: F401
    from prego_amd.registry import build_model
    ref = json.load(open(os.path.join(G, "g12_mroada_init.json")))[str(actionness)]
    cfg = anticipation_cfg(assembly101_cfg(hidden_dim=512), 4, actionness=actionness)
    torch.manual_seed(0)
    m = build_model(cfg)                       # parameter containers only: no device, no engine
    sd = m.state_dict()
    assert list(sd.keys()) == ref["keys"]
    assert [list(v.shape) for v in sd.values()] == ref["shapes"]
    for k, v in sd.items():
        assert np.allclose(v.flatten()[:8].numpy(), ref["head"][k], rtol=0, atol=0), k
        assert abs(float(v.double().sum()) - ref["sum"][k]) <= 1e-9 * max(1.0, abs(ref["sum"][k])), k
    assert ("f_actionness.0.weight" in sd) == actionness


def test_seeded_state_dict_helper_has_the_model_keys():
    import prego_amd.model  # noqa: F401
    from prego_amd.registry import build_model
    for act in (False, True):
        cfg = anticipation_cfg(assembly101_cfg(hidden_dim=512), 3, actionness=act)
        sd = W.miniroad_a_state_dict(cfg, 20, head_gain=2.0, ant_gain=3.0)
        m = build_model(cfg)
        ms = m.state_dict()
        assert sorted(sd) == sorted(ms)
        for k, v in sd.items():
            assert tuple(v.shape) == tuple(ms[k].shape) and v.dtype == np.float32, k
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})


def test_training_forward_is_refused_with_a_message():
    import prego_amd.model  # noqa: F401
    from prego_amd._lib import PregoError
    from prego_amd.registry import build_model
    m = build_model(anticipation_cfg(assembly101_cfg(hidden_dim=512), 2))
    m.train()
    x = torch.zeros(1, 4, 2048)
    with pytest.raises(PregoError, match="training is not built"):
        m(x, x)


def _tree(tmp_path):
    from scripts.gen_golden_anticipation import make_tree
    return make_tree(str(tmp_path))


def test_all_four_registry_names_resolve():
    import prego_amd.data  # noqa: F401
    import prego_amd.evaluate  # noqa: F401
    import prego_amd.loss  # noqa: F401
    import prego_amd.model  # noqa: F401
    from prego_amd.registry import CRITERIONS, DATA_LAYERS, EVAL, META_ARCHITECTURES
    assert META_ARCHITECTURES["MiniROADA"].__name__ == "MROADA"
    assert CRITERIONS["ANTICIPATION"].__name__ == "OadAntLoss"
    assert EVAL["ANTICIPATION"].__name__ == "AntEvaluate"
    assert DATA_LAYERS["THUMOS_ANTICIPATION"] is DATA_LAYERS["TVSERIES_ANTICIPATION"]


def test_feeder_windows_and_ant_target_match_the_reference(tmp_path):
    from prego_amd.registry import DATA_LAYERS
    import prego_amd.data  # noqa: F401
    cfg = _tree(tmp_path)
    g = np.load(os.path.join(G, "g12_feeder_windows.npz"))
    np.random.seed(0)
    tr = DATA_LAYERS[cfg["data_name"]](cfg, "train")
    te = DATA_LAYERS[cfg["data_name"]](cfg, "test")
    vids = ["vid_a", "vid_b"]
    assert [vids.index(x[0]) for x in tr.inputs] == list(g["train_vid"])
    assert [x[1] for x in tr.inputs] == list(g["train_start"]) and [x[2] for x in tr.inputs] == list(g["train_end"])
    for i in range(len(tr)):
        rgb, flow, t, at = tr[i]
        assert len(tr[i]) == 4 and rgb.dtype == torch.float32 and t.shape == (8, 5) and at.shape == (3, 5)
        assert np.array_equal(at.numpy(), g["train_ant"][i])
        assert abs(float(rgb.double().sum()) - g["train_rgb_sum"][i]) < 1e-6 * max(1.0, g["train_rgb_sum"][i])
    assert [x[2] for x in te.inputs] == list(g["test_end"])
    for i in range(len(te)):
        rgb, flow, t, at = te[i]
        assert rgb.shape[0] == t.shape[0] == at.shape[0] == g["test_end"][i]
        assert np.array_equal(at.numpy(), g[f"test_ant_{i}"]) and np.array_equal(t.numpy(), g[f"test_target_{i}"])


class _Log:
    def info(self, *a, **k):
        pass


@pytest.mark.parametrize("metric", ["AP", "cAP"])
def test_ant_evaluate_with_a_cpu_stand_in_matches_the_reference(tmp_path, metric):
    import prego_amd.data  # noqa: F401
    import prego_amd.evaluate  # noqa: F401
    from prego_amd.registry import DATA_LAYERS, EVAL
    from scripts.gen_golden_anticipation import StandIn
    cfg = dict(_tree(tmp_path), metric=metric)
    ref = json.load(open(os.path.join(G, "g12_ant_eval.json")))[f"standin_{metric}"]
    loader = torch.utils.data.DataLoader(DATA_LAYERS[cfg["data_name"]](cfg, "test"), batch_size=1, shuffle=False)
    ev = EVAL["ANTICIPATION"](cfg)
    mean = ev(StandIn().eval(), loader, _Log(), "cpu")
    assert abs(mean - ref["mean"]) < 1e-9
    got = [ev.result[f"anticipation_{l + 1}"]["mean_AP"] for l in range(3)]
    assert np.allclose(got, ref["steps"], rtol=0, atol=1e-9)
    assert "mean_AP" in ev.result


def test_ant_evaluate_refuses_thumos_postprocessing(tmp_path):
    import prego_amd.evaluate  # noqa: F401
    from prego_amd.registry import EVAL
    cfg = dict(_tree(tmp_path), data_name="THUMOS_ANTICIPATION")
    with pytest.raises(NotImplementedError):
        EVAL["ANTICIPATION"](cfg)
