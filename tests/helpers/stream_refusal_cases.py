"""Wrong calls of the nine streaming entries - MiniRoadEngine.step / step_wide / step_frames / step_ragged, StreamPool.push / push_frames /
push_ragged, TransformerStreamPool.push / push_bursts - and what each answers.  `record()` runs the table and returns (case id, exception
type, message) per case ('ok' where the call is accepted); scripts/gen_stream_refusals.py wrote tests/golden/stream_refusals.json with it
at the commit before the entries were put on prego_amd/_stream_call.py, and tests/test_gpu_stream_refusals.py holds every later tree to
that file.  The smallest legal call: 2 streams or slots, K = 2, pools of capacity 4, vote window 3, max_events 8; the MiniROAD dimensions
are the automaton's (tests/helpers/step_wide_cases.py).  No case's text holds a pointer or an allocator's byte count.
`step` does not check `out` / `argmax`, so no case hands it a wrong one: the kernel would be given the pointer."""
import torch

from tests.helpers import gru_automaton as A

CAPACITY, VOTE_WINDOW, MAX_EVENTS = 4, 3, 8
N, K, ANT_LEN, NCLS, HID, EMB = 2, 2, 4, 12, 1024, 2048
VIT_WINDOW = 32
OPEN, CLOSED = (0, 1, 2), 3
# entry: (owner, method, row shape of a legal call: one row per stream, [n, K], or packed rows)
ENTRIES = {
    "step": ("engine", "step", "one"), "step_wide": ("engine", "step_wide", "one"), "step_frames": ("engine", "step_frames", "frames"),
    "step_ragged": ("engine", "step_ragged", "packed"), "push": ("pool", "push", "one"), "push_frames": ("pool", "push_frames", "frames"),
    "push_ragged": ("pool", "push_ragged", "packed"), "vit_push": ("vit_pool", "push", "one"),
    "vit_push_bursts": ("vit_pool", "push_bursts", "packed"),
}
ENGINE, POOL, VIT = ("step", "step_wide", "step_frames", "step_ragged"), ("push", "push_frames", "push_ragged"), ("vit_push", "vit_push_bursts")
# model kind: (d_rgb, d_flow, operand type, anticipation head)
KINDS = {"ant": (A.RGB["d_rgb"], A.RGB["d_flow"], "bf16", True), "flow": (A.FLOW["d_rgb"], A.FLOW["d_flow"], "fp16", False),
         "no_rgb": (0, 2048, "bf16", False), "fp32": (A.RGB["d_rgb"], A.RGB["d_flow"], "fp32", False)}


class Ctx:
    """the engines, models and pools of the table, each built once: zero MiniROAD weights (no case looks at a value), slots 0..2 open"""

    def __init__(self, dev="cuda:0"):
        self.dev = torch.device(dev)
        self._made = {}

    def _once(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    def zeros(self, shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=self.dev)

    def engine(self, kind):
        def make():
            from prego_amd.engine import ANT_KEYS, MiniRoadEngine, param_order
            d_rgb, d_flow, dtype, head = KINDS[kind]
            e = MiniRoadEngine(d_rgb, d_flow, EMB, HID, NCLS, self.dev, dtype)
            shapes = {"layer1.0.weight": (EMB, d_rgb + d_flow), "layer1.0.bias": (EMB,), "layer1.1.weight": (EMB,), "layer1.1.bias": (EMB,),
                      "gru.weight_ih_l0": (3 * HID, EMB), "gru.weight_hh_l0": (3 * HID, HID), "gru.bias_ih_l0": (3 * HID,),
                      "gru.bias_hh_l0": (3 * HID,), "f_classification.0.weight": (NCLS, HID), "f_classification.0.bias": (NCLS,),
                      ANT_KEYS[0]: (ANT_LEN * HID, HID), ANT_KEYS[1]: (ANT_LEN * HID,)}
            e.set_weights({k: self.zeros(shapes[k]) for k in param_order()})
            if head:
                e.set_anticipation(self.zeros(shapes[ANT_KEYS[0]]), self.zeros(shapes[ANT_KEYS[1]]), ANT_LEN)
            return e
        return self._once(("engine", kind), make)

    def pool(self, kind):
        def make():
            from prego_amd.stream_pool import StreamPool
            p = StreamPool(self.engine(kind), capacity=CAPACITY, window=VOTE_WINDOW, max_events=MAX_EVENTS)
            assert tuple(p.open() for _ in OPEN) == OPEN
            return p
        return self._once(("pool", kind), make)

    def vit(self, kind):
        def make():
            import prego_amd.transformer  # noqa: F401  registers "Transformer"
            from prego_amd.config import assembly101_cfg
            from prego_amd.registry import build_model
            cfg = assembly101_cfg(model="Transformer", window_size=VIT_WINDOW, patch_dim=1, num_heads=8, attn_dropout_rate=0.0, dropout=0.0,
                                  num_layers=1, compute_dtype="fp16", no_rgb=kind == "no_rgb")
            return build_model(cfg, str(self.dev)).eval()
        return self._once(("vit", kind), make)

    def vit_pool(self, kind):
        def make():
            p = self.vit(kind).stream_pool(capacity=CAPACITY, vote_window=VOTE_WINDOW, max_events=MAX_EVENTS)
            assert tuple(p.open() for _ in OPEN) == OPEN
            return p
        return self._once(("vit_pool", kind), make)

    def dims(self, entry, kind):
        """(d_rgb, d_flow, n_classes, anticipation_length) of the model behind `entry`"""
        if ENTRIES[entry][0] == "vit_pool":
            m = self.vit("no_rgb" if kind == "no_rgb" else "flow")
            return m.d_rgb, m.d_flow, m.out_dim, 0
        d_rgb, d_flow, _, head = KINDS[kind]
        return d_rgb, d_flow, NCLS, ANT_LEN if head else 1


INT = ("argmax", "ant_argmax")


def legal(ctx, entry, kind, n=N, k=K, counts=None):
    """(bound method, keyword arguments of a legal call of n streams with k frames each (or `counts`), legal shape by tensor name)"""
    owner, method, rowkind = ENTRIES[entry]
    d_rgb, d_flow, ncls, L = ctx.dims(entry, kind)
    counts = [k] * n if counts is None else counts
    rows = {"one": (n,), "frames": (n, k), "packed": (sum(counts),)}[rowkind]
    shapes = {"rgb": rows + (d_rgb,), "flow": rows + (d_flow,), "h": (n, HID), "out": rows + (ncls,), "argmax": rows,
              "ant_out": rows + (L, ncls), "ant_argmax": rows + (L,)}
    kw = {"rgb": ctx.zeros(shapes["rgb"]) if d_rgb else None, "flow": ctx.zeros(shapes["flow"]) if d_flow else None}
    if owner == "engine":
        kw["h"] = ctx.zeros(shapes["h"])
    else:
        kw["slots"] = [2, 0, 1][:n]
    if rowkind == "packed":
        kw["counts"] = counts
    obj = getattr(ctx, owner)("no_rgb" if (owner == "vit_pool" and kind == "no_rgb") else "flow" if owner == "vit_pool" else kind)
    return getattr(obj, method), kw, shapes


def wrong_tensor(ctx, shape, name, how):
    dtype = torch.int32 if name in INT else torch.float32
    if how == "device":
        return torch.zeros(shape, dtype=dtype)
    if how == "dtype":
        return ctx.zeros(shape, torch.int64 if name in INT else torch.float64)
    if how == "contiguity":
        t = ctx.zeros(shape[:-1] + (2 * shape[-1],), dtype)[..., ::2]
        assert tuple(t.shape) == tuple(shape) and not t.is_contiguous()
        return t
    return ctx.zeros((shape[0] + 1,) + tuple(shape[1:]), dtype)      # "shape": one row too many


def cases():
    """(case id, function of a Ctx that makes the call), in the order they run"""
    out = []

    def add(cid, entry, kind, change=None, **legal_kw):
        def go(ctx):
            fn, kw, shapes = legal(ctx, entry, kind, **legal_kw)
            if change is not None:
                change(ctx, kw, shapes)
            return fn(**kw)
        out.append((f"{entry}/{kind}/{cid}", go))

    def put(**new):
        return lambda ctx, kw, shapes: kw.update(new)

    def put_wrong(*pairs, **new):
        def change(ctx, kw, shapes):
            for name, how in pairs:
                kw[name] = wrong_tensor(ctx, shapes[name], name, how)
            kw.update(new)
        return change

    def extra_axis(name):
        def change(ctx, kw, shapes):
            kw[name] = kw[name][None] if len(shapes[name]) == 2 else kw[name][0]
        return change

    for entry in ENTRIES:
        vit, eng = entry in VIT, entry in ENGINE
        main = "flow" if vit else "ant"
        add("legal", entry, main)
        add("rgb-none", entry, main, put(rgb=None))
        add("flow-none", entry, "no_rgb", put(rgb=None, flow=None))
        if not vit:
            add("want-ant-no-head", entry, "flow", put(want_ant=True))
        # every tensor argument wrong in device, dtype, contiguity and shape in turn
        names = ["rgb", "flow"] + (["h"] if eng else []) + ([] if entry == "step" else ["out", "argmax"]) + ([] if vit else ["ant_out", "ant_argmax"])
        for name in names:
            for how in ("device", "dtype", "contiguity", "shape"):
                add(f"{name}-{how}", entry, "flow" if name == "flow" else main, put_wrong((name, how), **({"want_ant": True} if name.startswith("ant_") else {})))
        add("frames-rank", entry, main, extra_axis("rgb"))
        if ENTRIES[entry][2] == "packed":
            add("counts-length", entry, main, put(counts=[K, K, K]))
            add("counts-cuda", entry, main, lambda ctx, kw, shapes: kw.update(counts=torch.tensor(kw["counts"], device=ctx.dev)))
            add("counts-cpu-tensor", entry, main, lambda ctx, kw, shapes: kw.update(counts=torch.tensor(kw["counts"])))
            add("counts-one-int", entry, main, put(counts=K))
            add("counts-33", entry, main, counts=[33, 1])
            add("counts-second-0", entry, main, put(counts=[K, 0]), counts=[K])
        if ENTRIES[entry][2] == "frames":
            add("frames-33", entry, main, k=33)
        if not eng:
            add("slot-twice", entry, main, put(slots=[0, 0]))
            add("slot-closed", entry, main, put(slots=[0, CLOSED]))
        if entry in ("step_frames", "step_ragged") + POOL:
            add("not-built-for", entry, "fp32")
    # 258 rows: beyond every engine entry's 256 (the pools' capacity of 4 cannot name that many)
    add("rows-258", "step", "ant", n=258)
    add("rows-258", "step_wide", "ant", n=258)
    add("rows-258", "step_frames", "ant", n=129, k=2)
    add("rows-258", "step_ragged", "ant", n=129, k=2)
    # wrong in two ways: which message wins
    add("two:not-built-for+want-ant", "step_frames", "fp32", put(want_ant=True))
    add("two:want-ant+rgb-none", "step", "flow", put(want_ant=True, rgb=None))
    add("two:want-ant+rgb-none", "push", "flow", put(want_ant=True, rgb=None))
    add("two:slot-closed+counts-length", "push_ragged", "ant", put(slots=[0, CLOSED], counts=[K, K, K]))
    add("two:counts-length+rgb-none", "push_ragged", "ant", put(counts=[K, K, K], rgb=None))
    add("two:rgb-none+counts-cuda", "step_ragged", "ant", lambda ctx, kw, shapes: kw.update(rgb=None, counts=torch.tensor(kw["counts"], device=ctx.dev)))
    add("two:counts-33+rgb-none", "vit_push_bursts", "flow", put(counts=[33, 1], rgb=None))
    add("two:rgb-device+out-dtype", "step_wide", "ant", put_wrong(("rgb", "device"), ("out", "dtype")))
    add("two:frames-rank+out-device", "push_frames", "ant", lambda ctx, kw, shapes: kw.update(rgb=kw["rgb"][0], out=wrong_tensor(ctx, shapes["out"], "out", "device")))
    add("two:slot-twice+rgb-none", "vit_push", "flow", put(slots=[0, 0], rgb=None))
    add("two:h-dtype+ant-out-shape", "step_ragged", "ant", put_wrong(("h", "dtype"), ("ant_out", "shape")))
    add("two:not-built-for+slot-closed", "push", "fp32", put(slots=[0, CLOSED]))
    return out


def record(dev="cuda:0"):
    """[[case id, exception type or 'ok', message with the device's name replaced by <dev>], ...]"""
    ctx = Ctx(dev)
    got = []
    for cid, go in cases():
        try:
            go(ctx)
            got.append([cid, "ok", ""])
        except Exception as e:       # noqa: BLE001  the type is part of the record
            got.append([cid, type(e).__name__, str(e).replace(str(ctx.dev), "<dev>")])
    torch.cuda.synchronize(ctx.dev)
    return got
