"""`MiniROAD` behind the reference's plug-in API (step_recognition/model/rnn/rnn.py:18-71).

Same constructor (`MROAD(cfg)`), same `forward(rgb_input, flow_input) -> {'logits': ...}`
(probabilities in eval mode, raw logits in training mode, rnn.py:66-70), same
state_dict keys/shapes/dtypes (`gru.*`, `layer1.*`, `f_classification.*`), so reference
checkpoints load here and ours load there.  The torch sub-modules are parameter
containers only (constructed in the reference's order, so a given torch seed gives
the reference's initial weights); every FLOP runs in libprego_amd.so.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .config import FEATURE_SIZES
from .engine import MiniRoadEngine
from ._lib import PregoError
from .registry import META_ARCHITECTURES


@META_ARCHITECTURES.register("MiniROAD")
class MROAD(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.use_flow = not cfg["no_flow"]
        self.use_rgb = not cfg["no_rgb"]
        self.d_rgb = FEATURE_SIZES[cfg["rgb_type"]] if self.use_rgb else 0
        self.d_flow = FEATURE_SIZES[cfg["flow_type"]] if self.use_flow else 0
        self.input_dim = self.d_rgb + self.d_flow
        self.hidden_dim = cfg["hidden_dim"]
        self.num_layers = cfg["num_layers"]
        self.out_dim = cfg["num_classes"]
        self.window_size = cfg["window_size"]
        self.embedding_dim = cfg["embedding_dim"]
        if self.num_layers not in (1, 2):
            raise PregoError(f"prego_amd MiniROAD runs nn.GRU with num_layers 1 or 2 (cfg['num_layers'] = {self.num_layers})")
        # parameter containers, reference construction order (rnn.py:38-47)
        self.gru = nn.GRU(self.embedding_dim, self.hidden_dim, self.num_layers, batch_first=True)
        self.layer1 = nn.Sequential(
            nn.Linear(self.input_dim, self.embedding_dim),
            nn.LayerNorm(self.embedding_dim),
            nn.ReLU(),
            nn.Dropout(p=cfg["dropout"]),
        )
        self.f_classification = nn.Sequential(nn.Linear(self.hidden_dim, self.out_dim))
        # build-specific knobs (not reference keys)
        self.compute_dtype = cfg.get("compute_dtype", "fp16")          # 'fp16' | 'bf16' | 'fp32' | 'fp16x2' (split operands: fp32-class results)
        self.assume_zero_flow = bool(cfg.get("assume_zero_flow", False))  # dataset.py:69 zeroes the flow half
        self.grad_compress = cfg.get("grad_compress")                    # None | 'bf16': data-parallel gradient all-reduce on bf16 (half the bytes)
        self._engines = {}            # (device, operand dtype) -> [MiniRoadEngine, parameter versions its copies belong to]

    # -- engine plumbing -------------------------------------------------------------------
    def _engine_dtype(self, train: bool) -> str:
        # fp16 operands are an inference mode (same speed as bf16, 8x less operand rounding); the training kernels (kept
        # activations, BPTT, wgrads, fused AdamW copies) take bf16 / fp32 handles
        if train and self.compute_dtype == "fp16x2":
            return "fp32"           # the split-operand mode is inference only; its training counterpart is the exact-fp32 engine
        return "bf16" if (train and self.compute_dtype == "fp16") else self.compute_dtype

    @property
    def _engine(self):
        """the training-side engine if one exists (trainer: gradient bucket, timeout check), else the eval engine"""
        dev = self.layer1[0].weight.device
        for train in (True, False):
            ent = self._engines.get((dev, self._engine_dtype(train)))
            if ent is not None:
                return ent[0]
        return None

    def engine(self, train: bool = False) -> MiniRoadEngine:
        dev = self.layer1[0].weight.device
        key = (dev, self._engine_dtype(train))
        ent = self._engines.get(key)
        if ent is None:
            ent = [MiniRoadEngine(self.d_rgb, self.d_flow, self.embedding_dim, self.hidden_dim, self.out_dim, dev, key[1],
                                  num_layers=self.num_layers), None]
            self._engines[key] = ent
        vers = tuple((p.data_ptr(), p._version) for p in self.parameters())
        if vers != ent[1]:
            self._ingest(ent[0])
            ent[1] = vers
        return ent[0]

    def _ingest(self, eng: MiniRoadEngine):
        """hand the current parameters to the engine (it keeps converted copies)"""
        eng.set_weights(dict(self.named_parameters()))

    def _mark_ingested(self, train: bool = True):
        """the engine's operand copies were refreshed in place (fused AdamW): record the current parameter versions as theirs"""
        ent = self._engines.get((self.layer1[0].weight.device, self._engine_dtype(train)))
        if ent is not None:
            ent[1] = tuple((p.data_ptr(), p._version) for p in self.parameters())

    def forward(self, rgb_input, flow_input):
        if self.training:
            from .autograd import miniroad_train_forward
            return {"logits": miniroad_train_forward(self, rgb_input, flow_input)}
        eng = self.engine()
        src = rgb_input if self.use_rgb else flow_input
        B, T = src.shape[0], src.shape[1]
        rgb = [rgb_input[b].contiguous() for b in range(B)] if self.use_rgb else None
        if self.use_flow and (not self.assume_zero_flow or not self.use_rgb):
            flow = [flow_input[b].contiguous() for b in range(B)]       # --no_rgb: flow is the model's only input (rnn.py:54-57)
        else:
            flow = None
        outs, _, _ = eng.forward_ragged(rgb, flow, softmax=True)
        return {"logits": torch.stack(outs, 0)}

    @torch.no_grad()
    def forward_clips(self, rgb_list, flow_list=None, want_probs=True, want_argmax=True):
        """Ragged batched inference (the data-parallel hot path): many whole videos per call."""
        eng = self.engine()
        return eng.forward_ragged(rgb_list, flow_list, softmax=True, want_out=want_probs, want_argmax=want_argmax)

    link_fed_eval = True           # Evaluate may feed forward_clips while it runs (engine().plan_starts / set_feed_events)

    @property
    def max_clips(self) -> int:
        """videos `Evaluate` may hand to one forward_clips call"""
        return self.engine().max_clips

    def check(self):
        """surface a recurrence spin timeout of the eval engine (PregoError, PREGO_ETIMEOUT); synchronises the stream"""
        self.engine().check()

    @torch.no_grad()
    def step(self, rgb, flow, h):
        """Online inference (not exposed by the reference, whose eval loop runs whole videos): one new frame per stream.
        rgb [n, d_rgb] / flow [n, d_flow] (None = zeros), h [n, hidden_dim] = the GRU state, updated in place.  Returns
        (probabilities [n, C], argmax int32 [n]) - the eval branch of MROAD.forward (rnn.py:66-70) at T = 1 with h0 = h."""
        return self.engine().step(rgb, flow, h, softmax=True)

    @torch.no_grad()
    def step_wide(self, rgb, flow, h):
        """`step` for up to 256 streams per call: the weights are read once per call whatever n is (csrc/stream_wide.hip), and every
        stream's results are bit for bit those of a 5..16-stream `step`.  Returns what `step` returns."""
        return self.engine().step_wide(rgb, flow, h, softmax=True)

    @torch.no_grad()
    def step_frames(self, rgb, flow, h):
        """A burst: K frames per stream in one call, rgb [n, K, d_rgb] / flow [n, K, d_flow] (None = zeros), 1 <= K <= 32, n K <= 256; h
        [n, hidden_dim] is advanced by K frames in place.  Returns (probabilities [n, K, C], argmax int32 [n, K]), every frame bit for bit
        `step_wide`'s for a call of 5..256 streams (csrc/stream_frames.hip).  Longer backlogs: forward with h0 / h_last."""
        return self.engine().step_frames(rgb, flow, h, softmax=True, want_ant=False)

    @torch.no_grad()
    def step_ragged(self, rgb, flow, counts, h):
        """`step_frames` with a frame count per stream: counts[s] in 1..32, R = sum(counts) <= 256, rgb [R, d_rgb] / flow [R, d_flow] (None =
        zeros) packed - stream s owns rows off[s] .. off[s] + counts[s]), `prego_amd.stream_pool.pack_bursts` builds them; h [n, hidden_dim]:
        stream s is advanced by counts[s] frames in place.  Returns (probabilities [R, C], argmax int32 [R]), every row bit for bit
        `step_frames`'s (csrc/stream_frames.hip)."""
        return self.engine().step_ragged(rgb, flow, counts, h, softmax=True, want_ant=False)

    @torch.no_grad()
    def stream_pool(self, capacity: int = 256, window: int = 200, max_events: int = 1024):
        """A StreamPool (prego_amd/stream_pool.py) on this model's inference engine: every live video owns a slot with its GRU state and
        its running aggregation record; `push(slots, rgb, flow)` advances any subset by one frame with `step_wide`'s bits (MiniROADA: the
        anticipation head included), `push_frames` by a burst of K frames each, `push_ragged` by a burst of its own length per slot, `close(slot)` returns the stream's 'pred' / 'changes_pred' (utils/aggregate.py:46-90).  Built after
        the weights are final: the pool keeps the engine it was built on."""
        from .stream_pool import StreamPool
        return StreamPool(self, capacity=capacity, window=window, max_events=max_events)


@META_ARCHITECTURES.register("MiniROADA")
class MROADA(MROAD):
    """`MiniROADA` (rnn.py:73-136): the MiniROAD trunk plus an anticipation head on every frame, anticipation_length steps ahead, through
    the SAME f_classification weights.  Eval forward returns {'logits': [B, T, C], 'anticipation_logits': [B, T, L, C]}, both as
    probabilities (rnn.py:131-134); the head is the fused kernel of csrc/ant_head.hip (the [frames, L * H] intermediate is never
    materialised).  Parameter containers are built in the reference's order (layer1, f_actionness when cfg['actionness'], gru,
    f_classification, anticipation_layer), so a given torch seed gives the reference's initial weights and state_dict keys match
    (f_actionness.0.* included, which the reference builds but never uses in forward).  Training mode returns both as raw logits
    (rnn.py:128-130) through one autograd Function (csrc/ant_head_bwd.hip for the head's backward); f_actionness never gets a gradient.
    `step` is the online use: one frame per stream, with the head on the new state (csrc/stream_ant.hip).  fp16x2 handles are not built
    for this model."""

    def __init__(self, cfg):
        nn.Module.__init__(self)
        self.use_flow = not cfg["no_flow"]
        self.use_rgb = not cfg["no_rgb"]
        self.d_rgb = FEATURE_SIZES[cfg["rgb_type"]] if self.use_rgb else 0
        self.d_flow = FEATURE_SIZES[cfg["flow_type"]] if self.use_flow else 0
        self.input_dim = self.d_rgb + self.d_flow
        self.embedding_dim = cfg["embedding_dim"]
        self.hidden_dim = cfg["hidden_dim"]
        self.num_layers = cfg["num_layers"]
        self.anticipation_length = cfg["anticipation_length"]
        self.out_dim = cfg["num_classes"]
        self.window_size = cfg.get("window_size")
        if self.num_layers != 1:
            raise PregoError(f"prego_amd MiniROADA runs one GRU layer (its h0 is (1, B, H), rnn.py:122; cfg['num_layers'] = {self.num_layers})")
        if not 1 <= int(self.anticipation_length) <= 32:
            raise PregoError(f"prego_amd MiniROADA: anticipation_length {self.anticipation_length} must be in 1..32")
        # parameter containers, reference construction order (rnn.py:93-110)
        self.layer1 = nn.Sequential(
            nn.Linear(self.input_dim, self.embedding_dim),
            nn.LayerNorm(self.embedding_dim),
            nn.ReLU(),
            nn.Dropout(p=cfg["dropout"]),
        )
        self.actionness = cfg["actionness"]
        if self.actionness:
            self.f_actionness = nn.Sequential(nn.Linear(self.hidden_dim, 1))
        self.relu = nn.ReLU()
        self.gru = nn.GRU(self.embedding_dim, self.hidden_dim, self.num_layers, batch_first=True)
        self.f_classification = nn.Sequential(nn.Linear(self.hidden_dim, self.out_dim))
        self.anticipation_layer = nn.Sequential(nn.Linear(self.hidden_dim, self.anticipation_length * self.hidden_dim))
        self.compute_dtype = cfg.get("compute_dtype", "fp16")
        self.assume_zero_flow = bool(cfg.get("assume_zero_flow", False))
        self.grad_compress = None
        self._engines = {}

    # training follows MROAD's rule (fp16 trains on bf16, fp16x2 on fp32): MROAD._engine_dtype

    def _ingest(self, eng: MiniRoadEngine):
        eng.set_weights(dict(self.named_parameters()))
        eng.set_anticipation(self.anticipation_layer[0].weight, self.anticipation_layer[0].bias, self.anticipation_length)

    def _inputs(self, rgb_input, flow_input):
        src = rgb_input if self.use_rgb else flow_input
        B = src.shape[0]
        rgb = [rgb_input[b].contiguous() for b in range(B)] if self.use_rgb else None
        if self.use_flow and (not self.assume_zero_flow or not self.use_rgb):
            flow = [flow_input[b].contiguous() for b in range(B)]
        else:
            flow = None
        return rgb, flow

    def forward(self, rgb_input, flow_input):
        if self.training:
            src = rgb_input if self.use_rgb else flow_input
            if not src.is_cuda:
                raise PregoError("MiniROADA training is not built for CPU tensors: prego_amd has no CPU fallback")
            from .autograd import miniroada_train_forward
            logits, ant = miniroada_train_forward(self, rgb_input, flow_input)
            return {"logits": logits, "anticipation_logits": ant}
        rgb, flow = self._inputs(rgb_input, flow_input)
        outs, _, _, ant, _ = self.engine().forward_ragged(rgb, flow, softmax=True, want_ant=True, want_ant_argmax=False)
        return {"logits": torch.stack(outs, 0), "anticipation_logits": torch.stack(ant, 0)}

    @torch.no_grad()
    def forward_clips(self, rgb_list, flow_list=None, want_probs=True, want_argmax=True, want_ant=False):
        """Ragged batched inference.  want_ant=False: as MROAD.forward_clips (outs, argmax, None).  want_ant=True: (outs [T_i, C],
        argmax [T_i], None, anticipation probabilities [T_i, L, C], anticipation argmax int32 [T_i, L] (with want_argmax))."""
        return self.engine().forward_ragged(rgb_list, flow_list, softmax=True, want_out=want_probs, want_argmax=want_argmax,
                                            want_ant=want_ant)

    link_fed_eval = False

    @torch.no_grad()
    def step(self, rgb, flow, h):
        """Online inference: one new frame per stream, as MROAD.step, with the anticipation head on the new state.  Returns (probabilities
        [n, C], argmax int32 [n], anticipation probabilities [n, L, C], anticipation argmax int32 [n, L]) - the eval branch of
        MROADA.forward (rnn.py:131-135) at T = 1 with h0 = h; h is updated in place.  bf16 / fp16 models of hidden_dim 1024 run the
        streaming kernels (csrc/stream_step.hip, csrc/stream_ant.hip), the others the general forward."""
        return self.engine().step(rgb, flow, h, softmax=True, want_ant=True)

    @torch.no_grad()
    def step_wide(self, rgb, flow, h):
        """`step` for up to 256 streams per call, the anticipation head included (csrc/stream_wide.hip).  Returns what `step` returns."""
        return self.engine().step_wide(rgb, flow, h, softmax=True, want_ant=True)

    @torch.no_grad()
    def step_frames(self, rgb, flow, h):
        """`MROAD.step_frames` with the anticipation head on the state after every frame.  Returns (probabilities [n, K, C], argmax int32
        [n, K], anticipation probabilities [n, K, L, C], anticipation argmax int32 [n, K, L])."""
        return self.engine().step_frames(rgb, flow, h, softmax=True, want_ant=True)

    @torch.no_grad()
    def step_ragged(self, rgb, flow, counts, h):
        """`MROAD.step_ragged` with the anticipation head on the state after every frame.  Returns (probabilities [R, C], argmax int32 [R],
        anticipation probabilities [R, L, C], anticipation argmax int32 [R, L])."""
        return self.engine().step_ragged(rgb, flow, counts, h, softmax=True, want_ant=True)
