"""`FusedAdamW`: torch.optim.AdamW as step_recognition/main.py:62-67 builds it (same constructor arguments, same `state`
entries - 'step', 'exp_avg', 'exp_avg_sq' - so optimizer state dicts interchange), with the arithmetic in ONE fused HIP launch
over all tensors (csrc/optim.hip) instead of torch's per-op kernels.  For a `MiniROAD` model the step also rewrites the engine's
bf16 / fp32 operand copies of the weights from the updated values in the same pass, so the training loop never re-ingests the
17.9 M parameters (`prego_miniroad_set_weights`) after `optimizer.step()`; for a `Transformer` (ViTEnc) model the same through
`prego_vit_adamw_step` (its set_weights is 5 + 4 per layer conversions and 10 + 7 per layer device copies)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import PregoError, check, ptr_array
from .engine import ANT_KEYS, _PARAM_ORDER, _stream_ptr


def _fused_keys(model):
    """the tensors the fused MiniROAD step updates: the ten of prego_miniroad_adamw_step, plus MiniROADA's anticipation_layer (its own launch)"""
    return list(_PARAM_ORDER) + (list(ANT_KEYS) if hasattr(model, "anticipation_layer") else [])


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, model=None):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._model = model if model is not None and hasattr(model, "engine") and hasattr(model, "gru") else None
        # the "Transformer" entry (ViTEnc): same idea through prego_vit_adamw_step
        self._vit = model if model is not None and hasattr(model, "_handle") and hasattr(model, "pre_head_ln") else None

    def is_guarded_for(self, model) -> bool:
        """True when step() runs `prego_miniroad_adamw_step` for exactly this model's ten tensors: that launch is a no-op on the DEVICE
        while the engine's timeout word is set (a forward / backward that gave up), so a training loop may call step() without
        synchronising first (prego_amd/trainer.py)."""
        if self._model is None or self._model is not model or len(self.param_groups) != 1:
            return False
        named = dict(model.named_parameters())
        keys = _fused_keys(model)
        want = {id(named[k]) for k in keys if k in named}
        # MiniROADA's f_actionness (cfg['actionness']) is built but never used in forward (rnn.py:98-99): it never has a gradient, so
        # every step skips it, as torch.optim.AdamW does
        idle = {id(p) for k, p in named.items() if k.startswith("f_actionness.")}
        have = {id(p) for p in self.param_groups[0]["params"]} - idle
        return len(want) == len(keys) and want == have and all(p.is_cuda for p in self.param_groups[0]["params"])

    def _state(self, p):
        st = self.state[p]
        if not st:
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            for p in ps:
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise PregoError("FusedAdamW: parameters must be contiguous fp32 CUDA tensors (the HIP path has no CPU fallback)")
            states = [self._state(p) for p in ps]
            steps = {int(st["step"].item()) for st in states}
            if len(steps) != 1:
                raise PregoError("FusedAdamW: parameters of one group must share the step count")
            step = steps.pop() + 1               # st['step'] moves only after the launch below was accepted
            grads = [p.grad.contiguous() for p in ps]
            dev = ps[0].device
            b1, b2 = group["betas"]
            hyper = (step, float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))
            m = self._model
            fused_model = False
            if m is not None:
                named = dict(m.named_parameters())
                want = [named[k] for k in _fused_keys(m)]
                fused_model = len(ps) == len(want) and {id(p) for p in ps} == {id(p) for p in want}
                if fused_model:             # the C ABI takes the ten tensors in prego_miniroad_set_weights' order
                    ps = want
                    states = [self.state[p] for p in ps]
                    grads = [p.grad.contiguous() for p in ps]
            fused_vit = False
            if self._vit is not None and not fused_model:
                from .transformer import _tensor_order
                v = self._vit
                named = dict(v.named_parameters())
                want = [named[k] for k in _tensor_order(v.num_layers)]
                fused_vit = len(ps) == len(want) and {id(p) for p in ps} == {id(p) for p in want}
                if fused_vit:               # prego_vit_set_weights' order
                    ps = want
                    states = [self.state[p] for p in ps]
                    grads = [p.grad.contiguous() for p in ps]
            with torch.cuda.device(dev):
                if fused_vit:
                    self._vit._handle()     # weights ingested (a no-op after the forward of this step)
                    check(lib.prego_vit_adamw_step(
                        self._vit._h, ptr_array([p.data_ptr() for p in ps]), ptr_array([g.data_ptr() for g in grads]),
                        ptr_array([st["exp_avg"].data_ptr() for st in states]), ptr_array([st["exp_avg_sq"].data_ptr() for st in states]),
                        len(ps), *hyper, C.c_void_p(_stream_ptr(dev))))
                    # raw-pointer update: bump the versions (autograd's in-place check, caches keyed on (data_ptr, _version)),
                    # then record the new versions as the ones the handle's copies belong to, so that the re-ingest is still skipped
                    torch._C._increment_version(ps)
                    sd = dict(self._vit.named_parameters())
                    self._vit._ver = tuple((p.data_ptr(), p._version) for p in sd.values())
                elif fused_model:
                    eng = m.engine(train=True)        # weights already ingested (versions unchanged since the forward)
                    n0 = len(_PARAM_ORDER)
                    check(lib.prego_miniroad_adamw_step(
                        eng.h, ptr_array([p.data_ptr() for p in ps[:n0]]), ptr_array([g.data_ptr() for g in grads[:n0]]),
                        ptr_array([st["exp_avg"].data_ptr() for st in states[:n0]]),
                        ptr_array([st["exp_avg_sq"].data_ptr() for st in states[:n0]]), *hyper, C.c_void_p(_stream_ptr(dev))))
                    if len(ps) > n0:        # MiniROADA: anticipation_layer.0.{weight, bias}, same guard, W_a operand copy rewritten
                        check(lib.prego_miniroad_adamw_step_anticipation(
                            eng.h, ptr_array([p.data_ptr() for p in ps[n0:]]), ptr_array([g.data_ptr() for g in grads[n0:]]),
                            ptr_array([st["exp_avg"].data_ptr() for st in states[n0:]]),
                            ptr_array([st["exp_avg_sq"].data_ptr() for st in states[n0:]]), *hyper, C.c_void_p(_stream_ptr(dev))))
                    # the engine's operand copies are now those of the NEW values: bump the parameter versions (raw-pointer
                    # update) and record them as ingested, so model.engine() does not re-ingest
                    # the data-parallel peer guard (engine.backward) pointed into THIS step's gradient bucket: one step, one flag
                    check(lib.prego_miniroad_set_peer_guard(eng.h, None))
                    torch._C._increment_version(ps)
                    m._mark_ingested(train=True)
                else:
                    numel = (C.c_int64 * len(ps))(*[p.numel() for p in ps])
                    check(lib.prego_adamw_step(
                        len(ps), ptr_array([p.data_ptr() for p in ps]), ptr_array([g.data_ptr() for g in grads]),
                        ptr_array([st["exp_avg"].data_ptr() for st in states]), ptr_array([st["exp_avg_sq"].data_ptr() for st in states]),
                        numel, *hyper, C.c_void_p(_stream_ptr(dev))))
                    torch._C._increment_version(ps)      # raw-pointer update: tell autograd / the weight caches the values moved
            for st in states:
                st["step"] += 1
        return loss
