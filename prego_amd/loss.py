"""`OadLoss` ("NONUNIFORM") behind the reference's CRITERIONS registry (criterions/loss.py:6-37): last frame only,
target L2-normalised per row (F.normalize, eps 1e-12), mean over the batch of sum_k -(y_k) log_softmax(logits)_k.
Loss value and dloss/dlogits come from one HIP kernel (csrc/train.hip::oad_loss_kernel)."""
from __future__ import annotations

import torch.nn as nn

from .autograd import oad_loss_autograd
from .registry import CRITERIONS


@CRITERIONS.register("NONUNIFORM")
class OadLoss(nn.Module):
    def __init__(self, cfg, reduction="mean"):
        super().__init__()
        if reduction not in ("mean", "sum"):         # loss.py:30-33 knows these two (anything else leaves `loss` unbound there)
            raise ValueError(f"OadLoss: reduction {reduction!r}: expected 'mean' or 'sum'")
        self.reduction = reduction
        self.num_classes = cfg["num_classes"]

    def forward(self, out_dict, target):
        return oad_loss_autograd(out_dict["logits"], target, self.reduction)


@CRITERIONS.register("ANTICIPATION")
class OadAntLoss(nn.Module):
    """`OadAntLoss` (criterions/loss.py:40-79): the multi-label cross entropy of OadLoss on the LAST frame's anticipation logits,
    anticipation_logits[:, -1] [B, L, C] taken as B * L one-frame rows against ant_target.view(-1, C); reduction 'sum' by default.
    Value and dloss/dlogits come from the same HIP kernel as OadLoss (prego_oad_loss_reduce); autograd carries the gradient back
    through the slice to anticipation_logits."""

    def __init__(self, cfg, reduction="sum"):
        super().__init__()
        if reduction not in ("mean", "sum"):
            raise ValueError(f"OadAntLoss: reduction {reduction!r}: expected 'mean' or 'sum'")
        self.reduction = reduction
        self.num_classes = cfg["num_classes"]

    def forward(self, out_dict, target, ant_target):
        C = self.num_classes
        last = out_dict["anticipation_logits"][:, -1, :, :].reshape(-1, 1, C)
        return oad_loss_autograd(last, ant_target.reshape(-1, 1, C), self.reduction)
