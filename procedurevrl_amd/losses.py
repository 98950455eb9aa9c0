"""Loss table (reference: lib/models/losses.py:11-61).  `MILNCELoss` runs on the HIP path and, unlike the
reference's hard-coded `.cuda()` (losses.py:18), works on whatever device the embeddings live on.  `SoftTargetCrossEntropy`
is timm's loss of the Mixup fine-tuning branch (tools/train_net.py:137-143), also on the HIP path."""
import torch.nn as nn

from .functional import milnce_loss, soft_target_cross_entropy


class MILNCELoss(nn.Module):
    def forward(self, video_embd, text_embd):
        return milnce_loss(video_embd, text_embd)


class SoftTargetCrossEntropy(nn.Module):
    """timm.loss.SoftTargetCrossEntropy: mean over rows of sum_j -target_j * log_softmax(x)_j.  `target` is a dense fp32
    [rows, K] tensor, or -- `forward(x, labels=..., plan=...)` -- the mixed target of hard labels under a mixup.MixPlan, which
    the kernel synthesises without materialising it."""

    def __init__(self, reduction="mean"):
        super().__init__()
        if reduction != "mean":
            raise NotImplementedError("SoftTargetCrossEntropy reduces by the mean over rows only")

    def forward(self, x, target=None, labels=None, plan=None):
        return soft_target_cross_entropy(x, target, labels, plan)


_LOSSES = {"cross_entropy": nn.CrossEntropyLoss, "bce": nn.BCELoss, "bce_logit": nn.BCEWithLogitsLoss, "milnce": MILNCELoss,
           "soft_target_cross_entropy": SoftTargetCrossEntropy}


def get_loss_func(loss_name):
    if loss_name not in _LOSSES.keys():
        raise NotImplementedError("Loss {} is not supported".format(loss_name))
    return _LOSSES[loss_name]
