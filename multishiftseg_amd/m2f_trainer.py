"""The stage-2 training step of Mask2Former around the HIP optimizer (optim.AdamW): the parameter groups and the optimizer of
train_m2f.py:211-299, the weight dict of maskformer_model.py:143-153 and its application :253-258, and M2FTrainStep, which runs
zero_grad / head / criterion / weighted sum / backward / clipped AdamW step. The reference reads every value from a detectron2
config; here each is an argument. One process, one GPU: no DDP.
Stage 1 (the epochs before warmup_epoch, train_m2f.py:437-447): M2FStage1Step trains class_embed2 alone under optim.Adam with
RelContrastiveLoss on MaskFormer.stage1_forward's (sem_seg, ood_score)."""
import torch
from torch import nn

from .optim import Adam, AdamW
from .trainer import configure_trainable_params

# train_m2f.py:233-244
NORM_MODULE_TYPES = (
    nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm, nn.GroupNorm, nn.InstanceNorm1d, nn.InstanceNorm2d,
    nn.InstanceNorm3d, nn.LayerNorm, nn.LocalResponseNorm,
)


def build_m2f_param_groups(model, base_lr, weight_decay, weight_decay_norm=0.0, weight_decay_embed=0.0, backbone_multiplier=0.1):
    """train_m2f.py:246-265: one {"params": [tensor], "lr", "weight_decay"} group per trainable tensor, in named_modules() order,
    each tensor once (by identity; a tensor shared under two names takes the rules of its first name). lr = base_lr, times
    backbone_multiplier where the MODULE name contains "backbone"; weight decay = weight_decay, then 0 for a parameter named
    relative_position_bias_table / absolute_pos_embed, then weight_decay_norm inside a norm module, then weight_decay_embed inside
    an nn.Embedding: a later rule overrides an earlier one."""
    groups, memo = [], set()
    for module_name, module in model.named_modules():
        for param_name, p in module.named_parameters(recurse=False):
            if not p.requires_grad or id(p) in memo:
                continue
            memo.add(id(p))
            lr, wd = base_lr, weight_decay
            if "backbone" in module_name:
                lr = lr * backbone_multiplier
            if "relative_position_bias_table" in param_name or "absolute_pos_embed" in param_name:
                wd = 0.0
            if isinstance(module, NORM_MODULE_TYPES):
                wd = weight_decay_norm
            if isinstance(module, nn.Embedding):
                wd = weight_decay_embed
            groups.append({"params": [p], "lr": lr, "weight_decay": wd})
    return groups


def build_m2f_optimizer(model, base_lr=1e-5, weight_decay=0.05, weight_decay_norm=0.0, weight_decay_embed=0.0, backbone_multiplier=0.1,
                        optimizer="ADAMW", clip_value=0.01):
    """train_m2f.py:267-299 for OPTIMIZER "ADAMW" with CLIP_GRADIENTS of type "full_model": AdamW over build_m2f_param_groups with
    clip_grad_norm_(all parameters, clip_value) inside every step (clip_value 0 / None: no clipping, as the reference's
    `clip_norm_val > 0.0`). Defaults: anomaly_ft.yaml:5 and Base-Cityscapes-SemanticSegmentation.yaml:25-33."""
    if optimizer != "ADAMW":
        raise NotImplementedError(f"build_m2f_optimizer has ADAMW only (no optimizer type {optimizer})")
    groups = build_m2f_param_groups(model, base_lr, weight_decay, weight_decay_norm, weight_decay_embed, backbone_multiplier)
    return AdamW(groups, lr=base_lr, max_norm=clip_value or None)


def m2f_weight_dict(class_weight, mask_weight, dice_weight, ood_weight, dec_layers, deep_supervision):
    """maskformer_model.py:143-153: the eight weighted keys, and with deep supervision `<key>_<i>` for i < dec_layers - 1."""
    weight_dict = {"loss_ce": class_weight, "loss_mask": mask_weight, "loss_dice": dice_weight, "loss_ood": ood_weight,
                   "loss_original_mask": mask_weight, "loss_original_dice": dice_weight, "loss_aug_mask": mask_weight,
                   "loss_aug_dice": dice_weight}
    if deep_supervision:
        aux = {}
        for i in range(dec_layers - 1):
            aux.update({f"{k}_{i}": v for k, v in weight_dict.items()})
        weight_dict.update(aux)
    return weight_dict


def weighted_losses(losses, weight_dict):
    """maskformer_model.py:253-258 out of place: {k: losses[k] * weight_dict[k]} for the keys of `losses` that `weight_dict` has, in
    the order of `losses`; the others are dropped. A new dict of new tensors: the criterion's entries are views of one table."""
    return {k: v * weight_dict[k] for k, v in losses.items() if k in weight_dict}


class M2FTrainStep:
    """One stage-2 step: optimizer.zero_grad() ; outputs = head(*head_args) ; criterion(outputs, targets, **criterion_kwargs) ;
    weighted_losses with the criterion's weight_dict ; sum ; backward ; optimizer.step(). `head` is any callable that returns the
    outputs dict (MultiScaleMaskedTransformerDecoder_GMA.set_trainable(), alone or behind the pixel decoder). Returns (the
    detached weighted losses, the total gradient norm before clipping as a 0-d device tensor, None without clipping)."""

    def __init__(self, head, criterion, optimizer):
        self.head, self.criterion, self.optimizer = head, criterion, optimizer

    def __call__(self, *head_args, targets, **criterion_kwargs):
        self.optimizer.zero_grad(set_to_none=True)
        outputs = self.head(*head_args)
        losses = weighted_losses(self.criterion(outputs, targets, **criterion_kwargs), self.criterion.weight_dict)
        if not losses:
            raise ValueError("M2FTrainStep: no loss of the criterion has a weight in its weight_dict")
        sum(losses.values()).backward()
        norm = self.optimizer.step()
        return {k: v.detach() for k, v in losses.items()}, norm


class M2FStage1Step:
    """One stage-1 step (train_m2f.py:414-456 for epoch < warmup_epoch; M2F.yaml:9, 24-27): only the parameters whose name contains
    one of `patterns` train (trainer.configure_trainable_params sets every requires_grad), under the HIP Adam with torch's L2
    weight decay. __call__(images, target): zero_grad ; (sem_seg, ood_score) = model.stage1_forward(images) ;
    loss(sem_seg, ood_score, target).mean() ; backward ; step -> the detached loss. `loss` is RelContrastiveLoss (it needs an even
    batch [orig...; aug...] and changes `target` in place, as the reference's does)."""

    def __init__(self, model, loss, lr=1e-4, weight_decay=1e-4, patterns=("class_embed2",)):
        self.model, self.loss = model, loss
        params, self.names = configure_trainable_params(model, tuple(patterns))
        if not params:
            raise ValueError(f"M2FStage1Step: no parameter name contains one of {tuple(patterns)}")
        self.optimizer = Adam(params, lr=lr, weight_decay=weight_decay)

    def __call__(self, images, target):
        self.optimizer.zero_grad(set_to_none=True)
        sem_seg, ood_score = self.model.stage1_forward(images)
        loss = self.loss(sem_seg, ood_score, target).mean()
        loss.backward()
        self.optimizer.step()
        return loss.detach()
