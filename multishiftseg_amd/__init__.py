"""multishiftseg_amd: the MultiShiftSeg networks on hand-written HIP kernels for the MI355X. Sub-modules are imported on demand
(`from multishiftseg_amd import kernels`); the names below are the package's module-level mirrors of reference classes."""

_M2F_TRAINER = ("build_m2f_param_groups", "build_m2f_optimizer", "m2f_weight_dict", "weighted_losses", "M2FTrainStep", "M2FStage1Step",
                "attach_grad_sync", "target_count")
_DDP = ("GradAllReduce", "CountAllReduce", "global_num_masks", "shard_pairs", "shard_batches")
_STAGE1_KERNELS = ("m2f_semantic_inference", "upsample_bilinear_nhwc", "stage1_chunks")


def __getattr__(name):
    if name == "MultiScaleMaskedTransformerDecoder_GMA":
        from .transformer_decoder import MultiScaleMaskedTransformerDecoder_GMA
        return MultiScaleMaskedTransformerDecoder_GMA
    if name == "HungarianMatcher":
        from .matcher import HungarianMatcher
        return HungarianMatcher
    if name == "SetCriterion":
        from .criterion import SetCriterion
        return SetCriterion
    if name == "class_mix_upsample":
        from .criterion import class_mix_upsample
        return class_mix_upsample
    if name == "class_mix_ood_loss":
        from .ood_loss import class_mix_ood_loss
        return class_mix_ood_loss
    if name == "masked_attention":
        from .kernels import masked_attention
        return masked_attention
    if name == "conv2d_dgrad_s2":
        from .kernels import conv2d_dgrad_s2
        return conv2d_dgrad_s2
    if name == "stem7_wgrad":
        from .kernels import stem7_wgrad
        return stem7_wgrad
    if name in ("prepare_targets", "M2FTargets"):
        from . import m2f_targets
        return getattr(m2f_targets, name)
    if name in ("ResNet", "build_resnet_backbone"):
        from . import resnet
        return getattr(resnet, name)
    if name == "MaskFormer":
        from .maskformer import MaskFormer
        return MaskFormer
    if name in _STAGE1_KERNELS:
        from . import kernels
        return getattr(kernels, name)
    if name in _M2F_TRAINER:
        from . import m2f_trainer
        return getattr(m2f_trainer, name)
    if name in _DDP:
        from . import ddp
        return getattr(ddp, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["MultiScaleMaskedTransformerDecoder_GMA", "HungarianMatcher", "SetCriterion", "class_mix_upsample", "class_mix_ood_loss", "masked_attention",
           "conv2d_dgrad_s2", "stem7_wgrad", "prepare_targets", "M2FTargets", "ResNet", "build_resnet_backbone", "MaskFormer", *_M2F_TRAINER,
           *_STAGE1_KERNELS, *_DDP]
