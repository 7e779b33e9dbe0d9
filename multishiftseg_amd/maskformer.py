"""The shell of Mask2Former: image batch -> anomaly score with the validation / test sweep around it, and, after set_trainable(),
image batch -> the predictor's training outputs for a whole-model stage-2 step.

Host-side mirror of the inference branch of ``MaskFormer.forward`` (lib/network/mask2former/maskformer_model.py:229-234,
260-277) together with the score the trainer forms from its output (train_m2f.py:387-407). The children keep the reference's
names -- ``backbone``, ``sem_seg_head.pixel_decoder``, ``sem_seg_head.predictor`` -- so a MaskFormer checkpoint's keys line up and
m2f_trainer.build_m2f_param_groups finds "backbone" in the module names.

The shell adds no arithmetic of its own: it zero-pads the batch bottom/right to the size divisibility (ImageList.from_tensors;
there is no pixel normalisation, the reference fork has none either), runs backbone -> pixel_decoder.forward_features -> predictor
with ``fuse_score`` and hands back what kernels.m2f_score_fused returns, already cropped to the images' own size.
Training (maskformer_model.py:235-258 without the criterion, which m2f_trainer.M2FTrainStep applies): ``set_trainable()`` switches
the backbone (ResNet.set_trainable) and the predictor; with it on and grad mode enabled forward() runs pad -> backbone ->
pixel_decoder.forward_features -> predictor on their autograd nodes, without ``fuse_score``, and returns the predictor's training
outputs dict for the padded batch. Off, or under torch.no_grad(), the shell is the evaluation shell.
Stage 1 (train_m2f.py:437-447, M2F.yaml:9): ``stage1_forward`` runs the backbone and the pixel decoder as in evaluation and the
predictor with ``semantic``: -> (the first 19 channels of the ``sem_seg`` map of semantic_inference, maskformer_model.py:341-345,
and the anomaly score of get_anomaly_score on the upsampled ``*_ood`` heads), the score attached to ``class_embed2`` alone.
``semantic_inference`` is the closed-set prediction by itself.
"""
import torch
from torch import nn

from .metric import OODMeter


def padded_size(size, divisibility):
    """ImageList.from_tensors: the next multiple of `divisibility` (<= 1: the size itself)."""
    if divisibility <= 1:
        return int(size)
    return (int(size) + divisibility - 1) // divisibility * divisibility


class _SemSegHead(nn.Module):
    """MaskFormerHead's two children under its names (mask_former_head.py: pixel_decoder, predictor)."""

    def __init__(self, pixel_decoder, predictor):
        super().__init__()
        self.pixel_decoder = pixel_decoder
        self.predictor = predictor


class MaskFormer(nn.Module):
    def __init__(self, backbone, pixel_decoder, predictor, size_divisibility=32):
        super().__init__()
        self.backbone = backbone
        self.sem_seg_head = _SemSegHead(pixel_decoder, predictor)
        if size_divisibility < 0:
            size_divisibility = getattr(backbone, "size_divisibility", 32)             # maskformer_model.py:77-79
        self.size_divisibility = size_divisibility
        self._trainable = False

    def set_trainable(self, flag=True, stem=False):
        """Opt in to (or out of) the differentiable path of the backbone and the predictor (the pixel decoder has no switch: it follows
        its parameters' requires_grad). With it on and grad mode enabled forward() returns the predictor's training outputs for the
        padded batch, so M2FTrainStep(head=model, ...) runs a whole-model step; off, or under torch.no_grad(), nothing changes.
        stem: ResNet.set_trainable's second opt-in -- backbone.stem.conv1.weight is trained too (the reference's stage-2 set of 53
        backbone weights with backbone.freeze(0, norms=True)); False (the default) refuses a trainable stem as before."""
        self._trainable = bool(flag)
        self.backbone.set_trainable(flag, stem=stem)
        self.sem_seg_head.predictor.set_trainable(flag)
        return self

    def pad(self, images):
        """[B, 3, H, W] -> [B, 3, Hp, Wp], zeros at the bottom and the right; the batch itself where nothing is to pad."""
        H, W = images.shape[-2:]
        Hp, Wp = padded_size(H, self.size_divisibility), padded_size(W, self.size_divisibility)
        if (Hp, Wp) == (H, W):
            return images
        out = images.new_zeros(images.shape[:-2] + (Hp, Wp))
        out[..., :H, :W] = images
        return out

    def forward(self, images):
        """The predictor's dict for the padded batch, with "ood_score" [B, H, W] at the images' own size -- or, after set_trainable()
        and with grad mode enabled, its training outputs (no "ood_score": fuse_score is inference-only)."""
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"MaskFormer takes [B, 3, H, W] image batches, got {tuple(images.shape)}")
        H, W = images.shape[-2:]
        if self._trainable and torch.is_grad_enabled():
            features = self.backbone(self.pad(images.float()))
            mask_features, _, multi_scale = self.sem_seg_head.pixel_decoder.forward_features(features)
            return self.sem_seg_head.predictor(multi_scale, mask_features, None)
        with torch.no_grad():
            x = self.pad(images.float())
            features = self.backbone(x)
            mask_features, _, multi_scale = self.sem_seg_head.pixel_decoder.forward_features(features)
            return self.sem_seg_head.predictor(multi_scale, mask_features, None, fuse_score=(x.shape[-2], x.shape[-1], H, W))

    def ood_score(self, images):
        """Anomaly score [B, H, W] (train_m2f.py:387-407 on maskformer_model.py:260-277)."""
        return self.forward(images)["ood_score"]

    def _semantic(self, images):
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"MaskFormer takes [B, 3, H, W] image batches, got {tuple(images.shape)}")
        if self._trainable:
            raise RuntimeError("MaskFormer: sem_seg / stage 1 run on the evaluation path of the backbone and the predictor: "
                               "set_trainable(False) first")
        H, W = images.shape[-2:]
        with torch.no_grad():
            x = self.pad(images.float())
            features = self.backbone(x)
            mask_features, _, multi_scale = self.sem_seg_head.pixel_decoder.forward_features(features)
        return self.sem_seg_head.predictor(multi_scale, mask_features, None, semantic=(x.shape[-2], x.shape[-1], H, W))

    def semantic_inference(self, images):
        """The closed-set prediction [B, 19, H, W] at the images' own size: the first 19 channels of the "sem_seg" map of
        maskformer_model.py:296-301, 341-345 (the per-instance channels behind them are what every caller slices off)."""
        with torch.no_grad():
            return self._semantic(images)["sem_seg"]

    def stage1_forward(self, images):
        """(sem_seg [B, 19, H, W], ood_score [B, H, W]) of train_m2f.py:438-446 at the images' own size. The backbone and the pixel
        decoder run as in evaluation, under no_grad; the predictor is forward-only apart from class_embed2, the only parameters a
        backward from ood_score reaches (any other trainable predictor parameter raises there). sem_seg never requires grad."""
        out = self._semantic(images)
        return out["sem_seg"], out["ood_score"]

    def evaluate(self, batches, meter=None, seg_meter=None, group=None):
        """valid_batch / test (train_m2f.py:469-509, test_m2f.py:109-158) with no copy to the host: `batches` yields (images, target);
        every score map goes to OODMeter.update on the device. Returns meter.compute().
        seg_meter (a metric.SegMeter): the closed-set half of the sweep as well -- ONE forward per batch feeds both meters, its
        "ood_score" the OODMeter and its "sem_seg" logits the SegMeter (the argmax is fused into the count). The score is the fused
        one of the sweep without a seg_meter, so the OOD measures are the same numbers; sem_seg is semantic_inference's map, built
        from the same last-step mask logits. Returns (meter.compute(), seg_meter.compute()).
        group (a process group, or True for the default one): the sweep is split over the ranks. Each rank consumes the `batches` it
        is given -- the caller shards them, e.g. ddp.shard_batches(loader) -- and after the loop every rank, one with an empty shard
        too, gathers the OOD keys and sums the confusion matrix (ddp.gather_meters), so every rank returns what one process
        returns over all batches, bit for bit. A rank that raises inside its sweep raises before the collective: its
        peers wait there until the process group's timeout. None: no collective, the sweep of one process."""
        meter = OODMeter() if meter is None else meter
        if seg_meter is None:
            for images, target in batches:
                meter.update(self.ood_score(images), target)
        else:
            if self._trainable:
                raise RuntimeError("MaskFormer: sem_seg runs on the evaluation path of the backbone and the predictor: set_trainable(False) first")
            for images, target in batches:
                if images.dim() != 4 or images.shape[1] != 3:
                    raise ValueError(f"MaskFormer takes [B, 3, H, W] image batches, got {tuple(images.shape)}")
                H, W = images.shape[-2:]
                with torch.no_grad():
                    x = self.pad(images.float())
                    features = self.backbone(x)
                    mask_features, _, multi_scale = self.sem_seg_head.pixel_decoder.forward_features(features)
                    out = self.sem_seg_head.predictor(multi_scale, mask_features, None, fuse_score=(x.shape[-2], x.shape[-1], H, W), sem_seg=True)
                meter.update(out["ood_score"], target)
                seg_meter.update(out["sem_seg"], target)
        if group is not None:
            from . import ddp
            ddp.gather_meters(group, meter, seg_meter)
        if seg_meter is None:
            return meter.compute()
        return meter.compute(), seg_meter.compute()
