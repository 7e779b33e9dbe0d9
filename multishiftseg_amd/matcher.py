"""HungarianMatcher of Mask2Former (lib/network/mask2former/modeling/matcher.py:70-189) on the HIP kernels of csrc/m2f_match.hip.

The reference solves one image at a time: draw points, two grid_samples, four einsums, a `.cpu()` of the [Q, T] cost and scipy's
linear_sum_assignment -- 16 images x 10 prediction steps = 160 host round trips per train step. Here all S x B problems of a step
are two launches and one device-to-host copy (`match_steps`), or none (`device_only=True`). There is no CPU path.
"""
import torch
from torch import nn

from . import kernels as K
from .m2f_targets import M2FTargets

MAX_QUERIES = 128       # include/mss_hip.h: T_b <= Q <= 128
MAX_STEPS = 16


def pairs_from_table(table, counts):
    """Host conversion of a match table [S,B,Tmax] (int, CPU: the query of target m, -1 in the padding) into the reference's
    return value: per step a list over images of (index_i, index_j) int64 tensors, index_i (queries) ascending, index_j the
    targets matched to them, len = T_b (matcher.py:153-156; scipy returns its row indices sorted)."""
    table = torch.as_tensor(table).to(torch.int64)
    out = []
    for s in range(table.shape[0]):
        per_image = []
        for b, t in enumerate(counts):
            i = table[s, b, :t]
            order = torch.argsort(i)
            per_image.append((i[order].contiguous(), order.contiguous()))
        out.append(per_image)
    return out


def _steps_of(outputs_list):
    """[last output, aux_outputs ...] of a model output dict, or the list as given."""
    if isinstance(outputs_list, dict):
        return [outputs_list] + list(outputs_list.get("aux_outputs", []))
    return list(outputs_list)


class HungarianMatcher(nn.Module):
    """Assignment between the targets and the predictions of the network (matcher.py:70-76): constructor, assertion, forward()
    result and __repr__ of the reference; `num_points` points are sampled per image and shared by all of its masks."""

    def __init__(self, cost_class: float = 1, cost_mask: float = 1, cost_dice: float = 1, num_points: int = 0):
        super().__init__()
        self.cost_class = cost_class
        self.cost_mask = cost_mask
        self.cost_dice = cost_dice
        assert cost_class != 0 or cost_mask != 0 or cost_dice != 0, "all costs cant be 0"
        self.num_points = num_points
        self.last_status = None         # [S,B] int32 on the device after a call (0 = solved)

    def _pack_targets(self, targets, device):
        """-> (tmask uint8 [sum T,H,W], tstart int32 [B+1], labels int32 [sum T], counts) on `device`. An M2FTargets
        (m2f_targets.prepare_targets) on that device already holds the pack: it is returned as it is, nothing is copied."""
        packed = getattr(targets, "packed", None)
        if isinstance(targets, M2FTargets) and packed is not None:
            have, want = packed[0].device, torch.device(device)
            if have.type == want.type and (want.index is None or want.index == have.index):
                return packed
        counts = [int(t["labels"].shape[0]) for t in targets]
        sizes = {tuple(t["masks"].shape[-2:]) for t in targets}
        if len(sizes) != 1:
            raise ValueError(f"the target masks of a batch share one (padded) size, got {sorted(sizes)}")
        for t, n in zip(targets, counts):
            if t["masks"].shape[0] != n:
                raise ValueError(f"{t['masks'].shape[0]} target masks for {n} labels")
        tmask = torch.cat([t["masks"].to(device=device).to(torch.uint8) for t in targets])
        labels = torch.cat([t["labels"].to(device=device).to(torch.int32) for t in targets])
        starts = [0]
        for n in counts:
            starts.append(starts[-1] + n)
        tstart = torch.tensor(starts, dtype=torch.int32)
        if torch.device(device).type == "cuda":                # pinned + non_blocking: the copy does not stall the host
            tstart = tstart.pin_memory().to(device, non_blocking=True)
        return tmask, tstart, labels, counts

    @torch.no_grad()
    def match_steps(self, outputs_list, targets, *, point_coords=None, device_only=False, packed=None):
        """The matching of S prediction steps (a list of {"pred_logits" [B,Q,C+1], "pred_masks" [B,Q,h,w]} dicts, or one output
        dict, taken with its "aux_outputs": the last output first) against the same targets in ONE call: two launches and one
        device-to-host copy. A step may give "pred_masks_pixel_major" [B,h,w,ldq] (the decoder's own layout) instead of
        "pred_masks". Returns a list over steps of forward()'s per-image pair lists; with device_only=True the [S,B,Tmax] int32
        table (the query of target m, -1 in the padding) with no host synchronisation (self.last_status holds the status).

        point_coords [S,B,P,2], (x, y) in [0,1): the sampled points. None draws them with one torch.rand((S,B,P,2)): the
        reference's distribution, NOT its draw order (it calls torch.rand(1,P,2) once per image, matcher.py:120), so the same
        seed gives other points than the reference's. packed: the result of _pack_targets(targets, device), for a caller that
        needs the packed targets itself (SetCriterion) and should not pack them twice."""
        steps = _steps_of(outputs_list)
        S = len(steps)
        B, Q = steps[0]["pred_logits"].shape[:2]
        if len(targets) != B:
            raise ValueError(f"{len(targets)} targets for a batch of {B}")
        counts = [int(t["labels"].shape[0]) for t in targets]
        if Q > MAX_QUERIES or max(counts) > Q or S > MAX_STEPS:
            raise NotImplementedError(f"HungarianMatcher on HIP takes T_b <= Q <= {MAX_QUERIES} and at most {MAX_STEPS} steps "
                                      f"(Q {Q}, T {counts}, S {S})")
        pixel_major = "pred_masks" not in steps[0]
        masks = [o["pred_masks_pixel_major" if pixel_major else "pred_masks"] for o in steps]
        logits = [o["pred_logits"] for o in steps]
        if not all(t.is_cuda for t in masks + logits):
            raise RuntimeError("HungarianMatcher runs on an MI355X only (CUDA tensors); there is no CPU path")
        dev = logits[0].device
        if point_coords is None:
            if self.num_points < 1:
                raise ValueError("num_points must be positive to draw points")
            point_coords = torch.rand((S, B, self.num_points, 2), device=dev)
        tmask, tstart, labels, counts = self._pack_targets(targets, dev) if packed is None else packed
        _, match, status, buf = K.m2f_match_cost([m.float() for m in masks], [c.float() for c in logits], tmask, tstart, labels,
                                                 point_coords.to(device=dev, dtype=torch.float32),
                                                 (self.cost_class, self.cost_mask, self.cost_dice), Tmax=max(counts),
                                                 pixel_major=pixel_major, solve=True)
        self.last_status = status
        if device_only:
            return match
        host = buf.cpu()                                      # the one copy: match table and status together
        Tmax = match.shape[2]
        bad = host[S * B * Tmax:].view(S, B).nonzero()
        if bad.numel():
            raise ValueError(f"cost matrix is infeasible or contains invalid numeric entries (step, image) {bad.tolist()}")
        return pairs_from_table(host[:S * B * Tmax].view(S, B, Tmax), counts)

    @torch.no_grad()
    def forward(self, outputs, targets, *, point_coords=None):
        """Performs the matching (matcher.py:158-179) of outputs["pred_logits"] [B,Q,C+1] / outputs["pred_masks"] [B,Q,h,w]
        against targets[b]["labels"] [T_b] / targets[b]["masks"] [T_b,H,W] (bool, uint8 or float 0/1). Returns a list over the
        batch of (index_i, index_j) int64 CPU tensors: the selected predictions in ascending order and the targets matched to
        them, len = min(Q, T_b) (T_b = 0: two empty tensors). NotImplementedError for T_b > Q or Q > 128; ValueError where scipy
        raises one (an infeasible or non-finite cost). point_coords [B,P,2] or [1,B,P,2] injects the points; see match_steps."""
        if point_coords is not None and point_coords.dim() == 3:
            point_coords = point_coords[None]
        one = {k: v for k, v in outputs.items() if k != "aux_outputs"}
        return self.match_steps([one], targets, point_coords=point_coords)[0]

    def __repr__(self, _repr_indent=4):
        pad = " " * _repr_indent
        return "\n".join([f"Matcher {type(self).__name__}"]
                         + [f"{pad}{k}: {getattr(self, k)}" for k in ("cost_class", "cost_mask", "cost_dice")])
