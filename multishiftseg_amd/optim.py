"""Adam with L2-coupled weight decay as one HIP kernel per parameter (mss_adam_step_f32):
the arithmetic of torch.optim.Adam(params, lr, weight_decay) that train_deeplab.py:134-149 builds
(not AdamW; rebuilt from scratch, state included, at the stage switch train_deeplab.py:151-166).

AdamW is the optimizer of Mask2Former's stage 2 (train_m2f.py:211-299): torch.optim.AdamW with one parameter group per tensor
inside FullModelGradientClippingOptimizer, i.e. clip_grad_norm_(all parameters, max_norm) before every step. Here both are ONE
call of mss_adamw_clip_step_f32 (csrc/m2f_optim.hip) over the whole tensor list: the launches of the norm, one single-workgroup
launch for the clip coefficient, the launches of the update; no host synchronisation, no device-to-host copy, two runs give the
same bits. Deviation from torch, deliberate: the clipped gradient g * coef is formed in registers and p.grad keeps the
unclipped values (clip_grad_norm_ scales p.grad in place); nothing in the stage-2 step reads p.grad after the optimizer."""
import ctypes

import torch

from ._lib import call, ptr, value


class Adam:
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.params = [p for p in params]
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.state = {}
        self.step_count = 0

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    @torch.no_grad()
    def step(self):
        self.step_count += 1
        for p in self.params:
            if p.grad is None:
                continue
            st = self.state.get(id(p))
            if st is None:
                st = self.state[id(p)] = (torch.zeros_like(p), torch.zeros_like(p))
            g = p.grad.contiguous()
            call("mss_adam_step_f32", ptr(p), ptr(g), ptr(st[0]), ptr(st[1]), p.numel(), float(self.lr),
                 float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay),
                 self.step_count)
            torch.autograd.graph.increment_version(p)   # packed-weight caches key on tensor._version


def adamw_plan(numels):
    """The launch plan of mss_adamw_clip_step_f32 for a list of element counts, from the library's own planner (host only):
    a list of (launch, block, tensor, chunk, slot), one entry per workgroup in issue order."""
    n = len(numels)
    sizes = (ctypes.c_longlong * max(n, 1))(*[int(v) for v in numels])
    entries = value("mss_adamw_plan", n, sizes, 0, None, None, None, None, None)
    if entries < 0:
        raise ValueError("mss_adamw_plan: bad tensor list")
    cap = max(int(entries), 1)
    launch, block, tensor, slot = ((ctypes.c_int * cap)() for _ in range(4))
    chunk = (ctypes.c_longlong * cap)()
    value("mss_adamw_plan", n, sizes, entries, launch, block, tensor, chunk, slot)
    return [(launch[i], block[i], tensor[i], chunk[i], slot[i]) for i in range(entries)]


def adamw_launches(numels, clip):
    """Kernel launches one step issues for this list: L for the update, plus L + 1 for the norm and the coefficient with clipping."""
    plan = adamw_plan(numels)
    if not plan:
        return 0
    per_stage = plan[-1][0] + 1
    return 2 * per_stage + 1 if clip else per_stage


class AdamW:
    """torch.optim.AdamW(groups, lr, betas, eps, weight_decay) preceded by clip_grad_norm_(all params, max_norm) (max_norm None:
    no clipping). `params` is a list of tensors or of {"params": [...], "lr": ..., "weight_decay": ...} dicts; param_groups'
    lr / weight_decay are read on every step. state[id(p)] = (exp_avg, exp_avg_sq), step_counts[id(p)] = that parameter's own
    count: a parameter whose grad is None is skipped, it does not enter the norm and neither its count nor its moments advance."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None):
        params = list(params)
        if params and not isinstance(params[0], dict):
            params = [{"params": params}]
        self.param_groups = []
        seen = set()
        for group in params:
            g = dict(group)
            g["params"] = [g["params"]] if isinstance(g["params"], torch.Tensor) else list(g["params"])
            g.setdefault("lr", lr)
            g.setdefault("weight_decay", weight_decay)
            for p in g["params"]:
                if id(p) in seen:
                    raise ValueError("some parameters appear in more than one parameter group")
                seen.add(id(p))
            self.param_groups.append(g)
        self.betas, self.eps, self.max_norm = betas, eps, max_norm
        self.state = {}
        self.step_counts = {}
        self._scratch = None                # float32 [chunks of the list]: the norm's partial sums, every slot written before it is read
        self.last_launches = 0

    @property
    def params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    @torch.no_grad()
    def step(self):
        ps, gs, lrs, wds = [], [], [], []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                    raise RuntimeError("optim.AdamW updates contiguous float32 CUDA parameters only; there is no CPU path")
                if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape:
                    raise RuntimeError(f"optim.AdamW: a gradient must be float32, on its parameter's device and of its shape, got "
                                       f"{g.dtype} on {g.device} of shape {tuple(g.shape)}")
                ps.append(p)
                gs.append(g.contiguous())
                lrs.append(float(group["lr"]))
                wds.append(float(group["weight_decay"]))
        clip = self.max_norm is not None
        n = len(ps)
        if n == 0:
            self.last_launches = 0
            return torch.zeros((), device=self.params[0].device) if clip and self.params else None
        dev = ps[0].device
        steps = []
        for p in ps:
            if id(p) not in self.state:
                self.state[id(p)] = (torch.zeros_like(p), torch.zeros_like(p))
                self.step_counts[id(p)] = 0
            steps.append(self.step_counts[id(p)] + 1)
        numel = (ctypes.c_longlong * n)(*[p.numel() for p in ps])
        scratch = norm = None
        slots = 0
        if clip:
            slots = value("mss_adamw_scratch_floats", n, numel)
            if self._scratch is None or self._scratch.numel() < slots or self._scratch.device != dev:
                self._scratch = torch.empty(max(slots, 1), dtype=torch.float32, device=dev)
            scratch = self._scratch
            # (total_norm, coefficient): fresh every step, the caller keeps [0]; a list of empty tensors launches nothing: norm 0
            norm = torch.empty(2, dtype=torch.float32, device=dev) if slots else torch.zeros(2, dtype=torch.float32, device=dev)
        voidp = ctypes.c_void_p * n
        launches = ctypes.c_int(0)
        call("mss_adamw_clip_step_f32", n, voidp(*[p.data_ptr() for p in ps]), voidp(*[g.data_ptr() for g in gs]),
             voidp(*[self.state[id(p)][0].data_ptr() for p in ps]), voidp(*[self.state[id(p)][1].data_ptr() for p in ps]), numel,
             (ctypes.c_double * n)(*lrs), (ctypes.c_double * n)(*wds), (ctypes.c_int * n)(*steps), float(self.betas[0]),
             float(self.betas[1]), float(self.eps), int(clip), float(self.max_norm) if clip else 0.0, ptr(scratch),
             scratch.numel() if clip else 0, ptr(norm), ctypes.byref(launches))
        self.last_launches = launches.value
        for p in ps:                                    # counted once the call has been issued: a call that raises advances nothing
            self.step_counts[id(p)] += 1
            torch.autograd.graph.increment_version(p)   # packed-weight caches key on tensor._version
        return norm[0] if clip else None
