"""float64 numpy restatement of torch.nn.utils.clip_grad_norm_ followed by torch.optim.AdamW's single-tensor step, written from
their definitions: per-tensor lr, weight decay and step counts; a tensor whose gradient is None is skipped (it does not enter
the norm, its count and its moments do not advance). tests/test_m2f_optim_cpu.py pins it against stock torch on the CPU."""
import numpy as np


class RefAdamW:
    def __init__(self, params, lrs, wds, betas=(0.9, 0.999), eps=1e-8, max_norm=None):
        self.p = [np.asarray(a, dtype=np.float64).copy() for a in params]
        self.m = [np.zeros_like(a) for a in self.p]
        self.v = [np.zeros_like(a) for a in self.p]
        self.t = [0] * len(self.p)
        self.lrs, self.wds = [float(x) for x in lrs], [float(x) for x in wds]
        self.betas, self.eps, self.max_norm = betas, eps, max_norm
        self.last_coef = None

    def step(self, grads):
        """grads: one array or None per parameter. Returns the total norm (None without clipping)."""
        live = [i for i, g in enumerate(grads) if g is not None]
        g64 = {i: np.asarray(grads[i], dtype=np.float64) for i in live}
        norm, coef = None, 1.0
        if self.max_norm is not None:
            with np.errstate(invalid="ignore", over="ignore"):
                norm = float(np.sqrt(sum(float((g * g).sum()) for g in g64.values())))
                coef = self.max_norm / (norm + 1e-6)
            if coef > 1.0:                                   # clamp(max=1): NaN stays NaN
                coef = 1.0
        self.last_coef = coef
        b1, b2 = self.betas
        for i in live:
            with np.errstate(invalid="ignore", over="ignore"):
                g = g64[i] * coef if self.max_norm is not None else g64[i]
                self.t[i] += 1
                t = self.t[i]
                self.p[i] *= 1.0 - self.lrs[i] * self.wds[i]
                self.m[i] += (g - self.m[i]) * (1.0 - b1)
                self.v[i] = self.v[i] * b2 + (1.0 - b2) * g * g
                bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
                denom = np.sqrt(self.v[i]) / np.sqrt(bc2) + self.eps
                self.p[i] += -(self.lrs[i] / bc1) * (self.m[i] / denom)
        return norm


def torch_cpu_run(params, lrs, wds, grad_steps, betas=(0.9, 0.999), eps=1e-8, max_norm=None):
    """Stock torch in float32 on the CPU: clip_grad_norm_(foreach=False) + AdamW(foreach=False), one group per tensor.
    grad_steps: per step a list of float32 arrays / None. Returns per step (params, exp_avg, exp_avg_sq, norm) as numpy copies
    (moments None until a tensor has taken a step)."""
    import torch
    ps = [torch.nn.Parameter(torch.from_numpy(np.array(a, dtype=np.float32))) for a in params]
    opt = torch.optim.AdamW([{"params": [p], "lr": lr, "weight_decay": wd} for p, lr, wd in zip(ps, lrs, wds)], betas=betas, eps=eps,
                            foreach=False)
    out = []
    for grads in grad_steps:
        for p, g in zip(ps, grads):
            p.grad = None if g is None else torch.from_numpy(np.array(g, dtype=np.float32))
        norm = None
        if max_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False).numpy().copy()
        opt.step()
        st = [opt.state.get(p, {}) for p in ps]
        out.append(([p.detach().numpy().copy() for p in ps], [s["exp_avg"].numpy().copy() if s else None for s in st],
                    [s["exp_avg_sq"].numpy().copy() if s else None for s in st], norm))
    return out


GROUPS = [(1e-5, 0.05), (1e-4, 0.0), (1e-6, 1e-2)]      # (lr, weight decay): the reference's pair, no decay, a backbone-like pair
STEPS = 6
NONE_STEPS = (1, 3)                                      # steps 2 and 4, counted from 1: one tensor has no gradient
ZERO_STEP = 4                                            # step 5: every gradient is zero


def parity_sizes(chunk, tensors_per_launch, blocks_per_launch):
    """The size list of the parity test: the vector tail (1 .. 5), the block edges, the chunk edges, more tensors than one launch
    holds (by 3) and one tensor with more chunks than one launch has blocks."""
    head = [1, 3, 4, 5, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 5]
    sevens = [7] * (tensors_per_launch + 3 - len(head) - 1)
    return head + sevens + [blocks_per_launch * chunk + 2 * chunk + 3]


def parity_case(sizes, seed=0, clip=True):
    """Inputs of the 6-step sequence and its float64 outcome. Gradient scales as tests/test_gpu_optim.py draws them (10^U(-6,0) per
    tensor and step, 10 % exact zeros). max_norm is set from the float64 norms, at the widest gap between two of them, so that
    steps fall on both sides of it. Returns a dict: p0, grads[step][tensor] (float32 / None), lrs, wds, max_norm, ref (RefAdamW after
    the last step), norms, coefs (float64, per step), moved (per tensor: the largest single-step move of an element)."""
    rng = np.random.default_rng(seed)
    n = len(sizes)
    p0 = [(rng.standard_normal(s) * 0.05).astype(np.float32) for s in sizes]
    lrs = [GROUPS[i % 3][0] for i in range(n)]
    wds = [GROUPS[i % 3][1] for i in range(n)]
    none_tensor = min(5, n - 1)
    grads = []
    for k in range(STEPS):
        row = []
        for i, s in enumerate(sizes):
            g = (rng.standard_normal(s) * 10.0 ** rng.uniform(-6, 0)).astype(np.float32)
            g[rng.random(s) < 0.1] = 0.0
            if k == ZERO_STEP:
                g[:] = 0.0
            row.append(None if (i == none_tensor and k in NONE_STEPS) else g)
        grads.append(row)
    max_norm = None
    if clip:
        norms = sorted(float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in row if g is not None))) for row in grads)
        nz = [v for v in norms if v > 0]
        gaps = [nz[j + 1] / nz[j] for j in range(1, len(nz) - 2)]            # at least two steps above, one non-zero step below
        j = 1 + int(np.argmax(gaps))
        max_norm = float(np.sqrt(nz[j] * nz[j + 1]))
    ref = RefAdamW(p0, lrs, wds, max_norm=max_norm)
    out_norms, coefs, moved = [], [], [0.0] * n
    for row in grads:
        before = [a.copy() for a in ref.p]
        out_norms.append(ref.step(row))
        coefs.append(ref.last_coef)
        for i, g in enumerate(row):
            if g is not None:
                moved[i] = max(moved[i], float(np.abs(ref.p[i] - before[i]).max()))
    return dict(sizes=sizes, p0=p0, grads=grads, lrs=lrs, wds=wds, max_norm=max_norm, ref=ref, norms=out_norms, coefs=coefs, moved=moved,
                none_tensor=none_tensor)
