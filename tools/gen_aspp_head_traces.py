"""Pin what the DeepLab head launches and computes on every ASPP route: for a table of configurations (stage-2 / stage-1 steps at
2 x 3 x 592 x 600 with the reference fixture's masks and permutations, eval forwards at 1 x 3 x 592 x 600, each under a setting of the
ASPP switches), record the full launch trace [(kind, tag, flops)] of kernels.ConvProfile and a SHA-256 of every result tensor's
bytes: score, logit, the loss as a float hex string, every gradient, every running_* buffer. Needs a GPU.

    python tools/gen_aspp_head_traces.py tests/golden/aspp_head_traces_parent.json

Every configuration runs twice in fresh models; a hash is recorded only where both runs agree, and a tensor whose two runs differ is
listed under "unstable" without one. tests/test_gpu_aspp_head_traces.py runs the same table (run_case) on a later tree and compares
row for row and hash for hash. Uses only DeepWV3Plus, trainer.TrainStep, kernels.ConvProfile / set_conv_profile / set_gemm_route,
synth, the fixture and the environment switches. Regenerate only at a commit whose head is the intended reference."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIXTURE = "deepwv3plus_train_step_2x592x600"
SWITCHES = ["MSS_ASPP_COMPOSE", "MSS_ASPP_DROPOUT_COMPACT", "MSS_WINO_ASPP3", "MSS_WINO_PAIR", "MSS_WINOGRAD"]
# name -> (mode, environment, GEMM route)
CASES = [
    ("stage2", "stage2", {}, None),
    ("stage2_dense", "stage2", {"MSS_ASPP_DROPOUT_COMPACT": "0"}, None),
    ("stage2_present", "stage2", {"MSS_ASPP_COMPOSE": "0"}, None),
    ("stage2_separate", "stage2", {"MSS_WINO_ASPP3": "0"}, None),
    ("stage2_separate_dense", "stage2", {"MSS_WINO_ASPP3": "0", "MSS_ASPP_DROPOUT_COMPACT": "0"}, None),
    ("stage2_separate_present", "stage2", {"MSS_WINO_ASPP3": "0", "MSS_ASPP_COMPOSE": "0"}, None),
    ("stage2_direct", "stage2", {"MSS_WINOGRAD": "0"}, None),
    ("stage2_bf16x3", "stage2", {}, "bf16x3"),
    ("stage1", "stage1", {}, None),
    ("eval", "eval", {}, None),
    ("eval_no_pair", "eval", {"MSS_WINO_PAIR": "0"}, None),
    ("eval_present", "eval", {"MSS_ASPP_COMPOSE": "0"}, None),
]


def load_inputs():
    import numpy as np
    import torch
    from multishiftseg_amd import synth
    g = np.load(os.path.join(ROOT, "tests", "golden", FIXTURE + ".npz"), allow_pickle=False)
    pairs, h, w = (int(v) for v in g["shape"])
    assert (pairs, h, w) == (1, 592, 600)
    params = synth.deepwv3plus_params(0)
    return dict(params={k: torch.from_numpy(np.asarray(v)) for k, v in params.items()},
                img=torch.from_numpy(synth.synth_image(int(g["image_seed"]), 2 * pairs, h, w)).cuda(),
                target=torch.from_numpy(g["target"].astype(np.int64)).cuda(),
                masks={"mod6": torch.from_numpy(g["stage2_drop_mod6"]), "mod7": torch.from_numpy(g["stage2_drop_mod7"])},
                perms=[torch.from_numpy(g[f"stage2_perm{i}"].astype(np.int64)) for i in range(3)])


def _plain(v):
    """A profiling tag as JSON holds it: tuples become lists."""
    if isinstance(v, (tuple, list)):
        return [_plain(e) for e in v]
    return v


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def run_case(case, inputs):
    """One fresh model, one step (or one eval forward) under the case's switches -> (trace, {tensor name: sha256 or loss hex})."""
    import torch
    from multishiftseg_amd import _lib, kernels as K
    from multishiftseg_amd.deepv3 import DeepWV3Plus
    from multishiftseg_amd.loss import RelContrastiveLoss
    from multishiftseg_amd.trainer import LOSS_PARAMS, TrainStep
    _name, mode, env, route = case
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    _lib.reset_env_cache()
    K.set_gemm_route(route)
    prof = K.ConvProfile()
    try:
        m = DeepWV3Plus(19)
        m.load_state_dict(inputs["params"], strict=True)
        m = m.cuda()
        m.uncertainty_func_init()
        res = {}
        if mode == "eval":
            m.eval()
            K.set_conv_profile(prof)
            with torch.no_grad():
                score, logit = m(inputs["img"][:1])
        else:
            step = TrainStep(m, RelContrastiveLoss(LOSS_PARAMS), stage=int(mode[-1]))
            step.keep_outputs = True
            m.dropout_masks = inputs["masks"]
            K.set_conv_profile(prof)
            loss = step(inputs["img"], inputs["target"].clone(), perms=inputs["perms"])
            score, logit = step.last_outputs
            res["loss"] = float(loss).hex()
            for n, p in m.named_parameters():
                if p.requires_grad:
                    res["grad:" + n] = _sha(p.grad)
        rows = prof.per_launch()
        trace = [[kind, _plain(tag), flops] for (kind, tag, _ms, _tf), (_k, flops, _s, _e) in zip(rows, prof.records)]
        res["score"] = _sha(score)
        if logit is not None:
            res["logit"] = _sha(logit)
        for k, v in m.state_dict().items():
            if "running_" in k:
                res["buffer:" + k] = _sha(v)
        return trace, res
    finally:
        K.set_conv_profile(None)
        K.set_gemm_route(None)
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
        _lib.reset_env_cache()


def main():
    inputs = load_inputs()
    doc = {}
    for case in CASES:
        (t1, r1), (t2, r2) = run_case(case, inputs), run_case(case, inputs)
        assert t1 == t2 and set(r1) == set(r2), case[0]
        unstable = sorted(k for k in r1 if r1[k] != r2[k])
        doc[case[0]] = dict(env=case[2], route=case[3], trace=t1, hashes={k: v for k, v in r1.items() if k not in unstable},
                            unstable=unstable)
        print(f"{case[0]}: {len(t1)} launches, {len(r1)} results, unstable: {unstable}", flush=True)
    with open(sys.argv[1], "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in doc.items()) + "\n}\n")


if __name__ == "__main__":
    main()
