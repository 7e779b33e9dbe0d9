"""CPU: the host side of Mask2Former stage 1 -- the chunk planner of kernels.m2f_semantic_inference, the exported names, and the
promise that the feature adds no entry point: include/mss_hip.h declared 141 functions at ABI version 25 with it (142 at version 26 since mss_conv2d_wgrad_plan)."""
import inspect
import os
import re

import pytest

from conftest import ROOT
from test_abi_cpu import header_declarations


def _chunks_ok(B, Hp, Wp, ldq, budget):
    from multishiftseg_amd import kernels as K
    chunks = K.stage1_chunks(B, Hp, Wp, ldq, budget)
    per = 4 * Hp * Wp * ldq
    assert all(n >= 1 for _, n in chunks)                                        # never an empty chunk
    assert [s for s, _ in chunks] == [sum(n for _, n in chunks[:i]) for i in range(len(chunks))] and sum(n for _, n in chunks) == B
    if budget >= per:                                                            # one image fits: every chunk respects the budget
        assert all(n * per <= budget for _, n in chunks)
        assert len(chunks) == -(-B // (budget // per))                           # and no more chunks than the budget asks for
    else:
        assert chunks == [(b, 1) for b in range(B)]                              # an image alone exceeds it: one image per chunk
    return chunks


def test_chunk_planner():
    from multishiftseg_amd import kernels as K
    for B in (1, 2, 3, 7, 16):
        for Hp, Wp, ldq in ((20, 28, 8), (704, 704, 100), (1024, 2048, 100)):
            per = 4 * Hp * Wp * ldq
            for budget in (0, 1, per - 1, per, per + 1, 2 * per, 3 * per - 1, 16 * per, 1 << 40):
                _chunks_ok(B, Hp, Wp, ldq, budget)
    assert K.stage1_chunks(16, 704, 704, 100, 1 << 30) == [(0, 5), (5, 5), (10, 5), (15, 1)]       # 0.2 GB per image
    assert K.stage1_chunks(3, 20, 28, 8, 2 * 4 * 20 * 28 * 8) == [(0, 2), (2, 1)]
    with pytest.raises(ValueError):
        K.stage1_chunks(0, 20, 28, 8, 1 << 20)


def test_default_budget_comes_from_the_environment(monkeypatch):
    from multishiftseg_amd import kernels as K
    monkeypatch.delenv(K.STAGE1_BUDGET_ENV, raising=False)
    assert K.stage1_budget() == 1 << 30
    per = 4 * 704 * 704 * 100
    monkeypatch.setenv(K.STAGE1_BUDGET_ENV, str(2 * per))
    assert K.stage1_budget() == 2 * per and [n for _, n in K.stage1_chunks(5, 704, 704, 100)] == [2, 2, 1]
    assert K.STAGE1_BUDGET_ENV in open(os.path.join(ROOT, "DESIGN.md")).read()   # the switch is listed with the others


def test_exported_names():
    import multishiftseg_amd as pkg
    from multishiftseg_amd import kernels, m2f_trainer, maskformer, transformer_decoder
    for name in ("M2FStage1Step", "m2f_semantic_inference", "upsample_bilinear_nhwc", "stage1_chunks"):
        assert name in pkg.__all__, name
    assert pkg.M2FStage1Step is m2f_trainer.M2FStage1Step
    assert pkg.m2f_semantic_inference is kernels.m2f_semantic_inference and pkg.upsample_bilinear_nhwc is kernels.upsample_bilinear_nhwc
    assert pkg.stage1_chunks is kernels.stage1_chunks
    assert callable(maskformer.MaskFormer.semantic_inference) and callable(maskformer.MaskFormer.stage1_forward)
    sig = inspect.signature(kernels.m2f_semantic_inference)
    assert list(sig.parameters)[:6] == ["class_logits", "mask_logits_nhwc", "image_size", "size", "class_logits_ood", "Q"]
    assert inspect.signature(kernels.m2f_class_mix_backward).parameters["want_dmasks"].default is True
    fwd = inspect.signature(transformer_decoder.MultiScaleMaskedTransformerDecoder_GMA.forward).parameters["semantic"]
    assert fwd.kind is inspect.Parameter.KEYWORD_ONLY and fwd.default is None
    step = inspect.signature(m2f_trainer.M2FStage1Step.__init__).parameters
    assert step["lr"].default == 1e-4 and step["weight_decay"].default == 1e-4 and step["patterns"].default == ("class_embed2",)


def test_the_feature_adds_no_entry_point():
    from multishiftseg_amd import _lib
    src = open(os.path.join(ROOT, "include", "mss_hip.h")).read()
    assert len(header_declarations()) == len(_lib.SIGNATURES) == 142          # (141 when the feature landed; mss_conv2d_wgrad_plan since)
    assert int(re.search(r"#define MSS_ABI_VERSION (\d+)", src).group(1)) == _lib.MSS_ABI_VERSION == 26
    assert "lat == NULL" in src and "dmasks == NULL" in src                        # both variants are documented at their declarations
