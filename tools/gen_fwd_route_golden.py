"""Pin the public answer of the forward routing: for a table of calls and MSS_GEMM* switch settings, record what
mss_conv2d_forward_route returns. The query launches nothing and dereferences no pointer, so this runs without a GPU; the pointer
fields are fake non-null integers with the stated alignment.

    python tools/gen_fwd_route_golden.py tests/golden/fwd_route_parent.json

tests/test_fwd_route_cpu.py compares a later library with the file and feeds the same rows to tests/fwd_route_check.cpp. The file
in the tree holds the answers of the last commit whose mss_conv2d_forward_route had conditions of its own (MSS_LIB pointed at a
build of it). Regenerate only at a commit whose routing is the intended reference. Every row is a call the launch accepts."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# one row = a name, these integers, then "code" (the recorded answer)
COLUMNS = ["N", "H", "W", "C", "ldx", "K", "Kpad", "ldy", "R", "stride", "dil", "batch", "x_bs", "w_bs", "affine", "in_ss_stride",
           "epilogue", "res", "stats", "w_split", "y_off", "k_steps", "k_imgs", "k_base", "w_img_stride", "env"]
# H x W: the INPUT grid (stride -2: dz's). pad = dil * (R // 2). affine: 0 none, 1 in_scale + in_shift + in_relu, 2 in_relu alone.
# epilogue: 0 none, 1 out_scale + out_shift + out_relu. res / w_split: 0 null, 1 set and 16-byte aligned, 2 set and 4 bytes off.
# y_off: bytes added to y. x_bs / w_bs: 0 = dense (rows * ldx, Kpad * C) where batch > 1. k_steps: 1 = set.
ENVS = [{}, {"MSS_GEMM": "0"}, {"MSS_GEMM_VARIANT": "2"}, {"MSS_GEMM_TAIL": "0"}, {"MSS_GEMM_TAIL": "1"}, {"MSS_GEMM_SPLIT_MFMA": "32"}]
SWITCHES = [("MSS_GEMM", 1), ("MSS_GEMM_VARIANT", 3), ("MSS_GEMM_TAIL", -1), ("MSS_GEMM_SPLIT_MFMA", 16)]
# the rows whose answer the single decision corrects: the 128 x 64 tile with an operand beyond 32-bit offsets runs conv_igemm_kernel (0)
OVER_SPAN_BN64 = ["bn64_x_span_over", "bn64_w_span_over"]


def kpad(K):
    return 64 if K <= 64 else (K + 127) // 128 * 128


def row(name, N, H, W, C, K, ldx=None, Kpad=None, ldy=None, R=1, stride=1, dil=1, batch=1, x_bs=0, w_bs=0, affine=0, in_ss_stride=0,
        epilogue=0, res=0, stats=0, w_split=0, y_off=0, k_steps=0, k_imgs=0, k_base=0, w_img_stride=0, env=0):
    return dict(name=name, N=N, H=H, W=W, C=C, ldx=C if ldx is None else ldx, K=K, Kpad=kpad(K) if Kpad is None else Kpad,
                ldy=K if ldy is None else ldy, R=R, stride=stride, dil=dil, batch=batch, x_bs=x_bs, w_bs=w_bs, affine=affine,
                in_ss_stride=in_ss_stride, epilogue=epilogue, res=res, stats=stats, w_split=w_split, y_off=y_off, k_steps=k_steps,
                k_imgs=k_imgs, k_base=k_base, w_img_stride=w_img_stride, env=env)


def gemm(name, M, C, K, **kw):
    """a 1x1 product over M rows: one image of 1 x M pixels"""
    return row(name, 1, 1, M, C, K, **kw)


def out_size(c):
    """(OH, OW, pad) of a row"""
    R, stride, dil = c["R"], c["stride"], c["dil"]
    pad = dil * (R // 2)
    if stride == -2:                                        # the caller's: an even size the strided forward maps to H x W
        return 2 * c["H"], 2 * c["W"], pad
    return (c["H"] + 2 * pad - dil * (R - 1) - 1) // stride + 1, (c["W"] + 2 * pad - dil * (R - 1) - 1) // stride + 1, pad


def workload():
    out = []
    # DeepLab (WideResNet-38 trunk at 1/8 resolution, ASPP, decoder, heads) at 1 x 512 x 1024 and 16 x 768 x 768
    for tag, N, h, w in (("1x512x1024", 1, 64, 128), ("16x768x768", 16, 96, 96)):
        out += [row(f"dl_{tag}_mod1_3x3", N, 8 * h, 8 * w, 16, 64, R=3),
                row(f"dl_{tag}_mod2_3x3", N, 4 * h, 4 * w, 64, 128, R=3, affine=1),
                row(f"dl_{tag}_mod3_3x3_s1", N, 2 * h, 2 * w, 128, 256, R=3, affine=1),
                row(f"dl_{tag}_mod4_3x3", N, h, w, 256, 512, R=3, affine=1),
                row(f"dl_{tag}_mod5_3x3_d2", N, h, w, 512, 1024, R=3, dil=2, affine=1),
                row(f"dl_{tag}_mod6_1x1_a", N, h, w, 1024, 512, affine=1),
                row(f"dl_{tag}_mod6_3x3_d4", N, h, w, 512, 1024, R=3, dil=4, affine=1),
                row(f"dl_{tag}_mod6_1x1_b", N, h, w, 1024, 2048, affine=1, in_ss_stride=1024, res=1),
                row(f"dl_{tag}_mod7_1x1_a", N, h, w, 2048, 1024, affine=1),
                row(f"dl_{tag}_mod7_1x1_b", N, h, w, 2048, 4096, affine=1, in_ss_stride=2048, stats=1),
                row(f"dl_{tag}_aspp_1x1", N, h, w, 4096, 256, affine=1),
                row(f"dl_{tag}_aspp_3x3_d12", N, h, w, 4096, 256, R=3, dil=12, affine=1),
                row(f"dl_{tag}_aspp_pool", 1, 1, N, 4096, 256),
                row(f"dl_{tag}_bot_aspp", N, h, w, 1280, 256, affine=1),
                row(f"dl_{tag}_bot_fine", N, 4 * h, 4 * w, 128, 48, affine=1),
                row(f"dl_{tag}_final_3x3", N, 4 * h, 4 * w, 304, 256, R=3, ldx=304),
                row(f"dl_{tag}_final_1x1", N, 4 * h, 4 * w, 256, 19, affine=1)]
    out += [row("dl_16x700x700_mod7_1x1_b", 16, 88, 88, 2048, 4096, affine=1, in_ss_stride=2048),        # 7744 pixels: tiles straddle images
            row("dl_16x700x700_mod7_1x1_b_split", 16, 88, 88, 2048, 4096, affine=1, in_ss_stride=2048, w_split=1)]
    # Winograd-domain batches: F(2x2) 16, F(4x4) 36, F(6x6) 64 positions of [tiles x C] x [C x K]
    for name, P, T, C, K in (("f2_mod2", 16, 32768, 64, 128), ("f4_mod4", 36, 16384, 256, 256), ("f4_mod4b", 36, 4096, 512, 512),
                             ("f6_mod4", 64, 1892, 512, 512), ("f6_mod5", 64, 2112, 512, 1024), ("f6_aspp", 64, 2304, 4096, 256),
                             ("f4_aspp", 36, 5184, 4096, 256), ("f6_final", 64, 29412, 256, 256), ("f6_final_dgrad_tail", 64, 29412, 256, 48),
                             ("f6_final_dgrad", 64, 29412, 256, 304)):
        for ws in (0, 1):
            out.append(gemm(f"wino_{name}" + ("_split" if ws else ""), T, C, K, batch=P, w_split=ws))
    for e in (3, 4):
        out.append(gemm(f"wino_f6_mod4_env{e}", 1892, 512, 512, batch=64, env=e))
    # the composed ASPP head's compose / project products
    out += [gemm("aspp_compose", 7168, 4096, 4096), gemm("aspp_project", 4603, 256, 4096), gemm("aspp_compose_tail0", 7168, 4096, 4096, env=3),
            gemm("aspp_compose_split", 7168, 4096, 4096, w_split=1)]
    # dropped-channel products: the one-batch form (images of 64 x 128 / 96 x 96 pixels) and the Winograd-domain k_imgs form
    out += [row("dropped_mod6", 2, 96, 96, 1024, 2048, k_steps=1, w_img_stride=2048 * 1024),
            row("dropped_mod7", 16, 96, 96, 2048, 4096, k_steps=1, w_img_stride=4096 * 2048),
            row("dropped_mod7_nogemm", 2, 64, 128, 2048, 4096, k_steps=1, w_img_stride=4096 * 2048, env=1),
            gemm("dropped_f6_aspp", 2592, 4096, 256, batch=72, k_steps=1, k_imgs=2, k_base=8),
            gemm("dropped_f4_aspp", 1152, 4096, 256, batch=128, k_steps=1, k_imgs=2, k_base=8),
            gemm("dropped_k_imgs_wide", 2048, 256, 256, batch=64, k_steps=1, k_imgs=2, k_base=3)]
    # the pixel decoder's Linears over 16 x 10 164 tokens, one image, and the mask-logits product
    for name, M in (("16img", 162624), ("1img", 10164)):
        for C, K in ((256, 256), (1024, 256), (256, 1024), (256, 288), (256, 32), (256, 96)):
            out.append(gemm(f"dec_{name}_{C}to{K}", M, C, K, epilogue=1))
            out.append(gemm(f"dec_{name}_{C}to{K}_split", M, C, K, epilogue=1, w_split=1))
    out += [row("mask_logits", 2, 1, 128 * 256, 256, 100), row("mask_logits_split", 2, 1, 128 * 256, 256, 100, w_split=1)]
    # the ResNet-50 backbone at 2 x 512 x 1024: stem, bottleneck 1x1 / 3x3, strided 3x3 and shortcuts, and the stride-2 data gradients
    out += [row("r50_stem", 2, 512, 1024, 4, 64, R=7, stride=2, dil=1, epilogue=1), row("r50_stem_odd", 1, 65, 131, 4, 64, R=7, stride=2, epilogue=1)]
    for name, h, cin, mid in (("res2", 128, 64, 64), ("res3", 64, 256, 128), ("res4", 32, 512, 256), ("res5", 16, 1024, 512)):
        s = 1 if name == "res2" else 2
        out += [row(f"r50_{name}_conv1", 2, h * s, 2 * h * s, cin, mid, epilogue=1),
                row(f"r50_{name}_conv2", 2, h * s, 2 * h * s, mid, mid, R=3, stride=s, epilogue=1),
                row(f"r50_{name}_conv3", 2, h, 2 * h, mid, 4 * mid, epilogue=1, res=1),
                row(f"r50_{name}_shortcut", 2, h * s, 2 * h * s, cin, 4 * mid, stride=s, epilogue=1)]
        if s == 2:
            out += [row(f"r50_{name}_conv2_dgrad", 2, h, 2 * h, mid, mid, R=3, stride=-2, res=1),
                    row(f"r50_{name}_shortcut_dgrad", 2, h, 2 * h, 4 * mid, cin, stride=-2),
                    row(f"r50_{name}_conv2_dgrad_split", 2, h, 2 * h, mid, mid, R=3, stride=-2, w_split=1)]
    out.append(row("dgrad_s2_k48", 1, 32, 32, 64, 48, R=3, stride=-2, affine=1))
    return out


def boundaries():
    out = []
    for K in (31, 32, 33, 64, 65):
        for M in (16383, 16384):
            out.append(gemm(f"K{K}_M{M}", M, 256, K))
        out.append(gemm(f"K{K}_batched", 16384, 256, K, batch=4))
        out.append(gemm(f"K{K}_split", 16384, 256, K, w_split=1))
        out.append(gemm(f"K{K}_nogemm", 16384, 256, K, env=1))
    for C in (16, 32, 48):                                   # C / BK = 1, 2, 3
        for K in (48, 128):
            for ws in (0, 1):
                out.append(gemm(f"C{C}_K{K}" + ("_split" if ws else ""), 16384, C, K, w_split=ws))
        out.append(gemm(f"C{C}_K128_variant2", 16384, C, 128, env=2))
        out.append(row(f"C{C}_3x3_split", 1, 64, 64, C, 128, R=3, w_split=1))
    for hw, tag in ((128, "whole"), (100, "straddle")):      # per-sample affine with (OH * OW) % 128 zero / non-zero
        for ws in (0, 1):
            for K in (48, 256):
                out.append(row(f"per_sample_{tag}_K{K}" + ("_split" if ws else ""), 200, 1, hw, 256, K, affine=1, in_ss_stride=256, w_split=ws))
        out.append(row(f"per_sample_{tag}_3x3", 4, 10, hw // 2, 64, 128, R=3, affine=1, in_ss_stride=64))
        out.append(row(f"per_sample_{tag}_3x3_k48", 4, 10, hw // 2, 64, 48, R=3, affine=1, in_ss_stride=64))
    out += [gemm("relu_only", 4096, 256, 128, affine=2), gemm("few_rows_8", 8, 4096, 256), gemm("few_rows_9", 9, 4096, 256),
            gemm("few_rows_16", 16, 4096, 256), gemm("few_rows_32", 32, 4096, 256), gemm("few_rows_33", 33, 4096, 256),
            gemm("few_rows_epilogue", 16, 4096, 256, epilogue=1), gemm("few_rows_nogemm", 16, 4096, 256, env=1)]
    # spans just under / over each 32-bit limit (nothing is touched: the pointers are fake). x: rows * ldx * 4 bytes with ldx = 1024;
    # w: batch entries w_bs apart
    under, over = (1 << 20) - 1, 1 << 20
    for tag, M in (("under", under), ("over", over)):
        out += [gemm(f"v3_x_span_{tag}", M, 256, 256, ldx=1024), gemm(f"bn64_x_span_{tag}", M, 256, 48, ldx=1024),
                gemm(f"split_x_span_{tag}", M, 256, 256, ldx=1024, w_split=1),
                row(f"rowaff_x_span_{tag}", 10485 if tag == "under" else 10486, 1, 100, 256, 256, ldx=1024, affine=1, in_ss_stride=256, w_split=1),
                row(f"split_conv_x_span_{tag}", 1, 512, M // 1024, 256, 128, ldx=1024, R=3, w_split=1)]      # signed offsets: 2^31 bytes
    for tag, d in (("under", 4), ("over", 0)):               # (w_bs + Kpad * C) * 4 bytes around 2^32
        out += [gemm(f"v3_w_span_{tag}", 4096, 256, 256, batch=2, w_bs=(1 << 30) - 256 * 256 - d),
                gemm(f"bn64_w_span_{tag}", 16384, 256, 48, batch=2, w_bs=(1 << 30) - 64 * 256 - d)]
    for tag, Kpad in (("under", 43648), ("over", 43776)):    # Kpad * 16384 * 6 bytes around 2^32
        out += [gemm(f"split_w_span_{tag}", 4096, 16384, 256, Kpad=Kpad, w_split=1),
                row(f"rowaff_w_span_{tag}", 8, 1, 100, 16384, 256, Kpad=Kpad, affine=1, in_ss_stride=16384, w_split=1)]
    for tag, Kpad in (("under", 4736), ("over", 4864)):      # 9 taps * Kpad * 16384 * 6 bytes
        out.append(row(f"split_conv_w_span_{tag}", 1, 32, 32, 16384, 256, Kpad=Kpad, R=3, w_split=1))
    out += [gemm("perimg_x_span_under", (1 << 20) - 128, 256, 256, ldx=1024, k_steps=1), gemm("split_batched_w_bs", 4096, 256, 256, batch=4, w_bs=256 * 256 + 64, w_split=1)]
    # wide tiles of a 256-channel output: mtiles at every threshold of the rounds, one position and batched, all three width rules
    for t in (511, 512, 513, 896, 897, 1023, 1024, 1025, 1152, 1271, 2304):
        for e in (0, 3, 4):
            out.append(gemm(f"tiles256_{t}_env{e}", t * 128, 256, 256, env=e))
        out += [gemm(f"tiles256_{t}_c128", t * 128, 128, 256), gemm(f"tiles256_{t}_affine_v2", t * 128, 256, 256, affine=1, env=2),
                gemm(f"tiles256_{t}_split", t * 128, 256, 256, w_split=1), gemm(f"tiles256_{t}_split_affine", t * 128, 256, 256, w_split=1, affine=1),
                gemm(f"tiles256_{t}_split_mfma32", t * 128, 256, 256, w_split=1, env=5),
                row(f"tiles256_{t}_perimg", t, 1, 128, 256, 256, k_steps=1, w_img_stride=256 * 256),
                row(f"tiles256_{t}_perimg_c128", t, 1, 128, 128, 256, k_steps=1, w_img_stride=256 * 128),
                gemm(f"tiles256_{t}_k_imgs", 128 * (t // 8), 256, 256, batch=8, k_steps=1, k_imgs=2, k_base=3),
                row(f"tiles256_{t}_split_conv", 1, t, 128, 16, 256, R=3, w_split=1), row(f"tiles256_{t}_split_conv_affine", 1, t, 128, 16, 256, R=3, w_split=1, affine=1),
                row(f"tiles256_{t}_split_conv_s2", 1, 2 * t, 256, 64, 256, stride=2, w_split=1)]
    out += [gemm("tiles256_batched_1920", 1920 // 2 // 64 * 128, 512, 512, batch=64), gemm("tiles256_batched_1920_tail1", 1920 // 2 // 64 * 128, 512, 512, batch=64, env=4)]
    # misaligned w_split / y / res: the split route only where its 16-byte accesses hold
    for ws, y_off, res in ((2, 0, 0), (1, 4, 0), (1, 0, 2), (1, 0, 1), (2, 4, 2)):
        out.append(gemm(f"misaligned_ws{ws}_y{y_off}_res{res}", 16384, 256, 256, w_split=ws, y_off=y_off, res=res))
        out.append(row(f"misaligned_conv_ws{ws}_y{y_off}_res{res}", 1, 64, 64, 64, 128, R=3, w_split=ws, y_off=y_off, res=res))
    out += [gemm("split_mfma16_ldy", 16384, 256, 256, w_split=1, ldy=258), gemm("split_mfma16_K", 16384, 256, 130, w_split=1, ldy=132),
            gemm("split_stats", 16384, 256, 256, w_split=1, stats=1), gemm("split_epilogue", 16384, 256, 256, w_split=1, epilogue=1)]
    # the igemm tiles: 256 x 64, 128 x 128 x 32 (C % 32 == 0, C >= 2048, K <= 256), 128 x 128 x 16
    out += [row("igemm_k32_step", 1, 64, 64, 2048, 256, R=3, dil=12), row("igemm_k16_c2032", 1, 64, 64, 2032, 256, R=3), row("igemm_k16_K384", 1, 64, 64, 2048, 384, R=3),
            row("igemm_s2_1x1", 1, 64, 64, 256, 512, stride=2), row("igemm_1x3", 1, 64, 64, 64, 128, R=3, affine=1, w_split=1)]
    return out


def cases():
    rows = workload() + boundaries()
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return rows


FAKE = 0x7f0000001000                                        # 4 KiB aligned, never read


def conv_args(_lib, c, keep):
    a = _lib.MssConvArgs()
    OH, OW, pad = out_size(c)
    a.x, a.w, a.y = FAKE, FAKE + 0x100000, FAKE + 0x200000 + c["y_off"]
    if c["affine"] == 1:
        a.in_scale, a.in_shift = FAKE + 0x300000, FAKE + 0x300400
    a.in_relu = 1 if c["affine"] else 0
    a.in_ss_stride = c["in_ss_stride"]
    if c["epilogue"]:
        a.out_scale, a.out_shift, a.out_relu = FAKE + 0x400000, FAKE + 0x400400, 1
    if c["res"]:
        a.res, a.ldres = FAKE + 0x500000 + (4 if c["res"] == 2 else 0), c["ldy"]
    if c["stats"]:
        a.stats = FAKE + 0x600000
    if c["w_split"]:
        a.w_split = FAKE + 0x700000 + (4 if c["w_split"] == 2 else 0)
    if c["k_steps"]:
        a.k_steps = FAKE + 0x800000
    a.N, a.H, a.W, a.C, a.ldx = c["N"], c["H"], c["W"], c["C"], c["ldx"]
    a.OH, a.OW, a.K, a.Kpad, a.ldy = OH, OW, c["K"], c["Kpad"], c["ldy"]
    a.R = a.S = c["R"]
    a.stride, a.dil, a.pad = c["stride"], c["dil"], pad
    a.batch = c["batch"]
    if c["batch"] > 1:
        a.x_bs = c["x_bs"] or c["N"] * c["H"] * c["W"] * c["ldx"]
        a.w_bs = c["w_bs"] or c["Kpad"] * c["C"]
        a.y_bs = c["N"] * OH * OW * c["ldy"]
    a.k_imgs, a.k_base, a.w_img_stride = c["k_imgs"], c["k_base"], c["w_img_stride"]
    keep.append(a)
    return a


def answers(_lib, rows):
    """mss_conv2d_forward_route of every row on the loaded library, switching the environment as the rows ask."""
    lib = _lib.load()
    saved = {k: os.environ.pop(k, None) for k, _ in SWITCHES}
    out, keep, cur = [], [], None
    try:
        for c in rows:
            if c["env"] != cur:
                for k, _ in SWITCHES:
                    os.environ.pop(k, None)
                os.environ.update(ENVS[c["env"]])
                lib.mss_env_reset()
                cur = c["env"]
            out.append(int(lib.mss_conv2d_forward_route(ctypes.byref(conv_args(_lib, c, keep)))))
    finally:
        for k, _ in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
        lib.mss_env_reset()
    return out


def main():
    from multishiftseg_amd import _lib
    rows = cases()
    got = answers(_lib, rows)
    with open(sys.argv[1], "w") as f:
        f.write('{"columns": %s,\n "envs": %s,\n "rows": [\n' % (json.dumps(["name"] + COLUMNS + ["code"]), json.dumps(ENVS)))
        f.write(",\n".join(json.dumps([c["name"]] + [c[k] for k in COLUMNS] + [g], separators=(",", ":")) for c, g in zip(rows, got)))
        f.write("\n]}\n")
    print(len(rows), "rows;", {code: got.count(code) for code in sorted(set(got))})


if __name__ == "__main__":
    main()
