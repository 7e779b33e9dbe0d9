"""Pin the public answers of the weight-gradient routing: for a table of shapes and MSS_WGRAD_* switch settings, record what
mss_conv2d_wgrad_workspace_bytes and mss_conv2d_wgrad_route return. Neither query launches anything or dereferences a pointer, so
this runs without a GPU; the pointer fields are fake non-null integers with the stated alignment.

    python tools/gen_wgrad_route_golden.py tests/golden/wgrad_route_parent.json

tests/test_wgrad_route_cpu.py compares a later library with the file (the route equal, the scratch never larger) and feeds the
same rows to tests/wgrad_route_check.cpp. Regenerate only at a commit whose routing is the intended reference."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# one row = these integers, then "ws" and "route" (the recorded answers)
COLUMNS = ["M", "C", "K", "Kpad", "Cp", "lddy", "ldx", "R", "stride", "dil", "batch", "affine", "in_ss_stride", "route", "k_imgs", "env"]
# affine: 0 none, 1 scale + shift + ReLU (16-byte aligned), 2 ReLU alone.  k_imgs > 0: the per-image form (k_steps set, k_base 8)
ENVS = [{}, {"MSS_WGRAD_TN": "0"}, {"MSS_WGRAD_TN": "1"}, {"MSS_WGRAD_TN": "4"}, {"MSS_WGRAD_TN": "5"}, {"MSS_WGRAD_TN": "7"},
        {"MSS_WGRAD_NARROW": "0"}, {"MSS_WGRAD_TN_AFFINE": "0"}, {"MSS_WGRAD_TN_TAIL": "0"}]
SWITCHES = ["MSS_WGRAD_TN", "MSS_WGRAD_NARROW", "MSS_WGRAD_TN_AFFINE", "MSS_WGRAD_TN_TAIL", "MSS_WGRAD_PERIMG_PACK", "MSS_WGRAD_TN_SLOTS"]


def kpad(K):
    return 64 if K <= 64 else (K + 127) // 128 * 128


def row(M, C, K, Kpad=None, Cp=None, lddy=None, ldx=None, R=1, stride=1, dil=1, batch=1, affine=0, in_ss_stride=0, route=0, k_imgs=0, env=0):
    return dict(M=M, C=C, K=K, Kpad=kpad(K) if Kpad is None else Kpad, Cp=C if Cp is None else Cp, lddy=K if lddy is None else lddy,
                ldx=C if ldx is None else ldx, R=R, stride=stride, dil=dil, batch=batch, affine=affine, in_ss_stride=in_ss_stride,
                route=route, k_imgs=k_imgs, env=env)


def cases():
    named = [row(2304, 4096, 256, batch=64), row(5184, 4096, 256, batch=36), row(29412, 256, 256, batch=64),      # Winograd-domain products
             row(162624, 256, 256), row(162624, 1024, 256), row(162624, 256, 1024), row(10164, 256, 256),           # pixel decoder Linears
             row(65536, 4096, 256), row(32768, 1280, 256, affine=1),                                                # ASPP 1x1, bot_aspp
             row(162624, 256, 288), row(162624, 256, 288, lddy=512),                                               # the merged 256 + 32 projection
             row(2592, 4096, 256, batch=72, k_imgs=2), row(1152, 4096, 256, batch=128, k_imgs=2)]                   # per-image form
    Ks = [19, 32, 33, 48, 64, 65, 128, 160, 192, 288, 304]
    Cs = [64, 128, 192, 256, 320, 4096]
    Ms = [63, 64, 511, 16383, 16384, 50001]
    out = []
    for e in range(len(ENVS)):
        for r in named:
            out.append(dict(r, env=e))
            if e == 0 and not r["k_imgs"]:
                out.append(dict(r, route=1))
    for K in Ks:                                                      # every K, C and M of the lists, not their full product
        for C in (128, 256):
            for M in (511, 16384):
                out.append(row(M, C, K))
    for C in Cs:
        for K in (64, 128):
            out.append(row(50001, C, K))
            out.append(row(50001, C, K, route=1))
    for M in Ms:
        for K in (48, 128):
            out.append(row(M, 256, K))
            out.append(row(M, 256, K, route=1))
    small = [(K, C, 16384) for K in (19, 64, 128, 160, 288) for C in (128, 256)]
    for e in range(1, len(ENVS)):
        for K, C, M in small:
            out.append(row(M, C, K, env=e))
    for K, C, M in small[1::2] + [(192, 320, 50001)]:
        K4 = (K + 3) // 4 * 4
        out.append(row(M, C, K, lddy=K + 64))                          # dy a channel slice of a wider buffer
        out.append(row(M, C, K, lddy=K + 64, route=1))
        out.append(row(M, C, K, ldx=C + 64))                           # x a channel slice
        out.append(row(M, C, K, Kpad=kpad(K) + 128, Cp=C + 4))         # padded result
        out.append(row(M, C, K, Cp=C + 128))
        for lddy in (K4, 256 if K <= 192 else 512):                   # Kpad = K rounded up to 4 (kernels.conv2d_wgrad), dense and sliced dy
            out.append(row(M, C, K, Kpad=K4, lddy=lddy))
            out.append(row(M, C, K, Kpad=K4, lddy=lddy, route=1))
        out.append(row(M, C, K, affine=1))
        out.append(row(M, C, K, affine=1, route=1))
        out.append(row(M, C, K, affine=2))
        out.append(row(M, C, K, affine=1, in_ss_stride=C))             # per-sample affine (Dropout2d fold)
        out.append(row(M, C, K, affine=1, env=7))
        out.append(row(M, C, K, R=3))                                  # 3x3, padding = dilation
        out.append(row(M, C, K, R=3, stride=2))
        out.append(row(M, C, K, R=3, dil=12))
    for Ko in (160, 192):                                             # the two-part GPU test's shapes
        for lddy in (Ko, 256):
            out.append(row(16385, 128, Ko, Kpad=Ko, lddy=lddy))
            out.append(row(16385, 128, Ko, Kpad=Ko, lddy=lddy, route=1))
    for batch in (36, 64):
        for K, C, M in ((128, 256, 600), (192, 4096, 600), (256, 320, 63), (256, 4096, 2304)):
            for e in (0, 1, 2, 3, 5, 8):
                out.append(row(M, C, K, batch=batch, env=e))
            out.append(row(M, C, K, batch=batch, route=1))
    return out


def conv_args(_lib, c, keep):
    """MssConvArgs of a case. M rows: a 1x1 product is one image of 1 x M pixels; a 3x3 one is M / 64 (rounded up) x 64 input pixels
    and M is replaced by the true output pixel count."""
    a = _lib.MssConvArgs()
    fake = 0x7f0000001000                                  # 4 KiB aligned, never read
    a.x, a.w, a.y = fake, fake + 0x100000, fake + 0x200000
    if c["affine"] == 1:
        a.in_scale, a.in_shift = fake + 0x300000, fake + 0x300400
    a.in_relu = 1 if c["affine"] else 0
    a.in_ss_stride = c["in_ss_stride"]
    R, stride, dil = c["R"], c["stride"], c["dil"]
    a.N, a.C, a.ldx, a.K, a.Kpad, a.ldy = 1, c["C"], c["ldx"], c["K"], c["Kpad"], c["lddy"]
    a.R = a.S = R
    a.stride, a.dil, a.pad = stride, dil, dil * (R // 2)
    if R == 1:
        a.H, a.W = 1, c["M"]
    else:
        a.H, a.W = -(-c["M"] // 64), 64
    a.OH, a.OW = (a.H - 1) // stride + 1, (a.W - 1) // stride + 1
    a.batch, a.route = c["batch"], c["route"]
    if c["batch"] > 1:
        a.x_bs, a.y_bs = a.H * a.W * c["C"], a.OH * a.OW * c["K"]
    if c["k_imgs"]:
        a.k_imgs, a.k_base = c["k_imgs"], 8
        a.k_steps = fake + 0x400000
    keep.append(a)
    return a


def answers(_lib, rows):
    """(workspace bytes, route) of every row on the loaded library, switching the environment as the rows ask."""
    lib = _lib.load()
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    out, keep, cur = [], [], None
    try:
        for c in rows:
            if c["env"] != cur:
                for k in SWITCHES:
                    os.environ.pop(k, None)
                os.environ.update(ENVS[c["env"]])
                lib.mss_env_reset()
                cur = c["env"]
            a = conv_args(_lib, c, keep)
            out.append((int(lib.mss_conv2d_wgrad_workspace_bytes(ctypes.byref(a), c["Cp"])), int(lib.mss_conv2d_wgrad_route(ctypes.byref(a), c["lddy"]))))
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
        lib.mss_env_reset()
    return out


def main():
    from multishiftseg_amd import _lib
    rows = cases()
    got = answers(_lib, rows)
    doc = {"columns": COLUMNS + ["ws", "route_answer"], "envs": ENVS,
           "rows": [[c[k] for k in COLUMNS] + list(g) for c, g in zip(rows, got)]}
    with open(sys.argv[1], "w") as f:
        f.write('{"columns": %s,\n "envs": %s,\n "rows": [\n' % (json.dumps(doc["columns"]), json.dumps(doc["envs"])))
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in doc["rows"]))
        f.write("\n]}\n")
    print(len(rows), "rows;", sum(1 for g in got if g[1]), "on the split-bf16 route;", sum(1 for g in got if g[0]), "with scratch")


if __name__ == "__main__":
    main()
