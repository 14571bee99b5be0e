"""The case table of tests/test_conv_igemm_exact_gpu.py: one entry per kernel variant and
edge of csrc/kernels/conv_igemm.hip / conv_wgrad.hip (no extension import: the CPU tier
checks every entry's exactness conditions).

A case = name, op, shape, dtype, regime (tests/_conv_ref.py), the ``*_config`` settings it
needs and ``expect``: the kernel variants it is meant to reach, as conv_igemm.last_launch()
reports them -- [(family, template arguments)], the conv kernel first, then the statistics
kernel of a deferred tree.  Shapes are non-square (a swapped OH / OW shows) and the smallest
that still reach the branch:

  fwd, fwd+stats, acc, aux, wgrad   (N, C, H, W, K, R, stride, pad)
  s2t                               (N, Cin, OH, OW, K): dy [N, K, OH, OW] -> dx [N, Cin, 2 OH, 2 OW]
  stem                              (N, H, W, K)
  dgrad_bn                          (N, K, H, W, Cc): dy [N, K, H, W] -> dx [N, Cc, H, W]; extra act, R
  wgrad_batch                       a tuple of wgrad shapes

Weight-gradient cases also carry ``splits`` = (split count, pixels per split, pixels in the
last split) they were designed for; the test recomputes them from conv_igemm.wgrad_splits.
"""
from collections import namedtuple

Case = namedtuple("Case", "name op shape dtype regime knobs expect extra splits")
CASES = []
GEN, STEM, S2T = 0, 1, 2          # loader modes (conv_igemm.h)
BS_NONE, BS_Y, BS_REC = 0, 1, 2   # BN backward sums in the epilogue (conv_igemm.hip)


def _add(name, op, shape, expect, dtype="bf16", regime="small", splits=None, extra=None, **knobs):
    name = f"{name}-{dtype}" + ("-large" if regime == "large" else "")
    assert all(c.name != name for c in CASES), name
    CASES.append(Case(name, op, shape, dtype, regime, knobs, [(f, tuple(v)) for f, v in expect], extra or {}, splits))


def fwd(BN, mode=GEN):
    return ("fwd", (BN, mode))


def glds(BP, BN, BS=BS_NONE, kxk=0, NS=2, NWP=2, NWC=2):
    return ("glds", (BP, BN, BS, kxk, NS, NWP, NWC))


def sum1(BN, NL=16):
    return ("stat_sum1", (BN, NL))


def tree(BN):
    return ("stat_tree", (BN,))


REG = dict(g1x1=(0, -1, -1))  # the register-staged general kernel for every conv
BOTH = ("bf16", "f16")

# ---- forward + statistics, small regime ---------------------------------------------------
S3 = (2, 64, 14, 18, 64, 3, 1, 1)        # 3x3 s1, ragged last tile (M = 504)
S3S2 = (2, 128, 15, 13, 128, 3, 2, 1)    # 3x3 s2, odd input, OH = 8, OW = 7
P189 = (3, 64, 7, 9, 256, 1, 1, 0)       # 1x1, M = 189
P297 = (3, 64, 11, 9, 256, 1, 1, 0)      # 1x1, M = 297 = 256 + 41
ACC = (2, 256, 14, 10, 128, 1, 2, 0)     # 1x1 s2 (OH = 7, OW = 5)
AUX = (2, 256, 14, 12, 128, 1, 1, 0)     # aux [2, 128, 7, 6] at the even pixels
C192 = (1, 192, 9, 11, 192, 3, 1, 1)     # Cout = 192: three 64-channel tiles
K5 = (2, 64, 12, 10, 128, 5, 1, 2)       # 5x5
K16 = (4, 1024, 7, 5, 64, 1, 1, 0)       # 16 K-steps
ST = (2, 128, 14, 10, 128, 1, 1, 0)      # 3 / 4 LDS stages
P64 = (2, 128, 9, 11, 64, 1, 1, 0)       # 1x1, 64-channel tiles, ragged M = 198


def WIDE(R):
    return (2, 256, 14, 12, 256, R, 1, R // 2)  # wide tiles (2304 terms for 3x3)


for dt in BOTH:
    for df, dn in ((0, "defer"), (-1, "inlaunch")):
        st64, st128 = ([sum1(64)], [sum1(128)]) if df == 0 else ([], [])
        _add(f"general_3x3_{dn}", "fwd+stats", S3, [fwd(64)] + st64, dt, "small2", stat_defer=df, **REG)
        _add(f"general_3x3_s2_{dn}", "fwd+stats", S3S2, [fwd(128)] + st128, dt, stat_defer=df, **REG)
        for bp in (128, 256):
            _add(f"glds_1x1_m297_bp{bp}_{dn}", "fwd+stats", P297, [glds(bp, 128)] + st128, dt, "small2",
                 g1x1=(1, bp, -1), stat_defer=df, wide=0)
for df, dn in ((0, "defer"), (-1, "inlaunch")):
    st64, st128 = ([sum1(64)], [sum1(128)]) if df == 0 else ([], [])
    _add(f"glds_1x1_m189_{dn}", "fwd+stats", P189, [glds(128, 128)] + st128, regime="small2", stat_defer=df, wide=0)
    _add(f"glds_3x3_{dn}", "fwd+stats", S3, [glds(128, 64, kxk=1)] + st64, regime="small2", stat_defer=df)
    _add(f"glds_3x3_s2_{dn}", "fwd+stats", S3S2, [glds(128, 128, kxk=1)] + st128, stat_defer=df, wide=0)
    for bp in (128, 256):
        _add(f"glds_1x1_bn64_bp{bp}_{dn}", "fwd+stats", P64, [glds(bp, 64)] + st64, g1x1=(1, bp, -1), stat_defer=df)
_add("glds_3x3_f16", "fwd+stats", S3, [glds(128, 64, kxk=1), sum1(64)], "f16", "small2")
_add("glds_3x3_cout192", "fwd+stats", C192, [glds(128, 64, kxk=1), sum1(64)])
_add("general_3x3_cout192", "fwd+stats", C192, [fwd(64), sum1(64)], g3x3=0)
_add("glds_5x5", "fwd+stats", K5, [glds(128, 128, kxk=1), sum1(128)], wide=0)
_add("general_5x5", "fwd+stats", K5, [fwd(128), sum1(128)], g3x3=0)
_add("glds_1x1_16_ksteps", "fwd+stats", K16, [glds(128, 64), sum1(64)])
_add("general_1x1_16_ksteps", "fwd+stats", K16, [fwd(64), sum1(64)], **REG)
# the statistics tree: level thresholds are in pixel tiles (keep these sizes)
_add("tree_one_level_16_rows", "fwd+stats", (8, 64, 56, 56, 64, 1, 1, 0), [glds(128, 64), sum1(64, 16)], stat_defer=0)
_add("tree_one_level_64_rows", "fwd+stats", (12, 64, 56, 56, 64, 1, 1, 0), [glds(128, 64), sum1(64, 64)], stat_defer=0)
_add("tree_two_level_defer", "fwd+stats", (48, 64, 56, 56, 64, 1, 1, 0), [glds(128, 64), tree(64)], stat_defer=0)
_add("tree_two_level_inlaunch", "fwd+stats", (48, 64, 56, 56, 64, 1, 1, 0), [glds(128, 64)], stat_defer=-1)
_add("tree_bn128_64_rows", "fwd+stats", (11, 64, 56, 56, 128, 1, 1, 0), [glds(128, 128, NWC=4), sum1(128, 64)])
_add("tree_bn128_two_level", "fwd+stats", (42, 64, 56, 56, 128, 1, 1, 0), [glds(128, 128), tree(128)], wide=0)
_add("tree_bn256_64_rows", "fwd+stats", (21, 64, 56, 56, 256, 1, 1, 0), [glds(256, 256, NWC=4), sum1(256, 64)], wide=3)
# wide 8-wave tiles: modes 0 (off) / 2 / 3 / 4 / 1 (auto)
for R in (1, 3):
    k = int(R != 1)
    for wm, var, st in ((0, glds(128, 128, kxk=k), sum1(128)), (2, glds(256, 128, kxk=k, NWP=4, NWC=2), sum1(128)),
                        (3, glds(256, 256, kxk=k, NWC=4), sum1(256)), (4, glds(128, 128, kxk=k, NWC=4), sum1(128)),
                        (1, glds(128, 128, kxk=k, NWC=4), sum1(128))):
        _add(f"wide_{R}x{R}_mode{wm}", "fwd+stats", WIDE(R), [var, st], wide=wm)
        if wm in (2, 3, 4):
            _add(f"wide_{R}x{R}_mode{wm}", "fwd", WIDE(R), [var], "f16", wide=wm)
for ns in (3, 4):
    _add(f"stages{ns}_1x1_bn128", "fwd+stats", ST, [glds(128, 128, NS=ns), sum1(128)], glds=ns, wide=0)
    _add(f"stages{ns}_1x1_bn64", "fwd+stats", K16, [glds(128, 64, NS=ns), sum1(64)], glds=ns)
    _add(f"stages{ns}_3x3_bn128", "fwd+stats", S3S2, [glds(128, 128, kxk=1, NS=ns), sum1(128)], glds=ns, wide=0)
    _add(f"stages{ns}_3x3_bn64", "fwd+stats", S3, [glds(128, 64, kxk=1, NS=ns), sum1(64)], regime="small2", glds=ns)
    _add(f"stages{ns}_1x1_bn128", "fwd", ST, [glds(128, 128, NS=ns)], "f16", glds=ns, wide=0)

# ---- accumulate / aux -----------------------------------------------------------------------
for dt in BOTH:
    for on, kn in ((1, "glds"), (0, "general")):
        var = glds(128, 128) if on else fwd(128)
        _add(f"accumulate_{kn}", "acc", ACC, [var], dt, g1x1=(on, -1, -1), wide=0)
        _add(f"aux_{kn}", "aux", AUX, [var], dt, g1x1=(on, -1, -1), wide=0)
_add("aux_wide_auto", "aux", AUX, [glds(128, 128, NWC=4)])
_add("accumulate_bp256", "acc", ACC, [glds(256, 128)], g1x1=(1, 256, -1), wide=0)

# ---- large regime (storage rounding, ties), no statistics --------------------------------------
for dt in BOTH:
    _add("wide_3x3_auto", "fwd", WIDE(3), [glds(128, 128, kxk=1, NWC=4)], dt, "large")
    _add("wide_1x1_auto", "fwd", WIDE(1), [glds(128, 128, NWC=4)], dt, "large")
    _add("general_3x3", "fwd", WIDE(3), [fwd(128)], dt, "large", **REG)
    _add("accumulate_glds", "acc", ACC, [glds(128, 128)], dt, "large", wide=0)
    _add("aux_glds", "aux", AUX, [glds(128, 128)], dt, "large", wide=0)
    _add("aux_general", "aux", AUX, [fwd(128)], dt, "large", **REG)
    _add("s2t", "s2t", (3, 64, 10, 14, 128), [fwd(64, S2T)], dt, "large")

# ---- S2T, stem ---------------------------------------------------------------------------------
for dt in BOTH:
    _add("s2t_bn64", "s2t", (3, 64, 10, 14, 128), [fwd(64, S2T)], dt)   # 420 pixels per parity class
    _add("stem_k64", "stem", (3, 23, 27, 64), [fwd(64, STEM), sum1(64)], dt, "small2",
         extra=dict(wgrad=("wgrad", (64, 64, STEM))))
_add("s2t_bn128", "s2t", (2, 128, 5, 9, 64), [fwd(128, S2T)])
_add("stem_k128", "stem", (3, 23, 27, 128), [fwd(128, STEM), sum1(128)], regime="small2",
     extra=dict(wgrad=("wgrad", (128, 64, STEM))))

# ---- data gradient + the producing BN's backward sums -------------------------------------------
DB256, DB64 = (3, 64, 7, 9, 256), (2, 128, 14, 10, 64)
for act, R in ((1, 1), (2, 1), (2, 3)):
    BS, k = (BS_Y if act == 1 else BS_REC), int(R != 1)
    ex = dict(act=act, R=R)
    for dt in BOTH:
        _add(f"dgrad_bn_act{act}_R{R}_wide0", "dgrad_bn", DB256, [glds(128, 128, BS, k), sum1(128)], dt, extra=ex, wide=0)
    # auto: BS_Y stays on 4 waves, the recomputed mask takes 8
    _add(f"dgrad_bn_act{act}_R{R}_auto", "dgrad_bn", DB256,
         [glds(128, 128, BS, k, NWC=2 if act == 1 else 4), sum1(128)], extra=ex)
    _add(f"dgrad_bn_act{act}_R{R}_wide4", "dgrad_bn", DB256, [glds(128, 128, BS, k, NWC=4), sum1(128)], extra=ex, wide=4)
    _add(f"dgrad_bn_act{act}_R{R}_bn64", "dgrad_bn", DB64, [glds(128, 64, BS, k), sum1(64)], extra=ex)

# ---- weight gradients ---------------------------------------------------------------------------
FIX_ALL = 1 << 20
WPATHS = (("reg", dict(wgrad=0, wgrad_fixup=0), None), ("glds4", dict(wgrad=2, wgrad_waves=4, wgrad_fixup=0), (2, 2, 0)),
          ("glds8", dict(wgrad=2, wgrad_waves=8, wgrad_fixup=0), (0, 0, 0)),
          ("fixup", dict(wgrad=2, wgrad_waves=8, wgrad_fixup=FIX_ALL), (0, 0, 1)))


def wvariant(shape, path):
    """BM | Cout, BN | C (128 when divisible, else 64); 8 waves as 2 x 4 (4 x 2 on 128 x 64)."""
    BM, BN = (128 if shape[4] % 128 == 0 else 64), (128 if shape[1] % 128 == 0 else 64)
    if path is None:
        return ("wgrad", (BM, BN, GEN))
    nwm, nwn, fix = path
    if nwm == 0:
        nwm = 4 if (BM, BN) == (128, 64) else 2
        nwn = 8 // nwm
    return ("wgrad_glds", (BM, BN, nwm, nwn, fix))


WSHAPES = [
    # name, shape, (splits, pixels per split, pixels in the last split)
    ("1x1_m189", (3, 256, 7, 9, 128, 1, 1, 0), (1, 192, 189)),           # one split, ragged
    ("3x3_m504", S3, (1, 512, 504)),
    ("3x3_s2_m112", S3S2, (1, 128, 112)),
    ("1x1_s2_m70", ACC, (1, 128, 70)),
    ("3x3_two_splits_ragged", (3, 64, 21, 19, 128, 3, 1, 1), (2, 640, 557)),
    ("3x3_several_splits", (4, 64, 28, 26, 128, 3, 1, 1), (5, 640, 352)),
    ("3x3_empty_last_split", (2, 64, 50, 82, 64, 3, 1, 1), (16, 576, 0)),  # split 14: 136 pixels, split 15: none
]
for K in (64, 128):
    for Cc in (64, 128):
        WSHAPES.append((f"1x1_tile{K}x{Cc}", (3, Cc, 9, 7, K, 1, 1, 0), (1, 192, 189)))
        WSHAPES.append((f"3x3_tile{K}x{Cc}", (3, Cc, 9, 7, K, 3, 1, 1), (1, 192, 189)))
for wn, sh, spl in WSHAPES:
    for pn, kn, path in WPATHS:
        _add(f"wgrad_{wn}_{pn}", "wgrad", sh, [wvariant(sh, path)], regime="small2", splits=spl, **kn)
# wgrad_config(1): the LDS-DMA kernel for the 1x1 convs only
_add("wgrad_1x1_m189_mode1", "wgrad", WSHAPES[0][1], [wvariant(WSHAPES[0][1], (0, 0, 0))], regime="small2",
     splits=WSHAPES[0][2], wgrad=1, wgrad_waves=8, wgrad_fixup=0)
_add("wgrad_3x3_m504_mode1", "wgrad", S3, [wvariant(S3, None)], regime="small2", splits=(1, 512, 504), wgrad=1,
     wgrad_waves=8, wgrad_fixup=0)
for wn, sh, spl in (WSHAPES[0], WSHAPES[4], WSHAPES[6]):
    for pn, kn, path in WPATHS:
        _add(f"wgrad_{wn}_{pn}", "wgrad", sh, [wvariant(sh, path)], "f16", "small2", splits=spl, **kn)
_add("wgrad_reduce_batch", "wgrad_batch", (WSHAPES[0][1], WSHAPES[4][1], WSHAPES[6][1]), [], regime="small2",
     wgrad_fixup=0)

BY_NAME = {c.name: c for c in CASES}


def expected_variants():
    """{family: set of template-argument tuples} the table claims to reach."""
    out = {}
    for c in CASES:
        for fam, v in list(c.expect) + ([c.extra["wgrad"]] if "wgrad" in c.extra else []):
            out.setdefault(fam, set()).add(tuple(v))
    return out
