"""Digests of every _C.bn_nhwc entry point, for comparing two builds of the extension bit for bit.

    [DPA_EXT_SO=ddp_practice_amd/_C_x.so] python scripts/exp/bn_bits.py OUT

Inputs are the seeded ones of tests/_bn_ref.py (float kind), in bf16, fp16 and fp32, channel counts
8 (4 in fp32), 24, 72, 320, 2048 and 2, 189 and 38,400 rows (38,400 rows at C <= 72 and, in bf16,
C = 320: the float64 inputs of the wider ones take gigabytes).  Every case runs under the default
grid targets, targets (1, 1, 1), statistics target 300 (a two-level tree at 38,400 rows: bf16
C = 320, fp32 C = 24) and, for the kernels with a ticket tree, the fenced hand-off; each runs twice
in-process and prints `BITS <case> <sha256>` (or `UNSTABLE <case>` when the two runs differ).  The
digest covers dtype, shape and raw bytes of every output."""
import hashlib
import sys

import torch

sys.path.insert(0, __file__.rsplit("/scripts", 1)[0])
from ddp_practice_amd import _ext  # noqa: E402
from tests import _bn_ref as R  # noqa: E402

DEV = "cuda"
TAG = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
ROWS = (2, 189, 38400)
# (name, (stats, apply, elemt) targets, hand-off)
SETTINGS = (("default", (0, 512, 1024), 1), ("one", (1, 1, 1), 1), ("st300", (300, 512, 1024), 1),
            ("fenced", (0, 512, 1024), 0), ("st300_fenced", (300, 512, 1024), 0))
TREE = ("fwd_stats", "bwd_stats", "bwd_elemt_rbn")  # the entry points the hand-off mode reaches


def digest(*ts):
    h = hashlib.sha256()
    for t in ts:
        t = t.detach().cpu().contiguous()
        h.update(str(t.dtype).encode() + str(tuple(t.shape)).encode())
        h.update(t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def channels(dt):
    return (4 if dt == torch.float32 else 8, 24, 72, 320, 2048)


def inputs(M, C, dt):
    """The main and the downsample branch's tensors on the device."""
    seed = R.elem_seed(dt, C, M)
    return tuple({k: (v.to(dt) if k in ("x", "res", "dy", "y") else v.float()).to(DEV)
                  for k, v in R.elem_inputs("float", M, C, dt, seed + extra).items()} for extra in (0, 500))


def bn_cases(B, M, C, dv, ds):
    """(name, f) per BN entry point and variant; f() returns the output tensors."""
    part = torch.zeros(int(B.MAX_PARTIAL_ROWS) * 2 * 2048, device=DEV)
    tk = torch.zeros(int(B.MAX_TICKETS), dtype=torch.int32, device=DEV)
    Z = lambda n: torch.zeros(n, device=DEV)  # noqa: E731
    like = lambda: torch.zeros_like(dv["x"])  # noqa: E731

    def stats(d):
        st, nbt = Z(3 * C + 4), torch.zeros(1, dtype=torch.int64, device=DEV)
        B.fwd_stats(d["x"], C, d["rm0"], part, tk, st, nbt)
        return st, nbt

    yield "fwd_stats", lambda: (*stats(dv), tk)
    st, rst = stats(dv)[0], stats(ds)[0]
    nbt3 = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    for train, mom, res, relu in ((True, 0.1, False, False), (True, 0.1, False, True), (True, -1.0, True, False),
                                  (True, 0.1, True, True), (False, 0.1, False, True), (False, 0.1, True, True)):
        def f(train=train, mom=mom, res=res, relu=relu):
            y, rm, rv, save = like(), dv["rm0"].clone(), dv["rv0"].clone(), Z(2 * C)
            B.apply(dv["x"], dv["res"] if res else None, y, C, st, dv["gamma"], dv["beta"], rm, rv, nbt3, mom, R.EPS,
                    train, relu, save)
            return y, rm, rv, save
        yield f"apply_{'train' if train else 'eval'}_mom{mom}_res{int(res)}_relu{int(relu)}", f
    for train in (True, False):
        def f(train=train):
            y, rm, rv, rrm, rrv = like(), dv["rm0"].clone(), dv["rv0"].clone(), ds["rm0"].clone(), ds["rv0"].clone()
            save, rsave = Z(2 * C), Z(2 * C)
            B.apply_resbn(dv["x"], ds["x"], y, C, st, dv["gamma"], dv["beta"], rm, rv, nbt3, 0.1, R.EPS, save, rst,
                          ds["gamma"], ds["beta"], rrm, rrv, nbt3, -1.0, R.EPS, rsave, train)
            return y, rm, rv, rrm, rrv, save, rsave
        yield f"apply_resbn_{'train' if train else 'eval'}", f

    def sums(act):
        out, dg, db = Z(2 * C), Z(C), Z(C)
        B.bwd_stats(dv["dy"], dv["y"] if act == 1 else None, dv["x"], C, act, dv["save"], dv["gamma"], dv["beta"], part,
                    tk, out, dg, db)
        return out, dg, db

    fs = Z(3 * C + 4)
    fs[2 * C] = M
    for act in (0, 1, 2):
        yield f"bwd_stats_act{act}", lambda act=act: (*sums(act), tk)
        out = sums(act)[0]
        for dres in (False, True):
            def f(act=act, dres=dres, out=out):
                dx, dr = like(), like()
                B.bwd_elemt(dv["dy"], dv["y"] if act == 1 else None, dv["x"], C, act, dv["save"], out, fs, dv["gamma"],
                            dv["beta"], dx, dr if dres else None)
                return dx, dr
            yield f"bwd_elemt_act{act}_dres{int(dres)}", f

    def f(out=sums(1)[0]):
        dx, dz, rout, rdg, rdb = like(), like(), Z(2 * C), Z(C), Z(C)
        B.bwd_elemt_rbn(dv["dy"], dv["y"], dv["x"], C, dv["save"], out, fs, dv["gamma"], dv["beta"], dx, dz, ds["x"],
                        ds["save"], part, tk, rout, rdg, rdb)
        return dx, dz, rout, rdg, rdb, tk
    yield "bwd_elemt_rbn", f


def pool_cases(B, dt):
    g = torch.Generator().manual_seed(77 + list(TAG).index(dt))
    for (N, H, W), C in (((2, 7, 9), channels(dt)[0]), ((3, 15, 12), 24), ((2, 56, 56), 72)):
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        x = torch.randn(N, H, W, C, generator=g).to(dt).to(DEV)
        dy = torch.randn(N, OH, OW, C, generator=g).to(dt).to(DEV)
        dp = torch.randn(N, C, generator=g).to(dt).to(DEV)

        def mp(x=x, dy=dy, N=N, H=H, W=W, C=C, OH=OH, OW=OW):
            y = torch.zeros(N, OH, OW, C, dtype=dt, device=DEV)
            idx = torch.zeros(N, OH, OW, C, dtype=torch.uint8, device=DEV)
            dx = torch.zeros_like(x)
            B.maxpool_fwd(x, y, idx)
            B.maxpool_bwd(dy, idx, dx)
            return y, idx, dx

        def ap(x=x, dp=dp, N=N, H=H, W=W, C=C):
            y, dx = torch.zeros(N, C, dtype=dt, device=DEV), torch.zeros_like(x)
            B.avgpool_fwd(x, y, H * W)
            B.avgpool_bwd(dp, dx, H * W)
            return y, dx
        yield f"maxpool_{N}x{H}x{W}x{C}", mp
        yield f"avgpool_{N}x{H}x{W}x{C}", ap


def main(out):
    B = _ext.load().bn_nhwc
    lines = []

    def run(case, f):
        a, b = digest(*f()), digest(*f())
        torch.cuda.synchronize()
        lines.append(f"BITS {case} {a}" if a == b else f"UNSTABLE {case}")
        print(lines[-1], flush=True)

    try:
        for dt, tag in TAG.items():
            for name, f in pool_cases(B, dt):
                run(f"{name}_{tag}", f)
            for M in ROWS:
                for C in channels(dt):
                    if M == ROWS[-1] and C > 72 and not (C == 320 and dt == torch.bfloat16):
                        continue
                    dv, ds = inputs(M, C, dt)
                    for sname, targets, wt in SETTINGS:
                        B.set_grid_targets(*targets)
                        B.set_handoff(wt)
                        for name, f in bn_cases(B, M, C, dv, ds):
                            if wt == 0 and not name.startswith(TREE):
                                continue
                            run(f"{name}_{tag}_C{C}_M{M}_{sname}", f)
    finally:
        B.set_grid_targets(0, 512, 1024)
        B.set_handoff(1)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1])
