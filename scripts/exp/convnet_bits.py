"""Digests of the ConvNet conv / BN kernels called op by op, for comparing two builds of the
extension bit for bit on the paths a training step does not reach (the per-layer ops, eval
forms, the stand-alone data gradient and weight gradients).

    [DPA_EXT_SO=ddp_practice_amd/_C_x.so] python scripts/exp/convnet_bits.py OUT

Inputs come from a fixed seed; every case runs twice at B = 1 and B = 3 in bf16, fp16 and fp32
and prints `BITS <case> <sha256>` (or `UNSTABLE <case>` when the two runs differ).  The digest
covers dtype, shape and raw bytes of every output.  DPA_LP_DYN_BWD / DPA_FP32_MERGED_BWD are
read once per process: run the script once per setting."""
import hashlib
import sys

import torch

sys.path.insert(0, __file__.rsplit("/scripts", 1)[0])
from ddp_practice_amd import _ext  # noqa: E402

DEV, EPS = "cuda", 1e-5


def digest(*ts):
    h = hashlib.sha256()
    for t in ts:
        t = t.detach().cpu().contiguous()
        h.update(str(t.dtype).encode() + str(tuple(t.shape)).encode())
        h.update(t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def block(g, B, C, H, dt):
    """A conv block's saved tensors: pre-BN output y, its statistics, pooled grad, index, xhat."""
    y = torch.randn(B, C, H, H, generator=g).to(dt)
    shift = torch.rand(C, generator=g) * 0.2 - 0.1
    d = y.float() - shift.view(1, -1, 1, 1)
    n = float(B * H * H)
    fslab = torch.cat([d.sum((0, 2, 3)), (d * d).sum((0, 2, 3)), torch.tensor([n])])
    fstats = torch.cat([fslab, shift])
    P = H // 2
    return dict(y=y, fslab=fslab, fstats=fstats, gamma=torch.rand(C, generator=g) + 0.5,
                beta=torch.rand(C, generator=g) * 0.4 - 0.2, dp=torch.randn(B, C, P, P, generator=g).to(dt),
                idx=torch.randint(0, 8, (B, C, P, P), generator=g, dtype=torch.uint8),
                xh=torch.randn(B, C, P, P, generator=g).to(dt), gsum=torch.randn(2 * C, generator=g))


def cases(C, B, dt):
    cb, cn = C.convblock, C.convnet
    g = torch.Generator().manual_seed(1000 * B + [torch.bfloat16, torch.float16, torch.float32].index(dt))
    D = lambda t: t.to(DEV)  # noqa: E731
    Z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)  # noqa: E731
    fp32 = dt == torch.float32
    x = torch.rand(B, 1, 28, 28, generator=g).to(dt)
    w1, b1 = torch.randn(16, 1, 5, 5, generator=g) * 0.2, torch.randn(16, generator=g) * 0.1
    w2, b2 = torch.randn(32, 16, 5, 5, generator=g) * 0.05, torch.randn(32, generator=g) * 0.1
    k1, k2 = block(g, B, 16, 28, dt), block(g, B, 32, 14, dt)
    p1 = torch.randn(B, 16, 14, 14, generator=g).to(dt)
    rm2 = torch.rand(32, generator=g) * 0.2 - 0.1
    shapes = ((x, w1, b1, 16, 28), (p1, w2, b2, 32, 14))

    for li, (xi, w, b, co, H) in enumerate(shapes, 1):
        ci = xi.size(1)
        for st in (True, False):
            def f(xi=xi, w=w, b=b, co=co, H=H, ci=ci, st=st):
                y = Z(B, co, H, H, dtype=dt)
                fslab = Z(cb.fwd_rows(ci, co, H, H, B) * cb.fslab_row(co))
                fstats = Z(cb.stats_len(co))
                if st:
                    cb.conv_fwd(D(xi), D(w), D(b), y, fslab, fstats, Z(co) + 0.05)
                else:
                    cb.conv_fwd(D(xi), D(w), D(b), y)
                return y, fslab, fstats
            yield f"conv_fwd{li}_{'stats' if st else 'plain'}", f

        def f(xi=xi, co=co, H=H, ci=ci, k=(k1, k2)[li - 1]):
            wslab = Z(cb.wgrad_rows(ci, co, H, H, B) * (co * ci * 25 + co))
            cb.conv_wgrad(D(xi), D(k["y"]), wslab)
            return (wslab,)
        yield f"conv_wgrad{li}", f

    def f():
        dx = Z(B, 16, 14, 14, dtype=dt)
        cb.conv_dgrad(D(k2["y"]), D(w2), dx)
        return (dx,)
    yield "conv_dgrad", f

    def conv1(st, gather):
        y1, wf, wd = Z(B, 16, 28, 28, dtype=dt), Z(cn.W2F_LEN, dtype=dt), Z(cn.W2D_LEN, dtype=dt)
        fslab, fstats, shift = Z(B * 4 * 33), Z(49), Z(16) + 0.05
        if not gather:
            a = (fslab, fstats, shift) if st else (None, None, None)
            cn.conv1_fwd_pack(D(x), D(w1), D(b1), y1, *a, D(w2), wf, wd)
            return y1, fslab, fstats, wf, wd
        N = 4 * B
        imgs = torch.randint(0, 256, (N, 28, 28), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
        labels, order = torch.arange(N) % 10, torch.randperm(N, generator=torch.Generator().manual_seed(8))
        ctr, lab, xb = Z(2, dtype=torch.int32), Z(B, dtype=torch.int64), Z(B, 1, 28, 28, dtype=dt)
        outs = []
        for _ in range(2):  # twice: the second launch reads the advanced step counter
            cn.conv1_fwd_pack_gather(xb, D(w1), D(b1), y1, fslab, fstats, shift, D(w2), wf, wd, D(imgs), D(labels),
                                     D(order), ctr, lab, 1.0 / 255, -0.5)
            outs += [xb.clone(), lab.clone(), ctr.clone(), y1.clone(), fslab.clone()]
        return outs
    yield "conv1_fwd_pack_stats", lambda: conv1(True, False)
    yield "conv1_fwd_pack_plain", lambda: conv1(False, False)
    yield "conv1_fwd_pack_gather", lambda: conv1(True, True)

    wpk_f, wpk_d = Z(cn.W2F_LEN, dtype=dt), Z(cn.W2D_LEN, dtype=dt)
    cn.conv1_fwd_pack(D(x), D(w1), D(b1), Z(B, 16, 28, 28, dtype=dt), None, None, None, D(w2), wpk_f, wpk_d)

    for train in (True, False):
        def f(train=train):
            ns = cn.fwd2_split(fp32)
            y2, fslab2, fstats2 = Z(B, 32, 14, 14, dtype=dt), Z(B * ns * 65), Z(97)
            po, io, xo = Z(B, 16, 14, 14, dtype=dt), Z(B, 16, 14, 14, dtype=torch.uint8), Z(B, 16, 14, 14, dtype=dt)
            rm1, rv1, nbt1 = Z(16), Z(16) + 1, Z(1, dtype=torch.int64)
            cn.conv2_fwd(D(k1["y"]), D(k1["fslab"]), D(k1["fstats"]), D(k1["gamma"]), D(k1["beta"]), rm1, rv1, nbt1, 0.1,
                         EPS, train, D(w2), D(b2), y2, fslab2 if train else None, fstats2, D(rm2), po, io, xo, wpk_f, None)
            return y2, fslab2, fstats2, po, io, xo, rm1, rv1, nbt1
        yield f"conv2_fwd_{'train' if train else 'eval'}", f

    def bwd2(kind):
        dp1, bslab1 = Z(B, 16, 14, 14, dtype=dt), Z(cn.dgrad2_rows(B, fp32) * 32)
        wslab2 = Z(cn.wgrad_bn_rows(2, B) * (32 * 400 + 32))
        a = (wpk_d, D(k2["y"]), D(k2["dp"]), D(k2["idx"]), D(k2["fstats"]), D(k2["gsum"]), D(k2["gamma"]), EPS, dp1,
             D(k1["idx"][:, :, :14, :14].contiguous()), D(k1["xh"][:, :, :14, :14].contiguous()), bslab1)
        if kind == "dgrad":
            cn.conv2_dgrad(*a, None)
            return dp1, bslab1
        dg, dbe, fdw, fdb = Z(32), Z(32), Z(10 * 1568), Z(10)
        fc = (None,) * 4
        if kind == "fc":
            gg = torch.Generator().manual_seed(9)
            fc = (D(torch.randn(B, 10, generator=gg).to(dt)), D(torch.randn(B, 1568, generator=gg).to(dt)), fdw, fdb)
        cn.conv2_bwd(*a, D(p1), wslab2, None, None, dg, dbe, *fc, None)
        return dp1, bslab1, wslab2, dg, dbe, fdw, fdb
    yield "conv2_dgrad", lambda: bwd2("dgrad")
    yield "conv2_bwd", lambda: bwd2("plain")
    yield "conv2_bwd_fc", lambda: bwd2("fc")

    for li, (xi, k, co) in enumerate(((x, k1, 16), (p1, k2, 32)), 1):
        def f(li=li, xi=xi, k=k, co=co):
            wslab = Z(cn.wgrad_bn_rows(li, B) * (co * xi.size(1) * 25 + co))
            dg, dbe = Z(co), Z(co)
            cn.conv_wgrad_bn(D(xi), D(k["y"]), D(k["dp"]), D(k["idx"]), D(k["fstats"]), D(k["gsum"]), None, D(k["gamma"]),
                             EPS, dg, dbe, wslab, None)
            return wslab, dg, dbe
        yield f"conv_wgrad_bn{li}", f

    def f():
        gg = torch.Generator().manual_seed(10)
        wslab1, dg, dbe = Z(cn.wgrad_bn_rows(1, B) * 416), Z(16), Z(16)
        wslab2, out2 = D(torch.randn(cn.wgrad_bn_rows(2, B) * 12832, generator=gg)), Z(12832)
        cn.conv1_wgrad_slab2(D(x), D(k1["y"]), D(k1["dp"]), D(k1["idx"]), D(k1["fstats"]), D(k1["gsum"]), None,
                             D(k1["gamma"]), EPS, dg, dbe, wslab1, wslab2, out2, None, None)
        return wslab1, dg, dbe, out2
    yield "conv1_wgrad_slab2", f


def main(out):
    C = _ext.load()
    lines = []
    for dt, tag in ((torch.bfloat16, "bf16"), (torch.float16, "fp16"), (torch.float32, "fp32")):
        for B in (1, 3):
            for name, f in cases(C, B, dt):
                a, b = digest(*f()), digest(*f())
                torch.cuda.synchronize()
                case = f"{name}_{tag}_B{B}"
                lines.append(f"BITS {case} {a}" if a == b else f"UNSTABLE {case}")
                print(lines[-1], flush=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1])
