"""ops/se.py's formulas, forward and backward, in float64 torch on the CPU from the already-rounded inputs.
``y`` of the backward is the STORED forward output: its sign is the ReLU mask (zero output: zero derivative)."""
import torch


def forward(u, idn, w1, b1, w2, b2):
    u, idn, w1, b1, w2, b2 = (t.detach().double().cpu() for t in (u, idn, w1, b1, w2, b2))
    C = u.shape[1]
    p = u.mean((2, 3))
    h = torch.relu(p @ w1.reshape(-1, C).t() + b1)
    s = torch.sigmoid(h @ w2.reshape(C, -1).t() + b2)
    return dict(p=p, h=h, s=s, y=torch.relu(u * s[:, :, None, None] + idn))


def backward(g, y, u, w1, w2, f):
    g, y, u, w1, w2 = (t.detach().double().cpu() for t in (g, y, u, w1, w2))
    C, HW = u.shape[1], u.shape[2] * u.shape[3]
    w1, w2 = w1.reshape(-1, C), w2.reshape(C, -1)
    gm = g * (y > 0)
    ds = (gm * u).sum((2, 3))
    dz2 = ds * f["s"] * (1 - f["s"])
    dz1 = (dz2 @ w2) * (f["h"] > 0)
    dp = dz1 @ w1
    return dict(gm=gm, ds=ds, dz2=dz2, dz1=dz1, dp=dp, d_identity=gm, db2=dz2.sum(0), dw2=dz2.t() @ f["h"],
                db1=dz1.sum(0), dw1=dz1.t() @ f["p"], du=gm * f["s"][:, :, None, None] + dp[:, :, None, None] / HW)
