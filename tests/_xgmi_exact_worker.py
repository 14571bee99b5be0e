"""Worker of tests/test_xgmi_exact_gpu.py: W processes on ONE GPU run the xGMI engine against each
other, and every rank compares every result bit for bit with tests/_xgmi_ref.py (each rank can
generate every rank's data, so each computes the whole reference itself).

The engine is opened small -- one-shot slots of 32 KiB (8192 elements, 4 workgroups), a two-shot
region of 256 KiB on a grid of 2 -- so the largest grid any rank launches is a handful of
workgroups.  Every output is a view into a sentinel-filled buffer whose guard elements are compared
after the call, inputs of out-of-place calls are compared with what was uploaded, and the engine's
error word is read after every call.  Each rank returns the bytes of every result (the parent
compares the ranks) and the number of elements it compared."""
import os
import time
import traceback
from datetime import timedelta

import torch
import torch.distributed  # noqa: F401  (TCPStore)

from . import _xgmi_ref as X

MAX_BYTES, TS_BYTES, TS_GRID = 32 << 10, 256 << 10, 2
SLOT = MAX_BYTES // 4            # 8192 elements: the one-shot limit
TS_MAX = TS_BYTES // 4           # 65536 elements: the two-shot limit
CHUNK = 2048                     # elements per one-shot workgroup and per two-shot chunk

ONESHOT_N = [1, 7, 8, 9, 2040, 2047, 2048, 2049, 2056, 4095, 4099, 8191, 8192]
SITE_N = [1, 2, 63, 64, 65, 127, 128]
WIDE = [(1, 1), (7, 7), (129, 3), (513, 8), (2049, 64), (4097, 9), (4224, 1), (4224, 64)]
SGD_SIZES = (7, 33, 1023, 1025, 4)   # 525 float4 granules: three exchanging workgroups
SLAB_SIZES = (7, 33, 1023, 1025, 36)  # the last tensor's gradient is the slab's 36 columns


def twoshot_sizes(world):
    """Shard edges (shards are whole 2048-element chunks), an empty and a one-element last shard,
    three chunks per shard on the grid of two, the region's maximum; large, small, large."""
    w = world
    return [TS_MAX, 1, 3 * w * CHUNK + 9, 5, w * CHUNK + 1, 2047, w * CHUNK, 2048, (w - 1) * CHUNK + 1, 2049,
            w * CHUNK - 1, (w - 1) * CHUNK]


def data(rank, n, dt, call):
    g = torch.Generator(device="cpu").manual_seed((call * 131 + rank) * 100003 + n)
    return torch.randn(n, generator=g).to(dt)


class Run:
    def __init__(self, rank, world, dev, x):
        self.rank, self.world, self.dev, self.x = rank, world, dev, x
        self.call = 0
        self.out, self.count = {}, {}

    def inputs(self, n, dt, place=None):
        """Fresh data of every rank for this call; ``place``: [(index, SPECIALS entry, rank)]."""
        self.call += 1
        xs = [data(r, n, dt, self.call) for r in range(self.world)]
        for i, sp, r in place or ():
            for k, v in enumerate(sp):
                xs[(r + k) % self.world][i] = v
        return xs

    def done(self, what):
        torch.cuda.synchronize()
        assert self.x.error() == 0, (what, self.x.error_string(), self.x.debug_state(2.0))

    def record(self, mode, key, g, n):
        self.out[f"{mode}:{self.call}:{key}"] = X.bits(g.view).numpy().tobytes()
        self.count[mode] = self.count.get(mode, 0) + n

    def reduce(self, mode, fn, ref, n, dn, op, inplace, place=None):
        """One all-reduce through ``fn(t, op, out)`` against ``ref(xs, op, dt)``."""
        dt = X.DTYPES[dn]
        xs = self.inputs(n, dt, place)
        what = (mode, self.call, n, dn, op, "in place" if inplace else "out of place", place)
        src = X.Guarded(n, dt, self.dev)
        src.load(xs[self.rank])
        dst = src if inplace else X.Guarded(n, dt, self.dev)
        fn(src.view, op, dst.view)
        self.done(what)
        want = ref(xs, op, dt)
        cnt = dst.check(want, what)
        if not inplace:
            assert src.check(xs[self.rank], (what, "input")) == n
        if op in ("sum", "avg"):  # AMP's overflow agreement: one rank's non-finite value reaches all
            nonfin = ~torch.stack([t.float().isfinite() for t in xs]).all(0)
            got = dst.view.float().cpu()
            assert not bool(got[nonfin].isfinite().any()), (what, "a non-finite contribution came out finite")
        self.record(mode, f"{n}{dn}{op}", dst, cnt)


# ------------------------------------------------------------------------------ modes
def oneshot(run):
    x = run.x
    fn = lambda t, op, o: x.all_reduce(t, op, o)
    for dn in X.DTYPES:
        for op in X.OPS:
            for n in ONESHOT_N:  # every (size, dtype, op) in place and out of place
                for inplace in (True, False):
                    run.reduce("oneshot", fn, X.reduce, n, dn, op, inplace=inplace)
    for dn in X.DTYPES:  # the same size three times in a row: calls k and k + 2 share a parity
        for n in (2049, 8192):
            for rep in range(3):
                run.reduce("oneshot", fn, X.reduce, n, dn, "sum", inplace=rep != 1)
    # SPECIALS on one rank: the first element, the last element of a full lane, the last element
    n, S = 2049, X.SPECIALS
    for dn in X.DTYPES:
        for op in ("sum", "avg"):
            for r in range(run.world):
                for i in range(len(S)):
                    place = [(0, S[i], r), (7, S[(i + 1) % len(S)], r), (n - 1, S[(i + 2) % len(S)], r)]
                    run.reduce("oneshot specials", fn, X.reduce, n, dn, op, inplace=bool(i & 1), place=place)


def _issued(x):
    """(one-shot, two-shot) launches this rank's host has issued on engine ``x``."""
    return tuple(x.issued())


def twoshot(run, C, x2):
    x = run.x
    fn = lambda t, op, o: x.all_reduce_twoshot(t, op, o)
    k = 0
    for dn in X.DTYPES:
        for op in X.OPS:
            for n in twoshot_sizes(run.world):
                run.reduce("twoshot", fn, X.reduce_twoshot, n, dn, op, inplace=bool(k & 1))
                k += 1
            k += 1  # 12 sizes: the next (dtype, op) starts on the other placement
    for dn in X.DTYPES:
        for rep in range(3):
            run.reduce("twoshot", fn, X.reduce_twoshot, 3 * run.world * CHUNK + 9, dn, "avg", inplace=rep != 1)
    # XgmiCollective routing: one-shot up to the slot, two-shot above; without a two-shot region
    # (the second engine) back-to-back slot-sized one-shot launches
    for eng, cases in ((x, [(SLOT, 1, 0), (SLOT + 1, 0, 1), (3 * SLOT + 5, 0, 1)]),
                       (x2, [(SLOT + 1, 2, 0), (3 * SLOT + 5, 4, 0)])):
        xc = C.xgmi.XgmiCollective(eng)
        fc = lambda t, op, o: xc.all_reduce(t, op, o)
        run.x = eng  # the error word read after each call is this engine's
        for n, d1, d2 in cases:
            a = _issued(eng)
            for dn, op, inplace in (("f32", "sum", True), ("bf16", "avg", False), ("f16", "max", True)):
                run.reduce("routing", fc, X.reduce_twoshot if d2 else X.reduce, n, dn, op, inplace)
            b = _issued(eng)
            assert (b[0] - a[0], b[1] - a[1]) == (3 * d1, 3 * d2), (n, a, b, "one-shot / two-shot launches")
        run.x = x
        del xc


def _site_call(run, site, n, grid):
    xs = run.inputs(n, torch.float32)
    t = X.Guarded(n, torch.float32, run.dev)
    t.load(xs[run.rank])
    o = X.Guarded(grid * n, torch.float32, run.dev)
    run.x.site_probe(site, t.view, o.view, grid)
    what = ("site", run.call, site, n, grid)
    run.done(what)
    cnt = o.check(X.site_sum(xs).repeat(grid), what)  # every workgroup's row
    t.check(xs[run.rank], (what, "input"))
    run.record("site", f"{site}-{n}-{grid}", o, cnt)


def _wide_call(run, n, nblk):
    xs = run.inputs(n, torch.float32)
    t = X.Guarded(n, torch.float32, run.dev)
    t.load(xs[run.rank])
    o = X.Guarded(n, torch.float32, run.dev)
    run.x.wide_probe(t.view, o.view, nblk)
    what = ("wide", run.call, n, nblk)
    run.done(what)
    cnt = o.check(X.site_sum(xs), what)
    t.check(xs[run.rank], (what, "input"))
    run.record("wide", f"{n}-{nblk}", o, cnt)


def sites(run):
    k = 0
    for grid in (1, 3, 4, 3):
        for n in SITE_N:  # two site ids in turn: their epochs and parities advance independently
            _site_call(run, k % 2, n, grid)
            k += 1
    for _ in range(3):  # one site, one size, three launches in a row
        _site_call(run, 0, 65, 3)
    for rnd in range(3):  # the finisher count changes from call to call
        for n, nblk in WIDE:
            _wide_call(run, n, nblk)
    for _ in range(3):
        _wide_call(run, 129, 3)


def graph(run):
    """One single-stream capture of a one-shot, a two-shot and a site exchange, replayed with
    fresh inputs (world 2 only: the ranks of a larger world run with one hardware queue)."""
    x, dev, f32 = run.x, run.dev, torch.float32
    na, nb, ns, grid = 4099, 2 * run.world * CHUNK + 1, 65, 3
    a = X.Guarded(na, f32, dev)
    b, bo = X.Guarded(nb, torch.bfloat16, dev), X.Guarded(nb, torch.bfloat16, dev)
    t, o = X.Guarded(ns, f32, dev), X.Guarded(grid * ns, f32, dev)

    def body():
        x.all_reduce(a.view, "sum")
        x.all_reduce_twoshot(b.view, "avg", bo.view)
        x.site_probe(1, t.view, o.view, grid)

    def load():
        xa, xb, xt = run.inputs(na, f32), run.inputs(nb, torch.bfloat16), run.inputs(ns, f32)
        a.load(xa[run.rank])
        b.load(xb[run.rank])
        t.load(xt[run.rank])
        bo.buf.copy_(X.sentinel(bo.total, torch.bfloat16))  # the outputs back to the sentinel
        o.buf.copy_(X.sentinel(o.total, f32))
        return xa, xb, xt

    def check(xa, xb, xt, what):
        run.done(what)
        c = a.check(X.reduce(xa, "sum", f32), (what, "one-shot"))
        c += bo.check(X.reduce_twoshot(xb, "avg", torch.bfloat16), (what, "two-shot"))
        b.check(xb[run.rank], (what, "two-shot input"))
        c += o.check(X.site_sum(xt).repeat(grid), (what, "site"))
        for key, g_ in (("a", a), ("b", bo), ("s", o)):
            run.record("graph", key, g_, 0)
        run.count["graph"] += c

    run.count["graph"] = 0
    ins = load()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()  # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(s)
    check(*ins, "warm-up")
    ins = load()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    for r in range(4):
        ins = load()
        g.replay()
        check(*ins, ("replay", r))


# ------------------------------------------------------------------------------ fused AMP/SGD step
def sgd(run, C):
    from . import _sgd_ref as R
    from . import test_sgd_amp_exact_gpu as T

    x, W, rank, dev = run.x, run.world, run.rank, run.dev
    NAN, INF = float("nan"), float("inf")
    GBI = (2.0, 0.5, 2)

    def fused(st, h, first=(), amp=True, prechk=None, slab=None, slab_out=None):
        n = len(st.sizes)
        C.optim.amp_sgd_fused(st.P.views, st.G.views, st.B.views, h["lr"], h["momentum"], h["dampening"],
                              h["weight_decay"], h["nesterov"], h["maximize"], list(first) or [0] * n,
                              st.scale if amp else None, st.tracker if amp else None, st.found if amp else None,
                              GBI[0], GBI[1], GBI[2], st.sync, x, slab=slab, slab_out=slab_out, prechk=prechk)

    def finish(st, what):
        torch.cuda.synchronize()
        assert x.error() == 0, (what, x.error_string(), x.debug_state(2.0))
        assert int(st.sync[3]) == 0, (what, st.sync.tolist())
        st.check_pads()

    def keep(what, got, keys="pgb"):
        for k in keys:
            for i, t in enumerate(got[k]):
                run.out[f"sgd:{what}:{k}{i}"] = t.numpy().tobytes()
                run.count["sgd"] = run.count.get("sgd", 0) + t.numel()

    def step(st, what, grads_all, h, exact, first=(), amp=True, found_inf=0.0, barrier=True, **kw):
        """Launch from the loaded state (this rank's gradients in it) and compare with the
        reference step on the rank-ordered fp32 average of every rank's gradients."""
        before = st.read()
        for a_, b_ in zip(before["g"], grads_all[rank]):
            T.same_bits(a_, b_, "uploaded grad")
        scale, trk, s0 = float(st.scale), int(st.tracker), int(st.sync[0])
        fused(st, h, first, amp, **kw)
        finish(st, what)
        got = st.read()
        avg = X.xg_average(grads_all)
        ref = R.amp_step(before["p"], avg, before["b"], first, scale=scale if amp else None, tracker=trk,
                         found_inf=found_inf, growth=GBI[0], backoff=GBI[1], interval=GBI[2], exact=exact, **h)
        T.check_step(got, ref, dict(before, g=avg), exact, "amp_sgd_fused (xgmi)")
        if amp:
            T.check_scalars(st, ref, s0 + int(barrier))  # three workgroups: one barrier generation
        else:
            assert int(st.sync[0]) == s0
        keep(what, got)
        return ref, got

    def inject(grads_all, r, t, i, val):
        out = [[g.clone() for g in gs] for gs in grads_all]
        out[r][t][i] = val
        return out

    sizes = list(SGD_SIZES)
    assert sum((n + 3) // 4 for n in sizes) == 525
    st = T.State(sizes, dev)
    first = [1, 0, 1, 0, 0]

    if W == 2:
        # every value exact in fp32, the average included (1/2): bitwise, two consecutive steps
        for oi, opt in enumerate([(False, False, False, False, False), (True, True, False, False, True),
                                  (True, False, True, True, False)]):
            assert opt in R.OPTION_GRID
            h = R.options(R.DYADIC, *opt)
            p, _, b = R.dyadic(sizes, 51 + oi)
            ga = [R.dyadic_grads(sizes, 60 + 10 * oi + r) for r in range(W)]
            st.load(p, ga[rank], b, scale=1024.0)
            step(st, f"dyadic{oi}.1", ga, h, True, first=first if opt[0] else ())
            assert float(st.scale) == 1024.0 and int(st.tracker) == 1
            ga = [R.dyadic_grads(sizes, 65 + 10 * oi + r) for r in range(W)]
            st.G.load(ga[rank])
            step(st, f"dyadic{oi}.2", ga, h, True)
            assert float(st.scale) == 2048.0 and int(st.tracker) == 0

    hf = R.options(R.FLOAT, True, True, False, False, True)
    p, _, b = R.normal(sizes, 71, scale=1000.0)
    ga = [R.normal(sizes, 72 + r, scale=1000.0)[1] for r in range(W)]
    # floats: within the counted bound of _sgd_ref around the exact fp32 average
    st.load(p, ga[rank], b, scale=1000.0)
    step(st, "float.1", ga, hf, False, first=first)
    ga2 = [R.normal(sizes, 82 + r, scale=1000.0)[1] for r in range(W)]
    st.G.load(ga2[rank])
    step(st, "float.2", ga2, hf, False)

    # one non-finite scaled gradient on ONE rank: the first element, a ragged tail (the last
    # granule holds one element), both sides of the first workgroup boundary (granule 255 | 256)
    places = [(0, 0), (3, 1024), (2, 979), (2, 980)]
    assert (11 + 979 // 4, 11 + 980 // 4) == (255, 256) and sizes[3] % 4 == 1
    k = 0
    for t, i in places:
        for val in (NAN, INF, -INF):
            bad_rank = k % W
            k += 1
            gi = inject(ga, bad_rank, t, i, val)
            st.load(p, gi[rank], b, scale=1000.0, tracker=1)
            ref, _ = step(st, f"nonfinite{k}", gi, hf, False, first=first)
            assert ref["found"] and float(st.scale) == 500.0 and int(st.tracker) == 0
    # two ranks each hold a finite 3e38: the AVERAGE is checked, so the step is skipped
    gi = inject(inject(ga, 0, 2, 500, 3e38), 1, 2, 500, 3e38)
    assert all(bool(torch.isfinite(g).all()) for gs in gi for g in gs)
    st.load(p, gi[rank], b, scale=1000.0, tracker=1)
    ref, got = step(st, "overflowing sum", gi, hf, False, first=first)
    assert ref["found"] and float(st.scale) == 500.0 and bool(got["g"][2][500].isinf())

    # plain mode (no scale): the average is stored and applied, no skip, no scale
    hd = R.options(R.DYADIC, True, True, False, False, True)
    if W == 2:
        p2, _, b2 = R.dyadic(sizes, 91, scale=1.0)
        gp = [R.dyadic_grads(sizes, 92 + r, scale=1.0) for r in range(W)]
        st.load(p2, gp[rank], b2)
        step(st, "plain", gp, hd, True, first=first, amp=False)
    gpl = [R.normal(sizes, 95 + r, scale=1.0)[1] for r in range(W)]
    st.load(p, gpl[rank], b, scale=7.0, tracker=1)
    step(st, "plain float", gpl, hf, False, first=first, amp=False)
    assert float(st.scale) == 7.0 and int(st.tracker) == 1

    # pre-checked mode: the producers' words decide, no grid barrier.  All clean: the barrier
    # mode's result, bitwise
    pd, _, bd = R.dyadic(sizes, 101)
    gd = [R.normal(sizes, 102 + r, scale=1024.0)[1] for r in range(W)]
    st.load(pd, gd[rank], bd, scale=1024.0, tracker=1)
    _, base = step(st, "barrier mode", gd, hf, False, first=first)
    base_scalars = (float(st.scale), int(st.tracker))
    st.load(pd, gd[rank], bd, scale=1024.0, tracker=1)
    _, pre = step(st, "pre-checked clean", gd, hf, False, first=first, barrier=False,
                  prechk=T._words([0] * 300, 1024.0))
    for key in "pgb":
        for i, (u, v) in enumerate(zip(pre[key], base[key])):
            T.same_bits(u, v, f"pre-checked vs barrier mode {T.NAMES[key]}[{i}]")
    assert (float(st.scale), int(st.tracker)) == base_scalars == (2048.0, 0)
    # one rank's word set, finite gradients everywhere: that rank pushes NaN in place of its
    # values, so EVERY workgroup of EVERY rank skips -- whichever lane read the word (word 299 is
    # read by lane 43; the last workgroup has 13 granules)
    for j, word in enumerate((0, 4, 299)):
        flagged = j % W
        w = [0] * 300
        if rank == flagged:
            w[word] = 1
        st.load(pd, gd[rank], bd, scale=1024.0, tracker=1)
        before = st.read()
        s0 = int(st.sync[0])
        fused(st, hf, first, prechk=T._words(w, 1024.0))
        finish(st, ("pre-checked, flagged", word))
        got = st.read()
        for key in "pb":  # (the stored gradients of this skipped step are the poisoned averages: unspecified)
            for i, (u, v) in enumerate(zip(got[key], before[key])):
                T.same_bits(u, v, f"word {word} set on rank {flagged}: {T.NAMES[key]}[{i}] of a skipped step")
        assert (float(st.scale), int(st.tracker), float(st.found)) == (512.0, 0, 0.0), (word, flagged)
        assert int(st.sync[0]) == s0
        keep(f"flagged{word}", got, "pb")

    # slab source: the last tensor's gradient is the column sums of a [rows][36] slab (three slab
    # workgroups of 16 columns, the last with 4), exchanged one granule per element.  Dyadic rows
    # whose sums are the dyadic gradient: exact in any association, so each rank pushes the bits
    # of the pre-summed gradient and the step is bitwise the step fed that gradient at any W.
    # The pre-summed step itself against _sgd_ref: bitwise at W = 2, within the counted bound at
    # W = 3 (the average by 1/3 rounds)
    ssz = list(SLAB_SIZES)
    ss = T.State(ssz, dev)
    for rows in (5, 37):
        for amp in (True, False):
            sc = 1024.0 if amp else 1.0
            ps, _, bs = R.dyadic(ssz, 110 + rows, scale=sc)
            gs = [R.dyadic_grads(ssz, 120 + rows + r, scale=sc) for r in range(W)]
            ss.load(ps, gs[rank], bs, scale=sc)
            _, want = step(ss, f"pre-summed{rows}{amp}", gs, hd, W == 2, first=first, amp=amp)
            want_s = (float(ss.scale), int(ss.tracker))
            slab = R.slab_rows(gs[rank][4], rows, 130 + rows + rank, sc).to(dev)
            mine = [g.clone() for g in gs[rank]]
            mine[4] = torch.full((36,), 12345.0)  # the region is written, never read
            ss.load(ps, mine, bs, scale=sc)
            s0 = int(ss.sync[0])
            fused(ss, hd, first, amp, slab=slab, slab_out=ss.G.views[4])
            finish(ss, ("slab", rows, amp))
            got = ss.read()
            for key in "pgb":
                for i, (u, v) in enumerate(zip(got[key], want[key])):
                    T.same_bits(u, v, f"slab rows={rows} amp={amp}: {T.NAMES[key]}[{i}] vs the pre-summed step")
            assert (float(ss.scale), int(ss.tracker)) == want_s and int(ss.sync[0]) == s0 + int(amp)
            keep(f"slab{rows}{amp}", got)
    return {k: v for k, v in T.RATIOS.items()}


def worker(rank, world, port, mode, q):
    try:
        if world >= 3:  # several ranks on one card: one HW queue each (runtime/device.shared_gpu_env)
            os.environ["GPU_MAX_HW_QUEUES"] = "1"
        from ddp_practice_amd import _ext

        C = _ext.load()
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        store = torch.distributed.TCPStore("127.0.0.1", port, world, False, timedelta(seconds=60))  # parent serves
        from ddp_practice_amd.parallel.comm import open_xgmi

        x, err = open_xgmi(rank, world, dev, store, "t", MAX_BYTES, 20.0, TS_BYTES)
        assert x is not None, err
        x2 = None
        if mode == "twoshot":
            x2, err = open_xgmi(rank, world, dev, store, "t2", MAX_BYTES, 20.0, 0)
            assert x2 is not None, err
        x.set_twoshot_blocks(TS_GRID)
        store.set(f"ready{rank}", "1")
        store.wait([f"ready{r}" for r in range(world)])
        run = Run(rank, world, dev, x)
        t0 = time.time()
        extra = None
        if mode == "oneshot":
            oneshot(run)
        elif mode == "twoshot":
            twoshot(run, C, x2)
        elif mode == "sites":
            sites(run)
        elif mode == "graph":
            assert world == 2
            graph(run)
        elif mode == "sgd":
            extra = sgd(run, C)
        else:
            raise ValueError(mode)
        torch.cuda.synchronize()
        assert x.error() == 0, x.error_string()
        secs = time.time() - t0
        store.set(f"done{rank}", "1")
        store.wait([f"done{r}" for r in range(world)])
        if x2 is not None:
            x2.close()
        x.close()
        q.put((rank, "ok", {"out": run.out, "count": run.count, "calls": run.call, "seconds": secs, "extra": extra}))
    except Exception:  # pragma: no cover - reported to the parent
        q.put((rank, "err", traceback.format_exc()))
    finally:
        q.close()
        q.join_thread()
        os._exit(0)
