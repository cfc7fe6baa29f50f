"""dev helper: pcc_fpfh_descriptors_batch against the loop it replaces (processFPFH per cluster, reference src/comparator.cpp:824-875).
In ONE process, on one context handle and ONE kept loop handle, the two versions alternating:
  batch   one pcc_fpfh_descriptors_batch for all clusters
  loop    set_input + fpfh_descriptors per cluster on one re-pointed handle (the only path before the batch call)
from host memory (NumPy arrays in, NumPy arrays out) and from device memory (CUDA tensors in and out), points only.
Workloads, from synth.rift_cloud at the density of the test scenes, all in one corner of space: 2 x 30 clusters of 300 points,
2 x 30 of 3000, and a mixed set of 60 clusters of 20 ... 5000 points.  Then:
  two CSRs  the same batch with normal_radius = fpfh_radius + 1e-11 (the two-CSR path: launch_normals_csr over a CSR of its own)
            against normal_radius = fpfh_radius (one CSR, the prefix is the whole row): same rows, same work but the second CSR
  sweep     PCC_OPT_FPFH_BATCH_BRUTE_MAX = 2048 / 4096 / 8192 / 16384 on the mixed workload, and ONE cluster alone of those sizes
            through either route
  chain     FPFH batch -> match_fpfh_batch, device-resident against through-the-host
Outputs are compared (bits and indices) before anything is timed.  Host clock around calls that end in a synchronise; a sample
is the mean over a window of at least --window seconds; every figure is the median of --repeats samples with their min .. max.
usage: exp_fpfh_batch.py [--window SECONDS] [--repeats N] [--out FILE]   (FILE: default profiles/fpfh_batch_exp.txt)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pointcloudcomparator_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=0.1)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_batch_exp.txt"))
args = ap.parse_args()
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def cloud(n, seed):
    return synth.rift_cloud(n, seed, extent=0.12 * (n / 600.0) ** (1.0 / 3.0))[0]


def sample(fn):
    """milliseconds per call of fn over a window of at least args.window seconds (fn ends in a synchronise)"""
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= args.window:
            return dt / n * 1e3


def alternate(fns):
    """{name: (median, min, max)} of args.repeats samples each, the versions taking turns"""
    for fn in fns.values():
        fn()  # warm-up
    got = {name: [] for name in fns}
    for _ in range(args.repeats):
        for name, fn in fns.items():
            got[name].append(sample(fn))
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in got.items()}


def fmt(stat):
    return f"{stat[0]:8.3f} ({stat[1]:.3f} .. {stat[2]:.3f})"


def host(x):
    return x.cpu().numpy() if capi._is_torch(x) else x


def same(a, b):
    ah, ai, bh, bi = host(a[0]), host(a[1]), host(b[0]), host(b[1])
    return np.array_equal(ai, bi) and ah.shape == bh.shape and (ah.view(np.uint32) == bh.view(np.uint32)).all()


rng = np.random.default_rng(20251017)
mixed = np.round(np.exp(rng.uniform(np.log(20), np.log(5000), 60))).astype(int)
WORKLOADS = {"2x30x300": [300] * 60, "2x30x3000": [3000] * 60, "mixed60": [int(v) for v in mixed]}

ctx = capi.Index(np.zeros((1, 3), np.float32), engine=capi.ENGINE_BRUTE, device=0)
loop_ix = capi.Index(cloud(300, 1), engine=capi.ENGINE_GRID, device=0)
say(f"pcc_fpfh_descriptors_batch against the loop of set_input + fpfh_descriptors on one kept handle; ms per call, median (min .. max) of "
    f"{args.repeats} samples of >= {args.window} s, alternating; {torch.cuda.get_device_name(0)}")
say(f"{'workload':10s} {'memory':6s} {'clusters':>8s} {'points':>7s} {'kept':>7s} | {'batch':>28s} | {'loop':>28s} | loop / batch")
staged = {}
for name, sizes in WORKLOADS.items():
    pts = [cloud(n, 500 + k) for k, n in enumerate(sizes)]
    offsets = np.cumsum([0] + sizes)
    allp = np.concatenate(pts)
    dev = torch.from_numpy(allp).cuda()
    dpts = [dev[offsets[k]:offsets[k + 1]] for k in range(len(sizes))]
    staged[name] = (allp, dev, offsets)

    def batch_host():
        return ctx.fpfh_descriptors_batch(allp, offsets)

    def loop_host():
        out = []
        for p in pts:
            loop_ix.set_input(p)
            out.append(loop_ix.fpfh_descriptors())
        return out

    def batch_dev():
        out = ctx.fpfh_descriptors_batch(dev, offsets)
        torch.cuda.synchronize()
        return out

    def loop_dev():
        out = []
        for p in dpts:
            loop_ix.set_input(p)
            out.append(loop_ix.fpfh_descriptors())
        torch.cuda.synchronize()
        return out

    ref = loop_host()
    for what, fn in (("batch, host", batch_host), ("batch, device", batch_dev), ("loop, device", loop_dev)):
        got = fn()
        bad = [k for k in range(len(sizes)) if not same(got[k], ref[k])]
        assert not bad, f"{name}: {what}: clusters {bad[:5]} differ from the loop from host memory"
    kept = sum(len(r[1]) for r in ref)
    for mem, fns in (("host", {"batch": batch_host, "loop": loop_host}), ("device", {"batch": batch_dev, "loop": loop_dev})):
        t = alternate(fns)
        say(f"{name:10s} {mem:6s} {len(sizes):8d} {sum(sizes):7d} {kept:7d} | {fmt(t['batch'])} | {fmt(t['loop'])} | {t['loop'][0] / t['batch'][0]:.2f}")

say()
say("one CSR (normal_radius = fpfh_radius = 0.05: the prefix is the whole row) against two (normal_radius = 0.05 + 1e-11), device memory")
say(f"{'workload':10s} | {'one CSR':>28s} | {'two CSRs':>28s} | two / one")
for name in WORKLOADS:
    allp, dev, offsets = staged[name]

    def one():
        out = ctx.fpfh_descriptors_batch(dev, offsets, 0.05, 0.05)
        torch.cuda.synchronize()
        return out

    def two():
        out = ctx.fpfh_descriptors_batch(dev, offsets, 0.05 + 1e-11, 0.05)
        torch.cuda.synchronize()
        return out

    a = one()
    assert int(ctx.stats()[2]) == 1
    b = two()
    assert int(ctx.stats()[2]) == 2
    assert np.float32((0.05 + 1e-11) ** 2) == np.float32(0.05 ** 2)  # the same rows: the results must agree
    assert all(same(x, y) for x, y in zip(a, b)), f"{name}: one CSR and two give different results"
    t = alternate({"one": one, "two": two})
    say(f"{name:10s} | {fmt(t['one'])} | {fmt(t['two'])} | {t['two'][0] / t['one'][0]:.2f}")

say()
default = ctx.get_option(capi.OPT_FPFH_BATCH_BRUTE_MAX)
say(f"PCC_OPT_FPFH_BATCH_BRUTE_MAX (default {default:.0f}) on mixed60, device memory: clusters on the work handle, ms")
allp, dev, offsets = staged["mixed60"]
sizes = WORKLOADS["mixed60"]
LIMITS = (2048, 4096, 8192, 16384)


def with_limit(limit, pts, off):
    def fn():
        ctx.set_option(capi.OPT_FPFH_BATCH_BRUTE_MAX, limit)
        out = ctx.fpfh_descriptors_batch(pts, off)
        torch.cuda.synchronize()
        return out
    return fn


ref = with_limit(default, dev, offsets)()
for limit in LIMITS:
    assert all(same(x, y) for x, y in zip(with_limit(limit, dev, offsets)(), ref)), f"limit {limit} changes a result"
t = alternate({limit: with_limit(limit, dev, offsets) for limit in LIMITS})
for limit in LIMITS:
    say(f"  limit {limit:6d}: {sum(n > limit for n in sizes):2d} of {len(sizes)} clusters on the work handle | {fmt(t[limit])}")
say("one cluster alone, device memory: through the batch kernels against the work handle, ms")
say(f"{'points':>7s} | {'batch kernels':>28s} | {'work handle':>28s} | work / batch")
for n in LIMITS:
    lone = torch.from_numpy(cloud(n, 17)).cuda()
    off = np.array([0, n])
    brute, work = with_limit(1 << 30, lone, off), with_limit(0, lone, off)
    assert same(brute()[0], work()[0]), f"{n} points: the routes differ"
    t = alternate({"brute": brute, "work": work})
    say(f"{n:7d} | {fmt(t['brute'])} | {fmt(t['work'])} | {t['work'][0] / t['brute'][0]:.2f}")
ctx.set_option(capi.OPT_FPFH_BATCH_BRUTE_MAX, default)

say()
say("the chain FPFH batch -> match_fpfh_batch over the 30 cluster pairs of 2x30x300, ms")
allp, dev, offsets = staged["2x30x300"]


def chain_device():
    d = ctx.fpfh_descriptors_batch(dev, offsets)
    return ctx.match_fpfh_batch([(d[k][0], d[30 + k][0]) for k in range(30)])


def chain_host():
    d = ctx.fpfh_descriptors_batch(allp, offsets)
    return ctx.match_fpfh_batch([(d[k][0], d[30 + k][0]) for k in range(30)])


a, b = chain_device(), chain_host()
assert all(np.array_equal(x, y) for x, y in zip(a, b)), "the chain's two forms differ"
t = alternate({"device": chain_device, "host": chain_host})
say(f"  device-resident descriptors {fmt(t['device'])} | through the host {fmt(t['host'])} | host / device {t['host'][0] / t['device'][0]:.2f}")
loop_ix.close()
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(LINES) + "\n")
