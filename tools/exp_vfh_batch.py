"""dev helper: pcc_vfh_descriptors_batch against the loop it replaces (processVHF per cluster, reference src/comparator.cpp:482-516).
In ONE process, on one context handle and ONE kept loop handle, the two versions alternating:
  batch   one pcc_vfh_descriptors_batch for all clusters
  loop    set_input + vfh_descriptor per cluster on one re-pointed handle (the only path before the batch call: the yardstick)
from host memory (NumPy arrays in, NumPy arrays out) and from device memory (CUDA tensors in and out), points only.
Workloads, from synth.rift_cloud at the density of the test scenes, all in one corner of space: 2 x 30 clusters of 300 points,
2 x 30 of 3000, and a mixed set of 60 clusters of 20 ... 5000 points (tools/exp_fpfh_batch.py's).  Then:
  kernels   the per-kernel split of the batch call from pcc_index_enable_timing: the centroid chains, the votes, the rebuild of
            the bins, and the whole call first to last kernel, device memory
  growth    the call with 10 and with 60 clusters of one size: what does not grow with the number of clusters
  sweep     PCC_OPT_VFH_BATCH_BRUTE_MAX = 2048 / 4096 / 8192 / 16384 on the mixed workload, and ONE cluster alone of those sizes
            through either route
  chain     batch(A), batch(B), match_vfh: device-resident against through the host
The batch is checked to carry the loop's bits before anything is timed.  Host clock around calls that end in a synchronise; a
sample is the mean over a window of at least --window seconds; every figure is the median of --repeats samples with their
min .. max.
usage: exp_vfh_batch.py [--window SECONDS] [--repeats N] [--out FILE]   (FILE: default profiles/vfh_batch_exp.txt)"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vfh_batch_exp.txt"))
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
    return x.cpu().numpy() if capi._is_torch(x) else np.asarray(x)


def same(a, b):
    ah, bh = host(a), host(b)
    return ah.shape == bh.shape and (ah.view(np.uint32) == bh.view(np.uint32)).all()


rng = np.random.default_rng(20251017)
mixed = np.round(np.exp(rng.uniform(np.log(20), np.log(5000), 60))).astype(int)
WORKLOADS = {"2x30x300": [300] * 60, "2x30x3000": [3000] * 60, "mixed60": [int(v) for v in mixed]}

ctx = capi.Index(np.zeros((1, 3), np.float32), engine=capi.ENGINE_BRUTE, device=0)
loop_ix = capi.Index(cloud(300, 1), engine=capi.ENGINE_GRID, device=0)
say(f"pcc_vfh_descriptors_batch against the loop of set_input + vfh_descriptor on one kept handle; ms per call, median (min .. max) of "
    f"{args.repeats} samples of >= {args.window} s, alternating; {torch.cuda.get_device_name(0)}")
say(f"{'workload':10s} {'memory':6s} {'clusters':>8s} {'points':>7s} | {'batch':>28s} | {'loop':>28s} | loop / batch")
staged = {}


def stage(sizes, seed0=500):
    pts = [cloud(n, seed0 + k) for k, n in enumerate(sizes)]
    offsets = np.cumsum([0] + list(sizes))
    allp = np.concatenate(pts)
    dev = torch.from_numpy(allp).cuda()
    return pts, allp, dev, offsets


def batch_fn(pts, offsets):
    def fn():
        out = ctx.vfh_descriptors_batch(pts, offsets)
        torch.cuda.synchronize()
        return out
    return fn


def loop_fn(clusters):
    def fn():
        out = []
        for p in clusters:
            loop_ix.set_input(p)
            out.append(loop_ix.vfh_descriptor())
        torch.cuda.synchronize()
        return out
    return fn


for name, sizes in WORKLOADS.items():
    pts, allp, dev, offsets = stage(sizes)
    dpts = [dev[offsets[k]:offsets[k + 1]] for k in range(len(sizes))]
    staged[name] = (allp, dev, offsets)
    batch_host, batch_dev = batch_fn(allp, offsets), batch_fn(dev, offsets)
    loop_host, loop_dev = loop_fn(pts), loop_fn(dpts)
    ref = loop_host()
    assert len({host(r).tobytes() for r in ref}) > len(sizes) // 2, f"{name}: the loop's descriptors do not tell the clusters apart"
    for what, fn in (("batch, host", batch_host), ("batch, device", batch_dev), ("loop, device", loop_dev)):
        got = fn()
        bad = [k for k in range(len(sizes)) if not same(got[k], ref[k])]
        assert not bad, f"{name}: {what}: clusters {bad[:5]} differ from the loop from host memory"
    for mem, fns in (("host", {"batch": batch_host, "loop": loop_host}), ("device", {"batch": batch_dev, "loop": loop_dev})):
        t = alternate(fns)
        say(f"{name:10s} {mem:6s} {len(sizes):8d} {sum(sizes):7d} | {fmt(t['batch'])} | {fmt(t['loop'])} | {t['loop'][0] / t['batch'][0]:.2f}")

say()
say("the kernels of one batch call, device memory, us (pcc_index_enable_timing, mean of 20 calls): the centroid chains (one wave per cluster, "
    "all clusters side by side), the votes, the rebuild of the bins; first to last kernel of the call")
say(f"{'workload':10s} {'largest':>7s} | {'chains':>8s} {'votes':>8s} {'bins':>8s} | {'call':>8s} | chains / largest, ns a link")
for name, sizes in WORKLOADS.items():
    allp, dev, offsets = staged[name]
    fn = batch_fn(dev, offsets)
    fn()
    ctx.enable_timing(2)
    for _ in range(20):
        fn()
    ms = ctx.timing()
    ctx.enable_timing(0)
    say(f"{name:10s} {max(sizes):7d} | {ms[4] * 1e3:8.1f} {ms[0] * 1e3:8.1f} {ms[1] * 1e3:8.1f} | {ms[2] * 1e3:8.1f} | {ms[4] * 1e6 / max(sizes):.1f}")
lone8192 = torch.from_numpy(cloud(8192, 17)).cuda()
fn = batch_fn(lone8192, np.array([0, 8192]))
fn()
ctx.enable_timing(2)
for _ in range(20):
    fn()
ms = ctx.timing()
ctx.enable_timing(0)
say(f"{'1x8192':10s} {8192:7d} | {ms[4] * 1e3:8.1f} {ms[0] * 1e3:8.1f} {ms[1] * 1e3:8.1f} | {ms[2] * 1e3:8.1f} | {ms[4] * 1e6 / 8192:.1f}")

say()
say("10 against 60 clusters of one size, device memory, ms: what does not grow with the number of clusters")
say(f"{'points':>7s} | {'batch, 10':>28s} | {'batch, 60':>28s} | 60 / 10 | {'loop, 10':>28s} | {'loop, 60':>28s} | 60 / 10")
for n in (300, 3000):
    fns = {}
    for k in (10, 60):
        pts, allp, dev, offsets = stage([n] * k, seed0=900)
        fns[f"batch{k}"] = batch_fn(dev, offsets)
        fns[f"loop{k}"] = loop_fn([dev[offsets[c]:offsets[c + 1]] for c in range(k)])
    t = alternate(fns)
    say(f"{n:7d} | {fmt(t['batch10'])} | {fmt(t['batch60'])} | {t['batch60'][0] / t['batch10'][0]:7.2f} | {fmt(t['loop10'])} | {fmt(t['loop60'])} | "
        f"{t['loop60'][0] / t['loop10'][0]:.2f}")

say()
default = ctx.get_option(capi.OPT_VFH_BATCH_BRUTE_MAX)
say(f"PCC_OPT_VFH_BATCH_BRUTE_MAX (default {default:.0f}) on mixed60, device memory: clusters on the work handle, ms")
allp, dev, offsets = staged["mixed60"]
sizes = WORKLOADS["mixed60"]
LIMITS = (2048, 4096, 8192, 16384)


def with_limit(limit, pts, off):
    def fn():
        ctx.set_option(capi.OPT_VFH_BATCH_BRUTE_MAX, limit)
        out = ctx.vfh_descriptors_batch(pts, off)
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
ctx.set_option(capi.OPT_VFH_BATCH_BRUTE_MAX, default)

say()
say("the chain batch(A), batch(B), match_vfh over the 30 x 30 cluster pairs of 2x30x300, ms")
allp, dev, offsets = staged["2x30x300"]
half = 30 * 300


def chain_device():
    a, _ = ctx.vfh_descriptors_batch(dev[:half], offsets[:31], return_packed=True)
    b, _ = ctx.vfh_descriptors_batch(dev[half:], offsets[30:] - half, return_packed=True)
    out = ctx.match_vfh(a, b)
    torch.cuda.synchronize()
    return out


def chain_host():
    a, _ = ctx.vfh_descriptors_batch(allp[:half], offsets[:31], return_packed=True)
    b, _ = ctx.vfh_descriptors_batch(allp[half:], offsets[30:] - half, return_packed=True)
    return ctx.match_vfh(a, b)


a, b = host(chain_device()), chain_host()
assert a.shape == (30, 30) and np.array_equal(a.view(np.uint64), b.view(np.uint64)), "the chain's two forms differ"
t = alternate({"device": chain_device, "host": chain_host})
say(f"  device-resident descriptors {fmt(t['device'])} | through the host {fmt(t['host'])} | host / device {t['host'][0] / t['device'][0]:.2f}")
loop_ix.close()
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(LINES) + "\n")
