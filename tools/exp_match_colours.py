"""dev helper: pcc_match_colour_elements against the path it replaces, per COMPARISON (the colour counts of the match loop,
reference src/comparator.cpp:1379-1509).  In ONE process, on one context handle, alternating:
  new     one pcc_match_colour_elements call over the record arrays of both scenes and the match table, from host memory
          (NumPy records) and from device memory (torch tensors)
  old     the parent commit's path: the host gather of the matched clusters -- both clusters of every match, one cloud per
          match and side -- plus one pcc_region_growing_rgb_batch call; for the device case the download of the two record
          arrays in front of it.  Timed twice: the difference between its two columns is the run-to-run spread the other
          differences have to beat
Clusters are cut from tools/exp_rgb.py's painted room as in tools/exp_rgb_batch.py, 30 per scene.  Workloads: 2 x 30 clusters of
300 points, 2 x 30 of 3000, and 60 clusters drawn from 11 ... 8000 points.  Match tables: `distinct` (matches[i] = i) and
`repeat` (every third row names cluster 0 of scene 2: a third of the matches repeat one cluster).  The table is checked against
the old path's counts before anything is timed.  Host clock around calls that end in a synchronise; every shape warmed up; each
figure from a window of at least --window seconds.
usage: exp_match_colours.py [--window SECONDS]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from pointcloudcomparator_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=0.2)
args = ap.parse_args()

BASE = np.array([[180, 170, 150], [90, 60, 40], [40, 90, 160], [200, 40, 40], [60, 160, 80]], np.int32)
rng = np.random.default_rng(20261020)
ROOM = synth.room_cloud(300000, synth.SEED_A)
_which = (np.floor(ROOM[:, 0] * 1.3).astype(int) + np.floor(ROOM[:, 1] * 0.9).astype(int) * 2) % len(BASE)
ROOM_RGB = np.clip(BASE[_which] + np.random.default_rng(8).integers(-2, 3, (len(ROOM), 3)), 0, 255).astype(np.uint8)


def cluster(n):
    """(n, 8) float32 pcl::PointXYZRGB records of the n points of the room nearest to one of its points"""
    centre = ROOM[rng.integers(len(ROOM))]
    d = ((ROOM - centre) ** 2).sum(1)
    take = np.sort(np.argpartition(d, n - 1)[:n])
    rec = np.zeros((n, 8), np.float32)
    rec[:, :3] = ROOM[take]
    rec[:, 3] = 1.0
    rec[:, 4] = synth.pack_rgb(ROOM_RGB[take]).view(np.float32)
    return rec


def scene(sizes):
    parts = [cluster(n) for n in sizes]
    return np.ascontiguousarray(np.concatenate(parts)), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def window(fn, seconds):
    """milliseconds per call of fn over a window of at least `seconds` (fn ends in a synchronise)"""
    fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e3


mixed = np.round(np.exp(rng.uniform(np.log(11), np.log(8000), 60))).astype(int)
WORKLOADS = {"2x30x300": [300] * 60, "2x30x3000": [3000] * 60, "mixed60": [int(v) for v in mixed]}
TABLES = {"distinct": np.arange(30, dtype=np.int32), "repeat": np.array([0 if i % 3 == 0 else i for i in range(30)], np.int32)}

ctx = capi.Index(np.zeros((1, 3), np.float32), engine=capi.ENGINE_BRUTE, device=0)
print(f"{'workload':9s} {'table':8s} {'points':>7s} {'segmented':>9s} {'saved':>5s} {'sweeps':>6s} | {'new host':>9s} {'old host':>9s} {'old again':>9s} | "
      f"{'new dev':>9s} {'old dev':>9s} {'old again':>9s} | old / new host, device   (ms per comparison)")
for name, sizes in WORKLOADS.items():
    rec1, off1 = scene(sizes[:30])
    rec2, off2 = scene(sizes[30:])
    dev1, dev2 = torch.from_numpy(rec1).cuda(), torch.from_numpy(rec2).cuda()
    for table, matches in TABLES.items():

        def old(r1, r2):
            clouds = []
            for i, j in enumerate(matches):  # the host gather: both clusters of every match
                clouds.append(r1[off1[i]:off1[i + 1]])
                clouds.append(r2[off2[j]:off2[j + 1]])
            res = ctx.region_growing_rgb_batch(clouds)
            return np.array([r[1] for r in res], np.int32).reshape(-1, 2)

        def old_host():
            return old(rec1, rec2)

        def old_dev():
            return old(dev1.cpu().numpy(), dev2.cpu().numpy())  # (the download of the cluster clouds the old path needs)

        def new_host():
            return ctx.match_colour_elements(rec1, off1, rec2, off2, matches)

        def new_dev():
            return ctx.match_colour_elements(dev1, off1, dev2, off2, matches)

        want = old_host()
        for fn in (new_host, new_dev, old_dev):
            assert np.array_equal(fn(), want), f"{name} / {table}: {fn.__name__} differs from the old path"
        new_dev()
        st = ctx.stats()
        t = {k: 0.0 for k in ("nh", "nd", "oh0", "oh1", "od0", "od1")}
        for rep in range(2):  # alternating, two rounds; the new figures are the means of their two windows
            t["nh"] += window(new_host, args.window) / 2
            t[f"oh{rep}"] = window(old_host, args.window)
            t["nd"] += window(new_dev, args.window) / 2
            t[f"od{rep}"] = window(old_dev, args.window)
        print(f"{name:9s} {table:8s} {int(st[2] + st[3]):7d} {int(st[4]):9d} {int(st[5]):5d} {int(st[7]):6d} | {t['nh']:9.3f} {t['oh0']:9.3f} {t['oh1']:9.3f} | "
              f"{t['nd']:9.3f} {t['od0']:9.3f} {t['od1']:9.3f} | {min(t['oh0'], t['oh1']) / t['nh']:.2f} {min(t['od0'], t['od1']) / t['nd']:.2f}", flush=True)
ctx.close()
