#!/usr/bin/env python3
"""What the plane-removal loop of the -e path costs in three forms, per scene, on one handle (EXPERIMENTS.md):
  (a) the loop as it was: pcc_sac_plane on a host array per turn + the compaction on the host (np.delete)
  (b) pcc_plane_removal from host memory (one upload, the compaction on the device)
  (c) pcc_plane_removal from device memory
Scenes: a room of five planes plus clutter at 10^5 and 10^6 points, and the 33 000-point two-plane scene of
tests/test_sac_gpu.py.  Warm; per run a host clock around a call that begins and ends with the handle's stream idle; (a), (b)
and (c) interleaved run by run; median [min max] of --runs runs.  The three forms must give the same planes and the same
remaining points, or the tool fails."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))


def room(n, seed=7, noise=0.005):
    """floor, ceiling and three walls of a 4 x 3 x 2.5 room holding 20 / 18 / 16 / 14 / 12 % of the points, 20 % clutter inside:
    five planes go before 30 % or less remain"""
    rng = np.random.default_rng(seed)
    parts = []
    for share, axis, at, ext in ((0.20, 2, 0.0, (4, 3)), (0.18, 2, 2.5, (4, 3)), (0.16, 0, 0.0, (3, 2.5)), (0.14, 1, 0.0, (4, 2.5)),
                                 (0.12, 0, 4.0, (3, 2.5))):
        m = int(n * share)
        uv = rng.random((m, 2)) * ext
        p = np.insert(uv, axis, at + rng.normal(0, noise, m), axis=1)
        parts.append(p)
    m = n - sum(len(p) for p in parts)
    parts.append(rng.random((m, 3)) * (3.6, 2.6, 2.1) + 0.2)
    pts = np.concatenate(parts).astype(np.float32)
    return np.ascontiguousarray(pts[rng.permutation(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/plane_removal_exp.txt")
    ap.add_argument("--only", default="", help="a scene name and a form, e.g. room_1000000:b -- that form alone (for a kernel trace)")
    args = ap.parse_args()
    import torch
    from plane_removal_util import two_plane_room
    from pointcloudcomparator_amd import capi
    assert capi.device_count() > 0, "no HIP device: nothing is measured without one"

    scenes = [("two_planes_33000", two_plane_room()), ("room_100000", room(100000)), ("room_1000000", room(1000000))]
    ix = capi.Index(np.zeros((1, 3), np.float32), auto_sync=False)
    lines = ["plane-removal loop, ms per cloud: median [min max] of %d runs, (a) (b) (c) interleaved, %d warm-up runs each" % (args.runs, args.warmup),
             "(a) pcc_sac_plane per turn on a host array + np.delete   (b) pcc_plane_removal, host memory   (c) pcc_plane_removal, device memory",
             "%-18s %7s %9s  %-26s %-26s %-26s %7s %7s" % ("scene", "planes", "remain", "(a) ms", "(b) ms", "(c) ms", "a / b", "a / c")]

    for name, pts in scenes:
        dev = torch.from_numpy(pts).cuda()
        torch.cuda.synchronize()
        n0 = len(pts)

        def form_a():
            cur, sizes, coeffs = pts, [], []
            while len(cur) > 0.3 * n0:
                inl, coeff, _ = ix.sac_plane(cur)
                if len(inl) == 0:
                    break
                sizes.append(len(inl)); coeffs.append(coeff)
                cur = np.ascontiguousarray(np.delete(cur, inl, 0))
            return cur, np.array(sizes), np.array(coeffs)

        def form_b():
            r = ix.plane_removal(pts, with_points=True)
            return r[6], r[3], r[2]

        def form_c():
            r = ix.plane_removal(dev, with_points=True)
            ix.sync()
            return r[6], r[3], r[2]

        forms = dict(a=form_a, b=form_b, c=form_c)
        if args.only:
            scene, form = args.only.split(":")
            if scene != name:
                continue
            for _ in range(args.warmup + 5):
                forms[form]()
            ix.sync()
            print("ran", args.only)
            continue
        results = {k: f() for k, f in forms.items()}
        rest_c = results["c"][0].cpu().numpy()
        for k, rest in (("b", results["b"][0]), ("c", rest_c)):
            assert (rest.view(np.uint32) == results["a"][0].view(np.uint32)).all() and rest.shape == results["a"][0].shape, (name, k)
            assert (results[k][1] == results["a"][1]).all(), (name, k)
            assert (results[k][2].view(np.uint32) == results["a"][2].view(np.uint32)).all(), (name, k)
        times = {k: [] for k in forms}
        for run in range(args.warmup + args.runs):
            for k, f in forms.items():
                ix.sync()
                t0 = time.perf_counter()
                f()
                ix.sync()
                if run >= args.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        cell = lambda v: "%7.3f [%7.3f %7.3f]" % (np.median(v), min(v), max(v))
        lines.append("%-18s %7d %9d  %-26s %-26s %-26s %7.2f %7.2f" % (
            name, len(results["a"][1]), len(results["a"][0]), cell(times["a"]), cell(times["b"]), cell(times["c"]),
            np.median(times["a"]) / np.median(times["b"]), np.median(times["a"]) / np.median(times["c"])))
        copies = []
        for f in (form_b, form_c):
            f()
            copies.append(ix.stats()[1])
        lines.append("%-18s host copies taken by (b) / (c): %d / %d" % ("", *copies))
    if args.only:
        return
    text = "\n".join(lines) + "\n"
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)


if __name__ == "__main__":
    main()
