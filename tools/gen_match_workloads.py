"""Replays the cluster-matching loop of two recorded runs into tests/golden/match_workloads.json.

The reference ships two result files of its own runs.  Each lists, per cluster of both clouds, the number of points, the
number of RIFT descriptors and the centroid.  From those numbers alone this tool replays what the cluster-matching loop
(reference src/comparator.cpp:1296-1365; here host/report.hpp, clusterSections) does before it calls matchRIFTFeaturesKnn:
per cluster of cloud 1 the three nearest free centroids of cloud 2, then the two gates (more than 3 descriptors on both
sides; integer quotient of the point counts equal to 1).  What passes is one (cluster1, cluster2, n1, n2) per call.

usage: gen_match_workloads.py REFERENCE_DIR [--out FILE] [--check]
  --check  compare with the committed file instead of writing (exit status 1 on a difference)"""
import argparse
import json
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
FILES = {"results": "build/results.txt", "cuarto2": "build/cuarto2MLSSmoothing.txt~"}
NOTE = ("Recorded numbers only: per gated pair the cluster of cloud 1, the cluster of cloud 2 and their descriptor counts "
        "(n1 is indexed, n2 asks).  The result files print centroids to six significant digits, so the choice of the three "
        "nearest clusters is a replay of the PRINTED values, not of the original floats; descriptor contents are not "
        "recorded and are synthesised by the tests.")


def parse(text):
    """{1: [(points, descriptors, (x, y, z)), ...], 2: [...]} in cluster order"""
    pat = re.compile(r"PCL ?([12]) cluster (\d+):\s*\n\s*Number of points: (\d+)\s*\n\s*Number of descriptors: (\d+)\s*\n"
                     r"\s*Coordinates of centroid: \[([^,\]]+),([^,\]]+),([^,\]]+)\]")
    clusters = {1: [], 2: []}
    for m in pat.finditer(text):
        which, j = int(m.group(1)), int(m.group(2))
        assert j == len(clusters[which]), "clusters are listed in order"
        clusters[which].append((int(m.group(3)), int(m.group(4)), tuple(float(m.group(k)) for k in (5, 6, 7))))
    return clusters


def nearest_free(c, others, taken):
    """nearestFreeCentroid of host/report.hpp: float differences, squares and sum in double, float square root, strict <"""
    arg, best = -1, np.float32(1000000000000.0)
    for j, o in enumerate(others):
        if j in taken:
            continue
        d2 = np.float32(sum(float(np.float32(c[a]) - np.float32(o[a])) ** 2 for a in range(3)))
        d = np.sqrt(d2, dtype=np.float32)
        if d < best:
            best, arg = d, j
    return arg


def replay(clusters):
    cents2 = [c[2] for c in clusters[2]]
    pairs = []
    for i, (p1, n1, c1) in enumerate(clusters[1]):
        taken, cand = set(), []
        for k in range(3):
            cand.append(nearest_free(c1, cents2, taken))
            if k < 2:
                taken.add(cand[k])
        for j in cand:
            if j == -1:
                continue
            p2, n2, _ = clusters[2][j]
            if n1 <= 3 or n2 <= 3:
                continue
            if p2 // p1 != 1:
                continue
            pairs.append([i, j, n1, n2])
    return pairs


def generate(reference_dir):
    doc = {"note": NOTE, "workloads": {}}
    for name, rel in FILES.items():
        clusters = parse((Path(reference_dir) / rel).read_text(errors="replace"))
        pairs = replay(clusters)
        doc["workloads"][name] = {
            "file": rel, "clusters1": len(clusters[1]), "clusters2": len(clusters[2]),
            "descriptor_counts": sorted({n for which in (1, 2) for _, n, _ in clusters[which] if n > 3}),
            "pairs": pairs,
        }
    return doc


def dumps(doc):
    # (one pair per line: the file stays readable and diffs stay small)
    head = {k: v for k, v in doc.items() if k != "workloads"}
    lines = ["{", f' "note": {json.dumps(head["note"])},', ' "workloads": {']
    names = list(doc["workloads"])
    for name in names:
        w = doc["workloads"][name]
        lines.append(f'  {json.dumps(name)}: {{')
        for k in ("file", "clusters1", "clusters2", "descriptor_counts"):
            lines.append(f'   {json.dumps(k)}: {json.dumps(w[k])},')
        lines.append('   "pairs": [')
        lines += [f'    {json.dumps(p)}{"," if n + 1 < len(w["pairs"]) else ""}' for n, p in enumerate(w["pairs"])]
        lines.append("   ]")
        lines.append("  }" + ("," if name != names[-1] else ""))
    lines += [" }", "}"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("reference_dir")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "match_workloads.json"))
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    text = dumps(generate(a.reference_dir))
    if a.check:
        sys.exit(0 if Path(a.out).read_text() == text else 1)
    Path(a.out).write_text(text)
    for name, w in json.loads(text)["workloads"].items():
        p = w["pairs"]
        print(f"{name}: clusters {w['clusters1']} / {w['clusters2']}, {len(p)} gated pairs, sum n1 {sum(x[2] for x in p)}, "
              f"sum n2 {sum(x[3] for x in p)}, distance pairs {sum(x[2] * x[3] for x in p):.3g}, "
              f"distinct reference clouds {len({x[0] for x in p})}")
