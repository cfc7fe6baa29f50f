"""Records the per-cluster tables of two recorded runs into tests/golden/cluster_tables.json.

The reference ships two result files of its own runs.  Each lists, per cluster of both clouds, the number of points, the number
of RIFT descriptors and the centroid, and -- where the run matched clusters -- one "Matched cluster i of PCL 1 with cluster j of
PCL 2" line per accepted match.  Those numbers are what pcc_cluster_matching takes beside the descriptors themselves (offsets
from the descriptor counts, centroids, point counts), so the tests replay the cluster-matching loop on them: candidates and gates
against tests/golden/match_workloads.json (tools/gen_match_workloads.py, whose parser this tool reuses), the recorded matches
against the candidates.

usage: gen_cluster_tables.py REFERENCE_DIR [--out FILE] [--check]
  --check  compare with the committed file instead of writing (exit status 1 on a difference)"""
import argparse
import json
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from gen_match_workloads import FILES, parse  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
NOTE = ("Recorded numbers only: per cluster [points, descriptors, [centroid as printed, six significant digits]], and the "
        "[cluster of PCL 1, cluster of PCL 2] of every 'Matched cluster' line.  Descriptor contents are not recorded and are "
        "synthesised by the tests.")
MATCHED = re.compile(r"Matched cluster (\d+) of PCL 1 with cluster (\d+) of PCL 2")


def generate(reference_dir):
    doc = {"note": NOTE, "runs": {}}
    for name, rel in FILES.items():
        text = (Path(reference_dir) / rel).read_text(errors="replace")
        clusters = parse(text)
        doc["runs"][name] = {
            "file": rel,
            "clusters1": [[p, n, list(c)] for p, n, c in clusters[1]],
            "clusters2": [[p, n, list(c)] for p, n, c in clusters[2]],
            "matched": [[int(m.group(1)), int(m.group(2))] for m in MATCHED.finditer(text)],
        }
    return doc


def dumps(doc):
    # (one cluster per line: the file stays readable and diffs stay small)
    lines = ["{", f' "note": {json.dumps(doc["note"])},', ' "runs": {']
    names = list(doc["runs"])
    for name in names:
        r = doc["runs"][name]
        lines.append(f'  {json.dumps(name)}: {{')
        lines.append(f'   "file": {json.dumps(r["file"])},')
        for key in ("clusters1", "clusters2", "matched"):
            lines.append(f'   {json.dumps(key)}: [')
            lines += [f'    {json.dumps(row)}{"," if n + 1 < len(r[key]) else ""}' for n, row in enumerate(r[key])]
            lines.append("   ]" + ("," if key != "matched" else ""))
        lines.append("  }" + ("," if name != names[-1] else ""))
    lines += [" }", "}"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("reference_dir")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "cluster_tables.json"))
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    text = dumps(generate(a.reference_dir))
    if a.check:
        sys.exit(0 if Path(a.out).read_text() == text else 1)
    Path(a.out).write_text(text)
    for name, r in json.loads(text)["runs"].items():
        print(f"{name}: clusters {len(r['clusters1'])} / {len(r['clusters2'])}, {len(r['matched'])} recorded matches")
