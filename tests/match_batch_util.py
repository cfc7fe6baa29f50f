"""Shared by the pcc_match_knn_batch tests: the replayed workloads (tests/golden/match_workloads.json) as descriptor pairs."""
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "match_workloads.json"


def workloads():
    return json.loads(GOLDEN.read_text())["workloads"]


def drawn_sizes(n_pairs=300, seed=20250117):
    """(cluster1, cluster2, n1, n2) for a synthetic batch: sizes drawn from the descriptor counts above 3 that the recorded
    runs list; every pair its own cluster1 except each tenth, which shares the previous pair's"""
    counts = sorted({n for w in workloads().values() for n in w["descriptor_counts"]})
    rng = np.random.default_rng(seed)
    sizes = []
    for p in range(n_pairs):
        n1, n2 = (int(counts[k]) for k in rng.integers(0, len(counts), 2))
        if p % 10 == 9:
            sizes.append((sizes[-1][0], p, sizes[-1][2], n2))
        else:
            sizes.append((p, p, n1, n2))
    return sizes
