"""What tests/test_vfh_batch_gpu.py and tools/exp_vfh_batch.py share: the clusters of a batch -- all in the same corner of space,
so that a neighbour, a centroid term or a vote from another cluster changes bits --, the expected descriptors (build/vfh_host
on each cluster ALONE, computed once per tag and left unchanged; for hundreds of tiny clusters the existing single call
pcc_vfh_descriptor on each cluster), bit comparisons and the files of build/vfh_batch_driver."""
import subprocess
from pathlib import Path

import numpy as np

import vfh_util
from pointcloudcomparator_amd import capi, synth

ROOT = Path(__file__).resolve().parent.parent
BATCH_DRIVER = ROOT / "build" / "vfh_batch_driver"
BINS = vfh_util.BINS
EMPTY = np.zeros((0, 3), np.float32)
NO_ROW = np.zeros((0, BINS), np.float32)
CENT_TILE = 512    # points of a parked tile of the centroid chains (csrc/vfh_device.hpp: 64 x VFH_CENT_ROWS)
VOTE_POINTS = 1024  # points of a vote item at most (csrc/vfh_batch_plan.hpp: VFH_BATCH_VOTE_POINTS)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def host(x):
    return x.cpu().numpy() if capi._is_torch(x) else np.asarray(x)


def cloud(n, seed=None):
    """the generator of the single call's scenes at their density (600 points per 0.12 m cube), in the same corner of space
    whatever n: clusters of one batch overlap"""
    if n == 0:
        return EMPTY
    return synth.rift_cloud(n, 100 + n if seed is None else seed, extent=0.12 * (max(n, 8) / 600) ** (1 / 3))[0]


def expected_rows(n):
    return 1 if n >= 2 else 0


def assert_same(got, want, what=""):
    """one cluster's result against its expected (m, 308) array, m = 0 or 1"""
    got = host(got)
    if len(want) == 0:
        assert got.shape == (0, BINS), f"{what}: a cluster without a descriptor returned {got.shape}"
        return
    assert got.shape == (BINS,) and got.dtype == np.float32, f"{what}: {got.shape} {got.dtype}"
    differ = bits(got) != bits(want[0])
    assert not differ.any(), (f"{what}: {int(differ.sum())} of 308 bins differ in their bits, first {int(np.argmax(differ))}: "
                              f"{got[differ][:4]} vs {want[0][differ][:4]}")


def assert_distinct(wants, what=""):
    """the expected descriptors of distinct clusters differ from one another: a kernel that writes one cluster's descriptor
    everywhere cannot pass"""
    rows = [bits(w[0]).tobytes() for w in wants if len(w)]
    assert len(rows) >= 2 and len(set(rows)) == len(rows), f"{what}: {len(rows)} expected descriptors, {len(set(rows))} distinct"


class Mirror:
    """tag, points[, radius] -> (m, 308) of build/vfh_host on that cluster alone (m = 0 below 2 points: the tool is not asked)"""

    def __init__(self, tmp):
        self.tmp, self.cache = Path(tmp), {}

    def __call__(self, tag, points, radius=None):
        key = (tag, radius)
        if key not in self.cache:
            if len(points) < 2:
                got = NO_ROW
            else:
                got = vfh_util.run_host(np.ascontiguousarray(points[:, :3]), self.tmp, tag=f"{tag.replace('-', '_')}_{len(self.cache)}", radius=radius)["hist"]
                assert got.shape == (1, BINS), tag
            got = np.array(got)
            got.setflags(write=False)
            self.cache[key] = got
        return self.cache[key]


def single_call(ix, points, radius=0.03):
    """the existing single call on a handle of the test's: (m, 308)"""
    if len(points) == 0:
        return NO_ROW
    ix.set_input(points)
    got = np.array(host(ix.vfh_descriptor(radius))).reshape(-1, BINS)
    got.setflags(write=False)
    return got


def run_batch_driver(clouds, split, tmp, timeout=120):
    """build/vfh_batch_driver: ([(m, 308) per cloud], (n1, n2) float64 distances, stdout)"""
    tmp = Path(tmp)
    files = []
    for k, p in enumerate(clouds):
        files.append(tmp / f"bd{k}.in")
        vfh_util.write_cloud(files[-1], p)
    r = subprocess.run([str(BATCH_DRIVER), str(tmp / "bd_out"), str(split)] + [str(f) for f in files], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    des = [vfh_util.read_result(tmp / f"bd_out.{k}") for k in range(len(clouds))]
    raw = (tmp / "bd_out.match").read_bytes()
    n1, n2 = (int(v) for v in np.frombuffer(raw[:8], np.int32))
    dist = np.frombuffer(raw[8:], np.float64).reshape(n1, n2)
    return des, dist, r.stdout
