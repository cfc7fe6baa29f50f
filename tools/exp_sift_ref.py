"""dev helper (no GPU): how far the float32 run of the NumPy restatement of the SIFT keypoint detector (tests/sift_ref.py) is
from its float64 run on every small test scene, and how far the host mirror (build/sift_host) is from the float64 run -- the
figures behind F32_VS_F64 in tests/test_sift_cpu.py and the table in EXPERIMENTS.md ("SIFT keypoints").  Largest deviation of
a DoG column over all octaves (mean intensities on the scale 0 .. 255); keypoints as (octave, point, column)."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import sift_ref
import sift_util

subprocess.check_call(["make", "build/sift_host"], cwd=ROOT, stdout=subprocess.DEVNULL)
print(f"{'scene':9s} {'octave sizes':>24s} {'stop':>5s} {'keypoints':>9s} {'mean row':>20s} | {'f32-f64':>9s} {'host-f64':>9s} {'ratio':>6s} | "
      f"{'same keypoints f32 / host':>25s} {'min margin':>10s}")
for name in sift_util.SMALL:
    p, rgb = sift_util.scene(name)
    r64 = sift_ref.sift_pipeline(p, rgb, np.float64)
    r32 = sift_ref.sift_pipeline(p, rgb, np.float32)
    h = sift_util.run_host(p, rgb, tempfile.mkdtemp(), dump=True)
    a = max(float(np.abs(x["dog"].astype(np.float64) - y["dog"]).max()) for x, y in zip(r32["octaves"], r64["octaves"]))
    b = max(float(np.abs(x["dog"].astype(np.float64) - y["dog"]).max()) for x, y in zip(h["octaves"], r64["octaves"]))
    same32 = r32["keypoints"] == r64["keypoints"]
    same_h = [tuple(int(v) for v in k) for k in h["ids"]] == r64["keypoints"]
    rows = " ".join(f"{o['rows'].mean():.0f}" for o in r64["octaves"])
    print(f"{name:9s} {'/'.join(str(s) for s in r64['sizes']):>24s} {r64['stop']:>5s} {len(r64['keypoints']):9d} {rows:>20s} | "
          f"{a:9.3g} {b:9.3g} {b / a:6.2f} | {str(same32):>12s} / {str(same_h):<10s} {r64['margins'].min():10.3g}")
