"""dev helper (no GPU): how far the float32 run of the NumPy restatement of the RIFT pipeline (tests/rift_ref.py) is from its
float64 run on every small test scene, and how far the host mirror (build/rift_host) is from the float64 run -- the figures
behind F32_VS_F64 / GIVEN_NORMALS in tests/test_rift_cpu.py and the table in EXPERIMENTS.md ("RIFT descriptors").
'own normals': every stage in the run's dtype; 'given normals': both runs take oracle.normals_radius' float32 normals."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oracle
import rift_ref
import rift_util

subprocess.check_call(["make", "build/rift_host"], cwd=ROOT, stdout=subprocess.DEVNULL)
print(f"{'scene':11s} {'points':>6s} {'row 3cm':>7s} {'kept':>5s} {'cond A':>8s} | own normals: {'f32-f64':>9s} {'host-f64':>9s} {'ratio':>6s} | "
      f"given normals: {'f32-f64':>9s} {'host-f64':>9s} {'ratio':>6s}")
for name in rift_util.SMALL:
    p, rgb = rift_util.scene(name)
    h64, i64, info = rift_ref.rift_pipeline(p, rgb, np.float64)
    h32, i32, _ = rift_ref.rift_pipeline(p, rgb, np.float32)
    nr = oracle.normals_radius(np.ascontiguousarray(p), 0.03)[:, :3]
    g64, j64, _ = rift_ref.rift_pipeline(p, rgb, np.float64, normals=nr)
    g32, j32, _ = rift_ref.rift_pipeline(p, rgb, np.float32, normals=nr)
    hh, ih, _ = rift_util.run_tool(rift_util.HOST, p, rgb, tempfile.mkdtemp())
    assert np.array_equal(i64, i32) and np.array_equal(j64, j32) and np.array_equal(ih, i64) and np.array_equal(ih, j64)
    a, b = np.abs(h32 - h64).max(), np.abs(hh - h64).max()
    c, d = np.abs(g32 - g64).max(), np.abs(hh - g64).max()
    print(f"{name:11s} {len(p):6d} {np.median(info['rows_normal']):7.0f} {len(i64):5d} {info['cond'].max():8.1e} | "
          f"             {a:9.3g} {b:9.3g} {b / a:6.2f} |                {c:9.3g} {d:9.3g} {d / c:6.2f}")
