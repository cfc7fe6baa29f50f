"""The shared __host__ __device__ arithmetic (csrc/libm_f32.hpp, plane_fit.hpp, rift_math.hpp, sift_math.hpp, rigid_solve.hpp)
as gfx950 evaluates it against the host compile of the same text, function by function (tests/cpp/test_device_math.hip):
the same case buffers through a kernel and through the host pass, outputs compared word for word.  The host pass itself is
pinned to the host's libm by tests/test_device_math_cpu.py."""
import re
import subprocess
from pathlib import Path

import pytest

from device_math_util import FUNCTIONS

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_device_returns_the_host_compiles_bits(gpu):
    exe = ROOT / "build" / "test_device_math"
    if not exe.exists():
        subprocess.check_call(["make", "build/test_device_math"], cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert r.stdout.rstrip().endswith("device math: 0 mismatches"), r.stdout[-2000:]
    for fn in FUNCTIONS:
        m = re.search(rf"^{fn}: (\d+) cases, 0 mismatches$", r.stdout, re.M)
        assert m and int(m.group(1)) > 0, fn
