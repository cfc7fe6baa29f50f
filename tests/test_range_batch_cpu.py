"""The scaffold the batch calls over ranges of ONE array share (pcc_fpfh_descriptors_batch, pcc_vfh_descriptors_batch:
csrc/range_batch_plan.hpp, csrc/entry.hpp, csrc/range_batch.hip), without a GPU: the plain-C++ header's own test binary;
the pieces that used to be copied exist once; the two calls keep none of them."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "pointcloudcomparator_amd" / "csrc"


def test_range_batch_header_on_the_cpu():
    """tests/cpp/test_range_batch_plan.cpp compiles csrc/range_batch_plan.hpp alone: the routes and both uploads against values
    recorded before the header existed, the host pack and its refusal, the offsets of one and two scenes"""
    subprocess.check_call(["make", "build/test_range_batch_plan"], cwd=ROOT)
    r = subprocess.run([str(ROOT / "build" / "test_range_batch_plan")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "range batch plan ok: 13 plans, 2 upload layouts" in r.stdout
    header = (CSRC / "range_batch_plan.hpp").read_text()
    assert "#include <hip" not in header and "hip_runtime" not in header and "pcc_internal.hpp" not in header and "__global__" not in header
    mk = (ROOT / "Makefile").read_text()
    assert "range_batch.hip" in re.search(r"^HIP_SRCS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert re.search(r"^hosttest:.*build/test_range_batch_plan", mk, flags=re.M)
    assert re.search(r"^asan:.*build/asan/test_range_batch_plan", mk, flags=re.M)
    assert "ASAN_OPTIONS=detect_leaks=1 build/asan/test_range_batch_plan" in mk
    assert "build/asan/test_range_batch_plan: " in mk and "$(SANFLAGS)" in mk.split("build/asan/test_range_batch_plan: ", 1)[1].split("\n\n", 1)[0]


def test_the_copied_pieces_exist_once():
    sources = {p.name: p.read_text() for p in sorted(CSRC.iterdir()) if p.suffix in (".hip", ".hpp")}

    def defined(pattern):
        return [name for name, text in sources.items() for _ in re.finditer(pattern, text, flags=re.M)]

    # the pack kernel, the finish kernel, the grid size of a grid-stride launch (ground.hip's helper computes something else and
    # has a name of its own), the arithmetic of "offsets must not decrease" and "2^31"
    assert defined(r"^k_\w*pack\s*\(const unsigned char\* __restrict__ pts, size_t stride, const unsigned int\* __restrict__ src") == ["range_batch.hip"]
    assert defined(r"^k_\w*batch_finish\s*\(const unsigned int\* __restrict__ pos") == ["rift_batch.hip"]
    assert defined(r"^\s*(?:static\s+|inline\s+)*(?:unsigned )?int\s+blocks_for\s*\(") == ["pcc_internal.hpp"]
    assert defined(r"\(n \+ 255\) / 256, 2048\)") == []
    assert defined(r"offsets\[\w+ \+ 1\] < \w*\.?offsets\[\w+\]|offsets\[\w+ \+ 1\] >= \w*\.?offsets\[\w+\]") == ["range_batch_plan.hpp"]
    assert defined(r"offsets\[(?:\w+\.)?n_clusters\] - (?:\w+\.)?offsets\[0\] >= \(1ull << 31\)") == ["range_batch_plan.hpp"]
    # the two calls are their stage kernels, their parameter check and their plan extras
    for name in ("fpfh_batch.hip", "vfh_batch.hip"):
        text = sources[name]
        for used in ('#include "entry.hpp"', "check_range_batch(", "stage_ranges(", "for_each_on_work_handle(", ": RangeStaging", "ClusterRanges"):
            assert used in text, (name, used)
        for gone in ("reinterpret_cast", "ConcatLayout", "WorkLease", "check_points(", "check_mem(", "pcc_index_set_input(", "finite3(", "blocks_for(size_t"):
            assert gone not in text, (name, gone)
        assert not re.search(r"k_\w*pack", text), name
    for name in ("cluster_desc.hip", "cluster_match.hip", "match_colour.hip", "range_batch.hip"):
        assert "check_cluster_offsets(" in sources[name], name
