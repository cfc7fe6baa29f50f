"""The pruned k = 1 kernel has two forms (PCC_OPT_NN1_KERNEL): 0 = one lane per query (k_grid_nn1), 1 = rows drained
flat with lanes over candidates (k_grid_nn1_flat2); 2 and 3 force how the flat form finishes the lanes its cube leaves
open (a second kernel over a compacted list / in place), which 1 chooses by the number of queries.  All of them are
exact: indices and d2 bits must equal the oracle's exhaustive scan -- reference src/comparator.cpp:571-577."""
import numpy as np
import pytest

import oracle
from pointcloudcomparator_amd import capi, synth

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _scenes():
    rng = np.random.default_rng(11)
    out = []
    a = synth.corridor_cloud(60000, synth.SEED_A)
    b = synth.corridor_cloud(20000, synth.SEED_B)
    out.append(("corridor", a, b))
    out.append(("objects", synth.corridor_cloud(60000, synth.SEED_A, layer="objects"),
                synth.corridor_cloud(20000, synth.SEED_B, layer="objects")))
    base = rng.random((3000, 3), dtype=np.float32)
    out.append(("duplicates", np.concatenate([base, base[::-1], base[:700]]),
                np.concatenate([base[rng.integers(0, 3000, 2000)], rng.random((1000, 3), dtype=np.float32)])))
    plane = rng.random((20000, 3), dtype=np.float32)
    plane[:, 2] = 0.25
    out.append(("plane", plane, rng.random((5000, 3), dtype=np.float32)))
    same = np.full((9000, 3), 0.5, np.float32)          # one cell holds everything: spans past the flat pass's capacity
    same[:100] = rng.random((100, 3), dtype=np.float32)
    out.append(("pile", same, rng.random((3000, 3), dtype=np.float32)))
    clumps = (rng.integers(0, 6, (30000, 3)) * np.float32(0.2) + rng.normal(0, 0.004, (30000, 3))).astype(np.float32)
    out.append(("clumps", clumps, (rng.random((8000, 3)) * 1.2 - 0.1).astype(np.float32)))
    far = synth.corridor_cloud(8000, synth.SEED_B)
    far[:3000] += np.float32([1.5, -2.0, 0.7])
    far[3000:4000] += np.float32(30.0)
    out.append(("far", a, far))
    nf = synth.corridor_cloud(30000, synth.SEED_A)
    nf[::97, 1] = np.nan
    qn = synth.corridor_cloud(9000, synth.SEED_B)
    qn[::53, 0] = np.inf
    out.append(("nonfinite", nf, qn))
    return out


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 12])
def test_nn1_kernel_forms_match_the_oracle(gpu, mode):
    """(12: form 2 with the listed open lanes finished one lane per query -- PCC_OPT_NN1_OPEN_FLAT = 0, round 3's kernel)"""
    open_flat, mode = (0, 2) if mode == 12 else (1, mode)
    for name, ref, qry in _scenes():
        oi, od = oracle.nn1_exhaustive(ref, qry)
        with capi.Index(ref, engine=capi.ENGINE_GRID) as ix:
            ix.set_option(capi.OPT_NN1_KERNEL, mode)
            ix.set_option(capi.OPT_NN1_OPEN_FLAT, open_flat)
            assert ix.get_option(capi.OPT_NN1_KERNEL) == mode and ix.get_option(capi.OPT_NN1_OPEN_FLAT) == open_flat
            for _ in range(2):  # (the second call takes the far route where the first had fallbacks)
                idx, d2 = ix.nn1(qry)
                assert (_bits(d2) == _bits(od)).all(), (name, mode, np.nonzero(_bits(d2) != _bits(od))[0][:5])
                assert (idx == oi).all(), (name, mode, np.nonzero(idx != oi)[0][:5])


def test_nn1_kernel_forms_agree_at_a_million(gpu):
    torch = pytest.importorskip("torch")
    n = 1_000_000
    a = torch.from_numpy(synth.corridor_cloud(n, synth.SEED_A)).cuda()
    b = torch.from_numpy(synth.corridor_cloud(n, synth.SEED_B)).cuda()
    res = []
    with capi.Index(a, engine=capi.ENGINE_GRID) as ix:
        for mode in (0, 1, 2, 3):
            ix.set_option(capi.OPT_NN1_KERNEL, mode)
            idx, d2 = ix.nn1(b)
            res.append((idx.cpu().numpy(), d2.cpu().numpy()))
    with capi.Index(a, engine=capi.ENGINE_BRUTE) as ix:  # the exhaustive kernel on a sample
        bi, bd = ix.nn1(b[:20000])
        bi, bd = bi.cpu().numpy(), bd.cpu().numpy()
    for idx, d2 in res:
        assert (idx == res[0][0]).all() and (_bits(d2) == _bits(res[0][1])).all()
        assert (idx[:20000] == bi).all() and (_bits(d2[:20000]) == _bits(bd)).all()


@pytest.mark.parametrize("stage", [0, 1, 2])
def test_three_level_sort_forms_build_the_same_index(gpu, stage):
    """PCC_OPT_SORT_STAGE1: level 1 of the sort for clouds beyond the L2s with and without bucket-sorted LDS tiles (references /
    queries): 2M x 2M through the three-level sort on both sides (thresholds lowered), results = the default's, bit for bit"""
    torch = pytest.importorskip("torch")
    n = 2_000_000
    a = torch.from_numpy(synth.corridor_cloud(n, synth.SEED_A)).cuda()
    b = torch.from_numpy(synth.corridor_cloud(n, synth.SEED_B)).cuda()
    with capi.Index(a, engine=capi.ENGINE_GRID) as ix:
        i0, d0 = ix.nn1(b)
        ix.set_option(capi.OPT_SORT_STAGE1, stage)
        ix.set_option(capi.OPT_SORT_MP_MIN, 1000)       # the three-level sort for both clouds
        ix.set_option(capi.OPT_SORT_MP_MIN_Q, 1000)
        ix.set_input(a)
        i1, d1 = ix.nn1(b)
        assert (i0 == i1).all().item() and (d0.view(torch.int32) == d1.view(torch.int32)).all().item()
        assert ix.stats()[1] == 0
    with capi.Index(a[:50000], engine=capi.ENGINE_BRUTE) as bx:      # and against the exhaustive kernel on a slice
        bi, bd = bx.nn1(b[:3000])
    with capi.Index(a[:50000], engine=capi.ENGINE_GRID) as gx:
        gx.set_option(capi.OPT_SORT_STAGE1, stage)
        gx.set_option(capi.OPT_SORT_MP_MIN, 1000)
        gx.set_option(capi.OPT_SORT_MP_MIN_Q, 1000)
        gx.set_input(a[:50000])
        gi, gdd = gx.nn1(b[:3000])
    assert (bi == gi).all().item() and (bd.view(torch.int32) == gdd.view(torch.int32)).all().item()


def test_options_are_per_handle_and_validated(gpu):
    a = synth.corridor_cloud(5000, synth.SEED_A)
    with capi.Index(a) as ix, capi.Index(a) as iy:
        ix.set_option(capi.OPT_FAR_MODE, 1)
        assert ix.get_option(capi.OPT_FAR_MODE) == 1 and iy.get_option(capi.OPT_FAR_MODE) == -1
        for opt, bad in ((capi.OPT_GRID_PPC, 0.0), (capi.OPT_FAR_MODE, 2), (capi.OPT_NN1_KERNEL, 4), (99, 1), (capi.OPT_ICP_WARM, 0.5)):
            with pytest.raises(capi.PccError):
                ix.set_option(opt, bad)


_FLAG = "flag"  # exactly 0 or 1
_INF = float("inf")
# option, built-in default, lowest and highest accepted value, values just outside either end, (fractional value, what is stored) for
# int options.  Read off the range switch and struct Options as they stood before the options became one table.
_OPTION_RANGES = [
    (capi.OPT_GRID_PPC, 0.75, 5e-324, 1024.0, [0.0, -5e-324, np.nextafter(1024.0, _INF)], None),
    (capi.OPT_GRID_TRIM, 3, 0, 8, [-0.5, 8.5], (2.5, 2)),
    (capi.OPT_FAR_MODE, -1, -1, 1, [-1.5, 1.5], (0.5, 0)),
    (capi.OPT_ICP_WARM, 1, 0, 1, _FLAG, None),
    (capi.OPT_ICP_DEVICE_LOOP, 1, 0, 1, _FLAG, None),
    (capi.OPT_EC_CELLS, 3, 0, 4, [-0.5, 4.5], (1.5, 1)),
    (capi.OPT_SORT_MP_MIN, 1.8e6, 0.0, 1.7e308, [-5e-324, -1.0], None),
    (capi.OPT_SORT_MP_MIN_Q, 2.5e6, 0.0, 1.7e308, [-5e-324, -1.0], None),
    (capi.OPT_NN1_KERNEL, 1, 0, 3, [-0.5, 3.5], (2.7, 2)),
    (capi.OPT_FLANN_SPLIT, 0, 0, 2, [-0.5, 2.5], (1.5, 1)),
    (capi.OPT_NN1_DENSE_MIN, 4, 1, 1000000, [0, 0.5, 1000000.5], (7.9, 7)),
    (capi.OPT_KNN_KERNEL, 1, 0, 1, _FLAG, None),
    (capi.OPT_KNN_CACHE_K, 0, 0, 512, [-0.5, 512.5], (50.5, 50)),
    (capi.OPT_NN1_OPEN_FLAT, 1, 0, 1, _FLAG, None),
    (capi.OPT_SORT_STAGE1, 1, 0, 2, [-0.5, 2.5], (1.5, 1)),
    (capi.OPT_ICP_SORTED, 1, 0, 1, _FLAG, None),
    (capi.OPT_OVERLAP_PREP, 1, 0, 2, [-0.5, 2.5], (1.9, 1)),
    (capi.OPT_GRID_AXES, -1, -2, 5, [-2.5, 5.5], (3.5, 3)),
    (capi.OPT_XCD_RUN, 256, 1, 4096, [0, 0.5, 4096.5], (32.5, 32)),
    (capi.OPT_FUSE_PARAMS, 0, 0, 3, [-0.5, 3.5], (2.5, 2)),
    (capi.OPT_HOST_PIPE, 1, 0, 1, _FLAG, None),
    (capi.OPT_SCAN_CHAINED, 1, 0, 1, _FLAG, None),
    (capi.OPT_KNN_RUN, 16, 1, 64, [0, 0.5, 64.5], (8.5, 8)),
    (capi.OPT_RIFT_LAYOUT, 1, 0, 1, _FLAG, None),
    (capi.OPT_SIFT_LAYOUT, 1, 0, 1, _FLAG, None),
    (capi.OPT_RIFT_BATCH_BRUTE_MAX, 8192, 0, 1073741824, [-0.5, 1073741824.5], (4500.5, 4500)),
]


def test_every_option_keeps_its_range_and_default(gpu):
    """all 26 options of pcc_index_set_option: the default a handle starts with, both ends of the accepted range (they
    round-trip), a fractional value inside an int option's range (its truncation is stored), and what is refused -- values just
    outside either end, anything but 0 and 1 for a flag, NaN, the infinities, an unknown option -- leaving the stored value alone"""
    assert [row[0] for row in _OPTION_RANGES] == list(range(1, 27))
    cloud = np.random.default_rng(3).random((100, 3), dtype=np.float32)
    with capi.Index(cloud) as ix:
        for opt, default, lo, hi, outside, frac in _OPTION_RANGES:
            assert ix.get_option(opt) == default, opt
            for v in (lo, hi):
                ix.set_option(opt, v)
                assert ix.get_option(opt) == v, (opt, v)
            if frac is not None:
                ix.set_option(opt, frac[0])
                assert ix.get_option(opt) == frac[1], (opt, frac)
            if outside is _FLAG:
                outside = [-1, -0.5, 0.5, 1.5, 2]
            before = ix.get_option(opt)
            for bad in list(outside) + [float("nan"), _INF, -_INF]:
                with pytest.raises(capi.PccError):
                    ix.set_option(opt, bad)
                assert ix.get_option(opt) == before, (opt, bad)
        with pytest.raises(capi.PccError):
            ix.set_option(99, 1)
        with pytest.raises(capi.PccError):
            ix.get_option(99)


def test_environment_variables_give_a_new_handle_its_defaults(gpu):
    """PCC_* variables in a fresh process: an int option keeps the truncation of a fractional value inside its range (2.7 -> 2),
    values pcc_index_set_option would refuse are ignored (a grid of 0 points per cell, a flag of 2), others are taken (8)"""
    import os
    import subprocess
    import sys
    from pathlib import Path
    child = ("import numpy as np\n"
             "from pointcloudcomparator_amd import capi\n"
             "with capi.Index(np.random.default_rng(3).random((100, 3), dtype=np.float32)) as ix:\n"
             "    print('options', *[ix.get_option(o) for o in (capi.OPT_NN1_KERNEL, capi.OPT_GRID_PPC, capi.OPT_HOST_PIPE, capi.OPT_KNN_RUN)])\n")
    env = dict(os.environ, PCC_NN1_KERNEL="2.7", PCC_GRID_PPC="0", PCC_HOST_PIPE="2", PCC_KNN_RUN="8")
    out = subprocess.run([sys.executable, "-c", child], cwd=Path(__file__).resolve().parents[1], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    assert [ln for ln in out.stdout.splitlines() if ln.startswith("options")] == ["options 2.0 0.75 1.0 8.0"]
