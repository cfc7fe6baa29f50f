"""pcc_match_knn_batch_dims without a GPU: the entry point is declared, exported and bound; it refuses bad arguments before it
looks at any device, in the documented order; the NumPy restatement the GPU tests compare with is sensitive to what it has to
pin (the order and the rounding of the sum, the bins beyond the third); zero padding leaves its bits alone; and the
plan/pack header passes its stand-alone program."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import match_batch_util as mbu  # noqa: E402
import match_dims_util as mdu  # noqa: E402


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_entry_point_is_declared_exported_and_bound():
    from pointcloudcomparator_amd import capi
    header = (ROOT / "include" / "pcc_nn.h").read_text()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+pcc_match_knn_batch_dims\s*\(", header, flags=re.S)
    assert m, "pcc_match_knn_batch_dims is not declared under a comment of its own"
    comment = m.group(1)
    assert "src/comparator.cpp:560-588" in comment and ":1296-1365" in comment   # the reference lines it stands for
    assert "LOWEST INDEX" in comment and "descriptor matching\n *   only" in comment.replace("\r", "")
    assert "pcc_match_knn_batch_dims" in capi.SYMBOLS
    fn = capi.LIB.pcc_match_knn_batch_dims
    assert fn.restype is C.c_int and len(fn.argtypes) == 13
    import inspect
    for f in (capi.match_knn_batch, capi.Index.match_knn_batch):
        p = inspect.signature(f).parameters
        assert p["dim"].default == 3 and p["return_d2"].default is False


def test_argument_validation_needs_no_gpu():
    from pointcloudcomparator_amd import capi
    L = capi.LIB
    a = np.zeros((4, 32), np.float32)
    ptrs, ns = (C.c_void_p * 1)(a.ctypes.data), (C.c_size_t * 1)(4)
    nulls = (C.c_void_p * 1)(None)
    out, d2, off = np.zeros(8, np.int32), np.full(8, 7, np.float32), np.full(2, 99, np.uintp)
    o, d, f = out.ctypes.data, d2.ctypes.data, off.ctypes.data
    thr = np.float32(0.05)

    def call(stride, dim, n_pairs=1, d1=ptrs, n1=ns, d2_=ptrs, n2=ns, mem=0, oo=o, dd=d, ff=f):
        return L.pcc_match_knn_batch_dims(None, n_pairs, d1, n1, d2_, n2, stride, dim, mem, thr, oo, dd, ff)

    def err():
        return L.pcc_last_error()

    # the dimension first: refused as unsupported whatever else is wrong, the message names the range
    for dim in (0, -1, 33):
        assert call(128, dim) == -5 and b"1 ... 32" in err()
        assert call(10, dim, mem=7, ff=None) == -5 and b"1 ... 32" in err()
    # then the stride: a multiple of 4 and >= 4 * dim (the >= 12 rule is dim 3's alone)
    for stride, dim in ((124, 32), (8, 3), (10, 2), (10, 1), (0, 1), (130, 32)):
        assert call(stride, dim) == -1 and b"stride" in err()
        assert call(stride, dim, mem=capi.MEM_DEVICE, ff=None) == -1 and b"stride" in err()
    # then everything pcc_match_knn_batch refuses, with its messages; a null handle with good arguments is the last refusal
    assert call(4, 1) == -1 and b"null index" in err()
    assert call(8, 2) == -1 and b"null index" in err()
    assert call(128, 32) == -1 and b"null index" in err()
    assert call(128, 32, dd=None) == -1 and b"null index" in err()              # out_d2 may be null
    assert call(128, 32, n_pairs=0, d1=None, n1=None, d2_=None, n2=None, oo=None, dd=None) == -1 and b"null index" in err()
    for kw in (dict(d1=None), dict(n1=None), dict(d2_=None), dict(n2=None), dict(oo=None), dict(ff=None)):
        assert call(128, 32, **kw) == -1
        assert b"null" in err() and b"null index" not in err()
    assert call(128, 32, d1=nulls) == -1 and b"null point pointer" in err()
    assert call(128, 32, d2_=nulls) == -1 and b"null point pointer" in err()
    assert call(128, 32, mem=capi.MEM_DEVICE) == -5 and b"PCC_MEM_HOST" in err()
    assert call(128, 32, mem=7) == -1 and b"mem space" in err()
    big = (C.c_size_t * 2)(2 ** 30, 2 ** 30)
    two = (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data + 128)
    small = (C.c_size_t * 2)(4, 3)
    assert call(128, 32, n_pairs=2, d1=two, n1=big, d2_=two, n2=small) == -5 and b"2^31" in err()
    assert call(128, 32, n_pairs=2, d1=two, n1=small, d2_=two, n2=big) == -5 and b"2^31" in err()
    assert call(128, 32, n1=(C.c_size_t * 1)(2 ** 31)) == -5
    # nothing was written by any refused call
    assert off.tolist() == [99, 99] and not out.any() and (d2 == 7).all()
    # pcc_index_create keeps refusing every dim != 3: N-dimensional search exists for descriptor matching only
    h = C.c_void_p()
    assert L.pcc_index_create(a.ctypes.data, 4, 128, 32, 0, 0, 0, C.byref(h)) == -5


def test_the_restatement_is_sensitive_to_what_it_pins():
    """on the 257 x 130 uniform pair of the GPU parity batch: a contracted multiply-add chain, another summation order, and
    a search on three bins each give visibly other answers -- a kernel that did any of these would fail the parity test"""
    pairs = mdu.parity_pairs()
    k = mdu.N1.index(257) * len(mdu.N2) + mdu.N2.index(130)
    assert mdu.family_of(mdu.N1.index(257), mdu.N2.index(130)) == "uniform"
    a, b = pairs[k]
    assert a.shape == (257, 32) and b.shape == (130, 32)
    arg3 = mdu.d2_chain(a, b, 3).argmin(1)
    for dim in (4, 8, 16, 32):
        chain = mdu.d2_chain(a, b, dim)
        fma = (bits(chain.min(1)) != bits(mdu.d2_fma(a, b, dim).min(1))).mean()
        assert fma > 0.10, (dim, fma)                                   # (24 - 35 % when this was written)
        if dim >= 8:
            pw = (bits(chain) != bits(mdu.d2_pairwise(a, b, dim))).mean()
            assert pw > 0.20, (dim, pw)                                 # (41 - 64 %)
    assert (mdu.d2_chain(a, b, 32).argmin(1) != arg3).mean() > 0.5      # (> 75 %)


def test_ties_at_32_dims_per_family():
    """the uniform family has no exact tie at dim 32; the quantised family as drawn has them in three bins and none in 32
    (no two records agree in 32 bins), so the GPU tie test uses quantised records with planted ties: assert they are there"""
    from pointcloudcomparator_amd import synth
    pairs = mdu.parity_pairs()
    tied = {"uniform": 0, "quantised": 0}
    tied3 = dict(tied)
    for k, (a, b) in enumerate(pairs):
        fam = mdu.family_of(k // len(mdu.N2), k % len(mdu.N2))
        tied[fam] += mdu.restate(a, b, 32, 0.05)[2]
        tied3[fam] += mdu.restate(a, b, 3, 0.05)[2]
    assert tied == {"uniform": 0, "quantised": 0} and tied3["uniform"] == 0 and tied3["quantised"] > 0
    for a, b in synth.descriptor_pairs(mbu.workloads()["results"]["pairs"], "uniform", seed=7):
        assert mdu.restate(a, b, 32, 0.05)[2] == 0
    a, b = mdu.tie_pair()
    row, d2, n_tied = mdu.restate(a, b, 32, 0.05)
    assert n_tied == 80 and len(row) == 101
    assert row[1:].tolist() == list(range(100))                          # the lowest index of each tied pair of references
    assert (bits(d2[1:]) == bits(np.float32(1 / 64) ** 2)).all()
    d = mdu.d2_chain(a, b, 32)
    assert ((d == d.min(1)[:, None]).sum(1)[:80] == 2).all()
    assert (d[np.arange(40), 300 + np.arange(40)] == d.min(1)[:40]).all()  # the partner lies in another slice of 256


def test_zero_padding_leaves_the_bits_alone():
    """the record is padded with zeros to 4, 8, 16 or 32 floats: (0 - 0) * (0 - 0) = +0 and d + 0 == d, on the bits, for
    every distance of the restatement, for +inf (an invalid record's distance) and for +0"""
    pairs = mdu.parity_pairs()
    a, b = pairs[mdu.N1.index(257) * len(mdu.N2) + mdu.N2.index(130)]
    a = a.copy()
    a[5, 0] = np.inf                                                     # as an invalid reference is packed
    b = np.concatenate([b, a[:3]])                                       # distance +0 among them
    for dim in mdu.DIMS:
        dp = next(w for w in (4, 8, 16, 32) if w >= dim)
        pa, pb = np.zeros((len(a), dp), np.float32), np.zeros((len(b), dp), np.float32)
        pa[:, :dim], pb[:, :dim] = a[:, :dim], b[:, :dim]
        plain, padded = mdu.d2_chain(a, b, dim), mdu.d2_chain(pa, pb, dp)
        assert (bits(plain) == bits(padded)).all(), dim
        assert np.isinf(plain[:, 5]).all() and (bits(plain[130:133, :3].diagonal()) == 0).all()
    z = np.float32(0) - np.float32(0)
    assert bits(z * z) == 0 and bits(np.float32(np.inf) + z * z) == bits(np.float32(np.inf))


def test_plan_and_pack_header_alone():
    """tests/cpp/test_match_dims_plan.cpp compiles csrc/match_dims_plan.hpp, the header match_dims.hip packs its records and
    builds its table with, on its own: every query in exactly one item per slice, no item across a pair, 4 * dim bytes read
    of an array's last record, invalid records as (+inf, 0, ...)"""
    subprocess.check_call(["make", "build/test_match_dims_plan"], cwd=ROOT)
    r = subprocess.run([str(ROOT / "build" / "test_match_dims_plan")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_match_dims_plan: ok" in r.stdout, r.stdout + r.stderr
    assert '#include "match_dims_plan.hpp"' in (ROOT / "pointcloudcomparator_amd" / "csrc" / "match_dims.hip").read_text()
    mk = (ROOT / "Makefile").read_text()
    assert "match_dims.hip" in re.search(r"^HIP_SRCS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert re.search(r"^hosttest:.*build/test_match_dims_plan.*build/match_dims_driver", mk, flags=re.M)
    assert re.search(r"^asan:.*build/asan/test_match_dims_plan", mk, flags=re.M)
    assert re.search(r"^build/asan/test_match_dims_plan:.*\n.*\n\t\$\(CXX\).*\$\(SANFLAGS\)", mk, flags=re.M)
