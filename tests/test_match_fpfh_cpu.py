"""pcc_match_fpfh_batch without a GPU: the entry point is declared, exported and bound; it refuses bad arguments before it looks
at any device, in the documented order, and writes nothing then; the NumPy restatement the GPU tests compare with is sensitive to
what it has to pin at 33 bins (the order and the rounding of the sum, bin 32); and the pack header passes its stand-alone
program."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import match_dims_util as mdu  # noqa: E402
import match_fpfh_util as mfu  # noqa: E402

INF = np.float32(np.inf)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_entry_point_is_declared_exported_and_bound():
    from pointcloudcomparator_amd import capi
    header = (ROOT / "include" / "pcc_nn.h").read_text()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+pcc_match_fpfh_batch\s*\(", header, flags=re.S)
    assert m, "pcc_match_fpfh_batch is not declared under a comment of its own"
    comment = m.group(1)
    assert "src/comparator.cpp:877-910" in comment and "LOWEST INDEX" in comment and "PCC_MEM_DEVICE" in comment
    assert header.index("int pcc_match_knn_batch_dims(") < header.index("int pcc_match_fpfh_batch(") < header.index("int pcc_voxel_grid(")
    assert "pcc_match_fpfh_batch" in capi.SYMBOLS
    fn = capi.LIB.pcc_match_fpfh_batch
    assert fn.restype is C.c_int and len(fn.argtypes) == 12
    import inspect
    p = inspect.signature(capi.Index.match_fpfh_batch).parameters
    assert p["threshold"].default == 0.25 and p["return_d2"].default is False
    mirror = (ROOT / "include" / "pcc" / "fpfh.hpp").read_text()
    assert "matchFPFH(" in mirror and "matchFPFHBatch(" in mirror and "no counterpart" not in mirror


def test_refusals_in_their_order_need_no_gpu():
    from pointcloudcomparator_amd import capi
    L = capi.LIB
    a = np.zeros((4, 64), np.float32)
    ptrs, ns = (C.c_void_p * 1)(a.ctypes.data), (C.c_size_t * 1)(4)
    nulls = (C.c_void_p * 1)(None)
    out, d2, off = np.zeros(8, np.int32), np.full(8, 7, np.float32), np.full(2, 99, np.uintp)
    o, d, f = out.ctypes.data, d2.ctypes.data, off.ctypes.data
    thr = np.float32(0.25)

    def call(stride=132, n_pairs=1, d1=ptrs, n1=ns, d2_=ptrs, n2=ns, mem=0, oo=o, dd=d, ff=f):
        return L.pcc_match_fpfh_batch(None, n_pairs, d1, n1, d2_, n2, stride, mem, thr, oo, dd, ff)

    def err():
        return L.pcc_last_error()

    # 1. the memory space, whatever else is wrong
    assert call(mem=7) == -1 and b"mem space" in err()
    assert call(stride=128, mem=7, ff=None, d1=None) == -1 and b"mem space" in err()
    assert call(mem=-1) == -1 and b"mem space" in err()
    # 2. the stride: a multiple of 4 and >= 132, in either memory space, whatever else is wrong
    for stride in (128, 130, 0, 12, 131, 134):
        for mem in (capi.MEM_HOST, capi.MEM_DEVICE):
            assert call(stride=stride, mem=mem) == -1 and b"stride" in err() and b"132" in err(), (stride, mem)
            assert call(stride=stride, mem=mem, ff=None, d1=None, oo=None) == -1 and b"stride" in err()
    # 3. everything pcc_match_knn_batch refuses, with its messages
    for kw in (dict(d1=None), dict(n1=None), dict(d2_=None), dict(n2=None), dict(oo=None), dict(ff=None)):
        for mem in (capi.MEM_HOST, capi.MEM_DEVICE):
            assert call(mem=mem, **kw) == -1
            assert b"null" in err() and b"null index" not in err()
    assert call(d1=nulls) == -1 and b"null point pointer" in err()
    assert call(d2_=nulls) == -1 and b"null point pointer" in err()
    big = (C.c_size_t * 2)(2 ** 30, 2 ** 30)
    two = (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data + 256)
    small = (C.c_size_t * 2)(2, 1)
    assert call(n_pairs=2, d1=two, n1=big, d2_=two, n2=small) == -5 and b"2^31" in err()
    assert call(n_pairs=2, d1=two, n1=small, d2_=two, n2=big) == -5 and b"2^31" in err()
    assert call(n1=(C.c_size_t * 1)(2 ** 31)) == -5
    assert call(n_pairs=2 ** 31, ) == -5 and b"2^31" in err()
    #    ... and a device pointer that is not 4-byte aligned (host arrays are read bytewise: any address will do)
    odd = (C.c_void_p * 1)(a.ctypes.data + 2)
    assert call(mem=capi.MEM_DEVICE, d1=odd) == -1 and b"aligned" in err()
    assert call(mem=capi.MEM_DEVICE, d2_=odd) == -1 and b"aligned" in err()
    assert call(mem=capi.MEM_HOST, d1=odd) == -1 and b"null index" in err()
    # 4. a null handle with good arguments is the last refusal, in either memory space and for every good stride
    for stride in (132, 136, 144, 256):
        for mem in (capi.MEM_HOST, capi.MEM_DEVICE):
            assert call(stride=stride, mem=mem) == -1 and b"null index" in err()
    assert call(dd=None) == -1 and b"null index" in err()                       # out_d2 may be null
    assert call(n_pairs=0, d1=None, n1=None, d2_=None, n2=None, oo=None, dd=None) == -1 and b"null index" in err()
    # nothing was written by any refused call
    assert off.tolist() == [99, 99] and not out.any() and (d2 == 7).all()
    # the 32-dimension cap of the other entry point stands
    assert L.pcc_match_knn_batch_dims(None, 1, ptrs, ns, ptrs, ns, 132, 33, 0, thr, o, d, f) == -5 and b"1 ... 32" in err()


def test_python_wrapper_refuses_a_mixture_before_any_call():
    from pointcloudcomparator_amd import capi

    class FakeCuda:  # (what the wrapper asks of a tensor before it decides; no device is needed to refuse)
        __module__ = "torch.fake"
        is_cuda = True
        ndim = 2
        shape = (4, 33)

    ix = capi.Index.__new__(capi.Index)  # (no handle: the refusal comes first)
    ix._h, ix.auto_sync = None, True
    with pytest.raises(ValueError, match="not both"):
        ix.match_fpfh_batch([(np.zeros((4, 33), np.float32), FakeCuda())])
    with pytest.raises(ValueError, match="not both"):
        ix.match_fpfh_batch([(np.zeros((4, 33), np.float32), np.zeros((2, 33), np.float32)), (FakeCuda(), FakeCuda())])


def test_the_restatement_is_sensitive_at_33_bins():
    """on the parity inputs: a contracted multiply-add chain and another summation order change distance bits in both families,
    and a search that stops at bin 31 returns other rows -- a kernel that did any of these would fail the GPU parity test"""
    pairs = mfu.parity_pairs()
    assert len(pairs) == 35 and all(a.shape[1] == 33 and b.shape[1] == 33 and a.dtype == np.float32 for a, b in pairs)
    fma = pw = 0
    per_family = {f: [0, 0] for f in mfu.FAMILIES}
    for k, (a, b) in enumerate(pairs):
        fam = mfu.family_of(k // len(mfu.N2), k % len(mfu.N2))
        chain = mdu.d2_chain(a, b, 33)
        n_fma = int((bits(chain) != bits(mdu.d2_fma(a, b, 33))).sum())
        n_pw = int((bits(chain) != bits(mdu.d2_pairwise(a, b, 33))).sum())
        fma, pw = fma + n_fma, pw + n_pw
        per_family[fam][0] += n_fma
        per_family[fam][1] += n_pw
    assert fma > 0 and pw > 0, (fma, pw)
    assert per_family["fpfh-like"][0] > 0 and per_family["fpfh-like"][1] > 0, per_family
    free = [mdu.restate(a, b, 33, INF) for a, b in pairs]
    thr = np.float32(np.median(np.concatenate([w[1][1:] for w in free])))
    differ = 0
    for a, b in pairs:
        r33, r32 = mdu.restate(a, b, 33, thr), mdu.restate(a, b, 32, thr)
        differ += int(len(r33[0]) != len(r32[0]) or not np.array_equal(r33[0], r32[0]) or not np.array_equal(bits(r33[1]), bits(r32[1])))
    assert differ > 0, "bin 32 changes nothing on the parity inputs: the GPU test would pin nothing about it"


def test_the_planted_cases_are_what_the_gpu_tests_say():
    a, b, perm = mfu.bin32_pair()
    assert a.shape == (300, 33) and b.shape == (130, 33)
    assert np.array_equal(mdu.restate(a, b, 33, 0.25)[0][1:], perm)
    assert np.array_equal(mdu.restate(a, b, 32, 0.25)[0], np.zeros(131, np.int32))     # 32 bins see one point
    a, b = mfu.tie_pair()
    row, d2, n_tied = mdu.restate(a, b, 33, 0.25)
    assert n_tied == 80 and row[1:].tolist() == list(range(100))
    assert (bits(d2[1:]) == bits(np.float32(1 / 64) ** 2)).all()
    d = mdu.d2_chain(a, b, 33)
    assert ((d == d.min(1)[:, None]).sum(1)[:80] == 2).all() and ((d == d.min(1)[:, None]).sum(1)[80:] == 1).all()
    assert (d[np.arange(40), 300 + np.arange(40)] == d.min(1)[:40]).all()              # the partner lies in another slice of 256
    assert (mdu.restate(a, b, 32, 0.25)[1] == 0).all()                                 # bin 32 supplies the whole distance


def test_zero_padding_to_36_leaves_the_bits_alone():
    a, b = mfu.parity_pairs()[mfu.N1.index(257) * len(mfu.N2) + mfu.N2.index(130)]
    a = a.copy()
    a[5, 0] = np.inf                                                     # as an invalid reference is packed
    b = np.concatenate([b, a[:3]])                                       # distance +0 among them
    pa, pb = np.zeros((len(a), 36), np.float32), np.zeros((len(b), 36), np.float32)
    pa[:, :33], pb[:, :33] = a, b
    plain, padded = mdu.d2_chain(a, b, 33), mdu.d2_chain(pa, pb, 36)
    assert (bits(plain) == bits(padded)).all()
    assert np.isinf(plain[:, 5]).all() and (bits(plain[130:133, :3].diagonal()) == 0).all()


def test_pack_header_alone_and_the_build_lists():
    """tests/cpp/test_match_fpfh_plan.cpp compiles csrc/match_fpfh_plan.hpp, the header match_fpfh.hip packs its records with, on
    its own: +0 padding, (+inf, 0, ...) for a non-finite bin 32, 132 bytes read of every record"""
    subprocess.check_call(["make", "build/test_match_fpfh_plan"], cwd=ROOT)
    r = subprocess.run([str(ROOT / "build" / "test_match_fpfh_plan")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_match_fpfh_plan: ok" in r.stdout, r.stdout + r.stderr
    assert '#include "match_fpfh_plan.hpp"' in (ROOT / "pointcloudcomparator_amd" / "csrc" / "match_fpfh.hip").read_text()
    mk = (ROOT / "Makefile").read_text()
    assert "match_fpfh.hip" in re.search(r"^HIP_SRCS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert re.search(r"^hosttest:.*build/test_match_fpfh_plan.*build/fpfh_match_driver", mk, flags=re.M)
    assert re.search(r"^asan:.*build/asan/test_match_dims_plan build/asan/test_match_fpfh_plan", mk, flags=re.M)
    assert re.search(r"^build/asan/test_match_fpfh_plan:.*\n.*\n\t\$\(CXX\).*\$\(SANFLAGS\)", mk, flags=re.M)
