"""pcc_region_growing_segmentation / Index.region_growing_segmentation: the reference's default segmentation path
(src/segmentation.cpp:218-327) in one call, against the sequence of existing GPU calls it replaces (bit for bit) and against the
oracle chain of tests/test_cli_gpu.py.

The scenes are tests/segment_util.py's; what the oracle chain gives for them (computed on the CPU):
  walls27               2187 points, one per 0.025 voxel: 2187 filtered points, 3 clusters of 729 / 729 / 729
  walls27+clutter+nan   2227 points, one of them NaN: 2226 filtered points, 3 clusters of 729 / 728 / 729, 40 points labelled -1
  dyadic52              8112 points on a 2^-12 lattice: 4949 voxels (3163 points share a voxel with another), 3 clusters.  Every
                        double sum is exact in any order, so the one call and the sequence must agree in every bit; its centroids
                        are NOT compared with oracle.voxel_grid, which sums in float"""
import numpy as np
import pytest

from pointcloudcomparator_amd import capi
from segment_util import assert_same_result, oracle_chain, plate60, same_bits, scene, sequence, with_colour

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    with capi.Index(np.zeros((1, 3), np.float32)) as ix:
        yield ix


@pytest.fixture(scope="module")
def results(ctx):
    """the one call over every scene, once"""
    return {name: ctx.region_growing_segmentation(scene(name)) for name in ("walls27", "walls27+clutter+nan", "dyadic52")}


# (scene, filtered points, cluster sizes, points labelled -1): the oracle's figures, as recorded above
FIGURES = [
    ("walls27", 2187, [729, 729, 729], 0),
    ("walls27+clutter+nan", 2226, [729, 728, 729], 40),
    ("dyadic52", 4949, None, None),
]


@pytest.mark.parametrize("name,nv,sizes,left_out", FIGURES)
def test_one_call_equals_the_sequence_of_existing_calls(ctx, results, name, nv, sizes, left_out):
    got = results[name]
    want = sequence(ctx, scene(name))
    assert len(want["filtered"]) == nv and want["n_clusters"] == 3
    assert_same_result(got, want)
    if sizes is not None:
        assert list(np.diff(got["offsets"])) == sizes and int((got["labels"] < 0).sum()) == left_out
    # the cluster clouds are the filtered records of the index list
    assert same_bits(got["cluster_points"], got["filtered"][got["cluster_index"]])


@pytest.mark.parametrize("name,nv,sizes,left_out", FIGURES[:2])
def test_one_call_equals_the_oracle_chain(results, name, nv, sizes, left_out):
    vox, nrm, lab, ncl = oracle_chain(name)
    assert (len(vox), ncl, list(np.bincount(lab[lab >= 0])), int((lab < 0).sum())) == (nv, 3, sizes, left_out)
    got = results[name]
    assert same_bits(got["filtered"], vox)  # (one point per voxel: the centroids are the points themselves)
    assert got["n_clusters"] == ncl
    np.testing.assert_array_equal(got["labels"], lab)
    same = (got["normals"].view(np.uint32) == nrm.view(np.uint32)) | (np.isnan(got["normals"]) & np.isnan(nrm))
    assert same.all(), (int((~same.all(1)).sum()), len(same))  # as tests/test_normals_gpu.py asserts for pcc_normals
    assert list(np.diff(got["offsets"])) == sizes


def test_colour_records(ctx):
    rec = with_colour(scene("dyadic52"))
    got = ctx.region_growing_segmentation(rec, has_rgb=True)
    want_filtered = ctx.voxel_grid(rec, 0.025, has_rgb=True)
    assert len(want_filtered) == 4949 and same_bits(got["filtered"], want_filtered)
    f = got["filtered"].view(np.uint32)
    assert (got["filtered"][:, 3] == 1.0).all() and (f[:, 5:] == 0).all()  # x, y, z, 1.0f, the colour word, 12 zero bytes
    assert len(np.unique(f[:, 4])) > 1000 and (f[:, 4] >> 24 == 0).all()
    # the cluster records carry the averaged colour word
    assert same_bits(got["cluster_points"], got["filtered"][got["cluster_index"]])
    assert_same_result(got, sequence(ctx, rec, has_rgb=True))
    # and nothing but the records depends on the colour
    plain = ctx.region_growing_segmentation(scene("dyadic52"))
    assert same_bits(got["filtered"][:, :3], plain["filtered"]) and same_bits(got["normals"], plain["normals"])
    np.testing.assert_array_equal(got["labels"], plain["labels"])


@pytest.mark.parametrize("case", ["one", "plate60", "nan", "empty"])
def test_small_clouds(ctx, case):
    pts = {"one": np.array([[1.0, 2.0, 3.0]], np.float32), "plate60": plate60(), "nan": np.full((40, 3), np.nan, np.float32),
           "empty": np.zeros((0, 3), np.float32)}[case]
    got = ctx.region_growing_segmentation(pts)
    if case in ("nan", "empty"):
        assert len(got["filtered"]) == 0 and got["n_clusters"] == 0 and list(got["offsets"]) == [0]
        assert ctx.stats()[0:3] == [0, 0, 0]
    assert_same_result(got, sequence(ctx, pts))  # (NaN normals -- fewer than 3 neighbours -- compare as bits)
    if case == "one":
        assert len(got["filtered"]) == 1 and same_bits(got["filtered"], pts) and np.isnan(got["normals"]).all()
    if case == "plate60":
        assert len(got["filtered"]) == 60 and got["n_clusters"] == 1 and list(got["offsets"]) == [0, 60]


def test_more_clusters_than_room(ctx, results):
    with pytest.raises(capi.PccError) as e:
        ctx.region_growing_segmentation(scene("walls27"), max_clusters=2)
    assert e.value.status == -6 and "max_clusters" in str(e.value)
    part, full = e.value.partial, results["walls27"]
    assert part["n_clusters"] == 3
    assert same_bits(part["filtered"], full["filtered"]) and same_bits(part["normals"], full["normals"])
    np.testing.assert_array_equal(part["labels"], full["labels"])
    assert ctx.region_growing_segmentation(scene("walls27"), max_clusters=3)["n_clusters"] == 3


def test_device_memory_equals_host_memory(ctx, results):
    import torch
    for name, cloud in (("walls27+clutter+nan", scene("walls27+clutter+nan")), ("colour", with_colour(scene("dyadic52")))):
        host = results[name] if name in results else ctx.region_growing_segmentation(cloud, has_rgb=True)
        dev = ctx.region_growing_segmentation(torch.from_numpy(np.array(cloud)).cuda(), has_rgb=name == "colour")
        assert all(dev[key].is_cuda for key in ("filtered", "normals", "labels", "cluster_points", "cluster_index"))
        assert_same_result(dev, host)


def test_ctx_is_untouched_and_the_work_handle_is_reused(gpu):
    rng = np.random.default_rng(8)
    other = rng.random((500, 3)).astype(np.float32)
    queries = rng.random((64, 3)).astype(np.float32)
    with capi.Index(other, engine=capi.ENGINE_GRID) as ix:
        before = ix.knn(queries, 7)
        first = ix.region_growing_segmentation(scene("walls27"))
        after = ix.knn(queries, 7)
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        assert ix.size == 500
        second = ix.region_growing_segmentation(scene("walls27"))
        assert_same_result(second, first)
        stats = ix.stats()
        assert stats[0:3] == [2187, 3, 2187] and stats[7] >= 1
        # a cloud of another size in between, then the first again
        ix.region_growing_segmentation(scene("walls27+clutter+nan"))
        assert ix.stats()[0:3] == [2226, 3, 2186]
        assert_same_result(ix.region_growing_segmentation(scene("walls27")), first)
        assert ix.knn(queries, 7)[0].tobytes() == before[0].tobytes()
