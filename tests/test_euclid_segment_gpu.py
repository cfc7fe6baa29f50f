"""pcc_euclidean_cluster_segmentation / Index.euclidean_cluster_segmentation: the reference's -e segmentation path
(src/segmentation.cpp:64-156) in one call, against the sequence of existing GPU calls it replaces (bit for bit) and against the
oracle chain (oracle.voxel_grid -> the loop of oracle.sac_plane + np.delete -> oracle.euclidean_clusters(0.05, 100, 250000)).

The scenes are tests/euclid_segment_util.py's; what the oracle chain gives for them (computed on the CPU, FIGURES there):
  rooms         3351 points, one per 0.025 voxel: planes of 1296 / 1296 (74 / 16 iterations), 759 remain, clusters of 252 / 216 /
                216 -- the two equal boxes numbered by their lowest member, 0 before 261 --, 75 points labelled -1
  rooms+nan     rooms with one NaN: 3350 filtered, planes of 1296 / 1295 (78 / 16), the same clusters
  big_rooms     19 504 points: planes of 7056 / 7056 (95 / 23), 5392 remain (the clustering's cells form, from 4096), clusters of
                1872 / 1728 / 1728, 64 labelled -1
  dyadic_rooms  16 056 points on a 2^-12 lattice, 7988 voxels: planes of 3209 / 3173 (69 / 14), 1606 remain, clusters of 581 / 465 /
                460 / 100 (the last exactly at min_size).  Every sum of a voxel is exact in any order, so the oracle's centroids are
                the library's in every bit"""
import numpy as np
import pytest

from pointcloudcomparator_amd import capi
from euclid_segment_util import (FIGURES, assert_same_result, figures_of, lattice2500, oracle_chain, oracle_chain_on, same_bits, scene, sequence,
                                 to_numpy, with_colour)
from plane_removal_util import lattice

pytestmark = pytest.mark.gpu
NAMES = ("rooms", "rooms+nan", "big_rooms", "dyadic_rooms")


@pytest.fixture(scope="module")
def ctx(gpu):
    with capi.Index(np.zeros((1, 3), np.float32)) as ix:
        yield ix


@pytest.fixture(scope="module")
def results(ctx):
    """the one call over every scene, once"""
    return {name: ctx.euclidean_cluster_segmentation(scene(name)) for name in NAMES}


def check_figures(res, name):
    points, filtered, planes, remaining, sizes, lowest, left_out = FIGURES[name]
    got = figures_of(res)
    assert len(scene(name)) == points
    assert got[:4] == (filtered, planes, remaining, sizes) and got[5] == left_out, got
    if lowest is not None:
        assert got[4] == lowest
    assert not res["ended_without_model"]


@pytest.mark.parametrize("name", NAMES)
def test_one_call_equals_the_sequence_of_existing_calls(ctx, results, name):
    got = results[name]
    want = sequence(ctx, scene(name))
    check_figures(want, name)
    assert_same_result(got, want)
    assert list(np.diff(got["offsets"])) == FIGURES[name][4]
    # the cluster clouds are the remaining records of the index list
    assert same_bits(got["cluster_points"], got["points"][got["cluster_index"]])


@pytest.mark.parametrize("name", NAMES)
def test_one_call_equals_the_oracle_chain(results, name):
    want = oracle_chain(name)
    check_figures(want, name)  # (a drifting scene shows here)
    got = results[name]
    assert got["n_filtered"] == want["n_filtered"]
    assert same_bits(got["points"], want["points"])  # (one point per voxel, or exact sums: the centroids are the oracle's)
    np.testing.assert_array_equal(got["plane_sizes"], want["plane_sizes"])
    np.testing.assert_array_equal(got["iterations"], want["iterations"])
    assert same_bits(got["coefficients"], want["coefficients"])
    assert got["n_clusters"] == want["n_clusters"]
    np.testing.assert_array_equal(got["labels"], want["labels"])  # (cluster order with its ties)
    assert list(np.diff(got["offsets"])) == FIGURES[name][4] == want["cluster_sizes"]
    assert got["ended_without_model"] == want["ended_without_model"]


def test_colour_records(ctx, results):
    rec = with_colour(scene("rooms"))
    got = ctx.euclidean_cluster_segmentation(rec, has_rgb=True)
    assert_same_result(got, sequence(ctx, rec, has_rgb=True))
    p, c = got["points"].view(np.uint32), got["cluster_points"].view(np.uint32)
    # x, y, z, 1.0f, the colour word (one point per voxel: its own), 12 zero bytes
    assert (got["points"][:, 3] == 1.0).all() and (p[:, 5:] == 0).all() and (c[:, 5:] == 0).all()
    assert len(np.unique(c[:, 4])) > 500 and (c[:, 4] >> 24 == 0).all()
    assert set(map(int, c[:, 4])) <= set(map(int, rec.view(np.uint32)[:, 4]))
    assert same_bits(got["cluster_points"], got["points"][got["cluster_index"]])
    # and nothing but the records depends on the colour
    plain = results["rooms"]
    assert same_bits(got["points"][:, :3], plain["points"]) and same_bits(got["coefficients"], plain["coefficients"])
    for key in ("labels", "offsets", "cluster_index", "plane_sizes", "iterations"):
        np.testing.assert_array_equal(got[key], plain[key], err_msg=key)
    assert got["n_filtered"] == plain["n_filtered"] and got["n_clusters"] == plain["n_clusters"]


def test_other_cluster_sizes(ctx):
    kw = dict(min_size=1, max_size=250)
    got = ctx.euclidean_cluster_segmentation(scene("rooms"), **kw)
    want = oracle_chain_on(scene("rooms"), **kw)
    assert want["cluster_sizes"] == [216, 216, 75]  # (the box of 252 is above max_size)
    assert list(np.diff(got["offsets"])) == [216, 216, 75] and got["n_clusters"] == 3
    np.testing.assert_array_equal(got["labels"], want["labels"])
    assert_same_result(got, sequence(ctx, scene("rooms"), **kw))


def test_no_plane_taken(ctx):
    got = ctx.euclidean_cluster_segmentation(scene("rooms"), stop_fraction=1.0)
    want = oracle_chain_on(scene("rooms"), stop_fraction=1.0)
    assert len(want["plane_sizes"]) == 0 and len(want["points"]) == 3351
    assert len(got["plane_sizes"]) == 0 and got["coefficients"].shape == (0, 4) and len(got["points"]) == 3351
    assert same_bits(got["points"], want["points"]) and got["n_clusters"] == want["n_clusters"] >= 1
    np.testing.assert_array_equal(got["labels"], want["labels"])
    assert list(np.diff(got["offsets"])) == want["cluster_sizes"]
    assert_same_result(got, sequence(ctx, scene("rooms"), stop_fraction=1.0))


@pytest.mark.parametrize("n", [2500, 2048])
def test_many_clusters(ctx, n):
    """2500 clusters of one point: the host sort above 2048 clusters and the two-digit extraction; 2048: the rank kernel full"""
    pts = np.ascontiguousarray(lattice2500()[:n])
    got = ctx.euclidean_cluster_segmentation(pts, stop_fraction=1.0, min_size=1, max_clusters=4096)
    assert got["n_filtered"] == n and len(got["points"]) == n and got["n_clusters"] == n
    # one point per cluster: sizes tie everywhere, so the order is the lowest member's, the point's own index
    np.testing.assert_array_equal(got["labels"], np.arange(n))
    np.testing.assert_array_equal(got["offsets"], np.arange(n + 1))
    np.testing.assert_array_equal(got["cluster_index"], np.arange(n))
    assert same_bits(got["cluster_points"], got["points"])
    assert ctx.stats()[0:5] == [n, n, n, 0, 0]


@pytest.mark.parametrize("case", ["one", "two", "nan", "empty", "lattice"])
def test_small_clouds(ctx, case):
    pts = {"one": np.array([[1.0, 2.0, 3.0]], np.float32), "two": np.array([[1.0, 2.0, 3.0], [2.0, 2.0, 3.0]], np.float32),
           "nan": np.full((40, 3), np.nan, np.float32), "empty": np.zeros((0, 3), np.float32), "lattice": lattice()}[case]
    kw = dict(stop_fraction=0.0) if case == "lattice" else {}
    got = ctx.euclidean_cluster_segmentation(pts, **kw)
    assert got["n_clusters"] == 0 and list(got["offsets"]) == [0] and len(got["cluster_index"]) == 0
    if case in ("nan", "empty"):
        assert got["n_filtered"] == 0 and len(got["points"]) == 0 and len(got["plane_sizes"]) == 0 and not got["ended_without_model"]
        assert ctx.stats()[0:5] == [0, 0, 0, 0, 0]
    if case == "one":
        assert got["n_filtered"] == 1 and same_bits(got["points"], pts) and got["ended_without_model"] and list(got["labels"]) == [-1]
    if case == "two":
        assert got["ended_without_model"] and len(got["points"]) == 2 and len(got["plane_sizes"]) == 0 and list(got["labels"]) == [-1, -1]
    if case == "lattice":
        assert got["n_filtered"] == 49 and list(got["plane_sizes"]) == [49] and len(got["points"]) == 0 and len(got["labels"]) == 0
        assert not got["ended_without_model"] and ctx.stats()[0:4] == [49, 0, 0, 1]
    assert_same_result(got, sequence(ctx, pts, **kw))


def test_more_clusters_than_room(ctx, results):
    with pytest.raises(capi.PccError) as e:
        ctx.euclidean_cluster_segmentation(scene("rooms"), max_clusters=2)
    assert e.value.status == -6 and "max_clusters" in str(e.value)
    part, full = e.value.partial, results["rooms"]
    assert part["n_clusters"] == 3 and part["n_filtered"] == 3351
    assert same_bits(part["points"], full["points"]) and same_bits(part["coefficients"], full["coefficients"])
    for key in ("labels", "plane_sizes", "iterations"):
        np.testing.assert_array_equal(part[key], full[key], err_msg=key)
    assert ctx.euclidean_cluster_segmentation(scene("rooms"), max_clusters=3)["n_clusters"] == 3


def test_more_planes_than_room(ctx, results):
    with pytest.raises(capi.PccError) as e:
        ctx.euclidean_cluster_segmentation(scene("rooms"), max_planes=1)
    assert e.value.status == -6 and "max_planes" in str(e.value)
    part, full = e.value.partial, results["rooms"]
    assert len(part["plane_sizes"]) == 1 and part["n_filtered"] == 3351
    assert list(part["plane_sizes"]) == [1296] and same_bits(part["coefficients"], full["coefficients"][:1])
    assert ctx.euclidean_cluster_segmentation(scene("rooms"), max_planes=2)["n_clusters"] == 3


def test_device_memory_equals_host_memory(ctx, results):
    import torch
    colour = with_colour(scene("rooms"))
    for name, cloud in (("rooms+nan", scene("rooms+nan")), ("colour", colour)):
        host = results[name] if name in results else ctx.euclidean_cluster_segmentation(cloud, has_rgb=True)
        dev = ctx.euclidean_cluster_segmentation(torch.from_numpy(np.array(cloud)).cuda(), has_rgb=name == "colour")
        assert all(dev[key].is_cuda for key in ("points", "labels", "cluster_points", "cluster_index"))
        assert_same_result(dev, host)
        if name == "colour":
            assert (to_numpy(dev["points"]).view(np.uint32)[:, 5:] == 0).all()


def test_ctx_is_untouched_and_the_work_handle_is_reused(gpu):
    rng = np.random.default_rng(8)
    other = rng.random((500, 3)).astype(np.float32)
    queries = rng.random((64, 3)).astype(np.float32)
    from segment_util import assert_same_result as assert_same_growing, scene as growing_scene
    with capi.Index(other, engine=capi.ENGINE_GRID) as ix:
        before = ix.knn(queries, 7)
        first = ix.euclidean_cluster_segmentation(scene("rooms"))
        after = ix.knn(queries, 7)
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        assert ix.size == 500
        second = ix.euclidean_cluster_segmentation(scene("rooms"))
        assert_same_result(second, first)
        assert ix.stats()[0:5] == [3351, 3, 684, 2, 0]
        # a cloud of another size in between, then the first again
        ix.euclidean_cluster_segmentation(scene("dyadic_rooms"))
        assert ix.stats()[0:4] == [7988, 4, 1606, 2]
        assert_same_result(ix.euclidean_cluster_segmentation(scene("rooms")), first)
        # the default path's call shares the work handle: either one in between changes nothing in the other
        grown = ix.region_growing_segmentation(growing_scene("walls27"))
        assert_same_result(ix.euclidean_cluster_segmentation(scene("rooms")), first)
        assert_same_growing(ix.region_growing_segmentation(growing_scene("walls27")), grown)
        assert ix.knn(queries, 7)[0].tobytes() == before[0].tobytes()
