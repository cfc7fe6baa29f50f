/*
 * pcc_nn.h -- C-ABI of libpcc_nn: the MI355X (gfx950) nearest-neighbour /
 * radius-search engine that replaces the pcl::KdTreeFLANN path of
 * adr-arroyo/PointCloudComparator.
 *
 * The reference has no FFI layer: it calls PCL C++ classes one query at a time
 * (SURVEY.md 8b).  Each entry point below names the reference interface it
 * replaces (file:line relative to the reference tree).  Everything is plain C:
 * opaque handle, pointers, sizes, int status.  No allocation crosses the ABI;
 * outputs are caller-allocated.
 *
 * Memory spaces: every data pointer is tagged by a `mem` argument --
 * PCC_MEM_HOST (library copies H2D/D2H itself) or PCC_MEM_DEVICE (pointer is
 * HBM on the index's device; results are written to device memory on the
 * index's stream and the call returns without synchronising).
 *
 * Points are AoS with a byte stride; the first `dim` floats of each element
 * are the coordinates.  dim must be 3 -- that is what every hot call site of
 * the reference searches on (pcl::PointXYZRGB 32 B, pcl::PointXYZ 16 B, and
 * pcl::Histogram<32> 128 B through PCL's 3-float DefaultPointRepresentation,
 * SURVEY.md 3.2 / 9.1).
 *
 * Semantics shared by all searches:
 *   - reference points with a non-finite coordinate are skipped; returned
 *     indices are positions in the ORIGINAL cloud (PCL index_mapping_);
 *   - d2 = ((dx*dx)+dy*dy)+dz*dz in fp32, every op rounded separately
 *     (FLANN L2_Simple<float>); distances are SQUARED;
 *   - exact-distance ties resolve to the LOWEST original index;
 *   - a non-finite query never aborts: idx = -1, d2 = +inf, count = 0.
 *   - a squared distance that overflows float (>= FLT_MAX) is no neighbour, as in FLANN (its result sets start
 *     with worst_distance = FLT_MAX and reject dist >= worst): idx = -1, d2 = +inf.
 */
#ifndef PCC_NN_H
#define PCC_NN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PCC_VERSION 100

typedef struct pcc_index pcc_index;

enum pcc_status {
    PCC_OK = 0,
    PCC_ERR_INVALID = -1,     /* bad argument */
    PCC_ERR_EMPTY = -2,       /* no valid reference point ("Cannot create a KDTree with an empty input cloud") */
    PCC_ERR_DEVICE = -3,      /* HIP runtime failure (no GPU, launch error, ...) */
    PCC_ERR_NOMEM = -4,
    PCC_ERR_UNSUPPORTED = -5, /* dim != 3, k too large, ... */
    PCC_ERR_OVERFLOW = -6,    /* caller-provided output capacity too small */
    PCC_ERR_INTERNAL = -7     /* the library caught itself in a state it rules out (a bounded loop that ran out): a bug to report */
};
enum pcc_mem { PCC_MEM_HOST = 0, PCC_MEM_DEVICE = 1 };
/* search engine behind an index.  Both are exact and return identical bits.
 *   BRUTE: tiled exhaustive scan (query tile in registers, reference tile in LDS)
 *   GRID : cell-sorted references, exact ring search with conservative bounds,
 *          BRUTE fallback for queries the rings do not resolve
 *   AUTO : GRID when the cloud is large enough to amortise its build. */
enum pcc_engine { PCC_ENGINE_AUTO = 0, PCC_ENGINE_BRUTE = 1, PCC_ENGINE_GRID = 2 };
/* which of several references at EXACTLY the same distance a k = 1 search names.
 *   LOWEST_INDEX: the lowest original index (default; what every engine computes on the GPU)
 *   FLANN       : the one pcl::KdTreeFLANN returns -- the first its kd-tree walk reaches.  The GPU
 *                 result is kept for every query whose minimiser is unique; queries with a second reference at
 *                 the same distance are flagged on the GPU and only those are walked through a host-side
 *                 restatement of FLANN's KDTreeSingleIndex (built once per indexed cloud).  Applies to pcc_nn1
 *                 and pcc_match_knn (the call sites that hand indices on, src/comparator.cpp:576-580); distances
 *                 are the same bits either way. */
enum pcc_ties { PCC_TIES_LOWEST_INDEX = 0, PCC_TIES_FLANN = 1 };

#define PCC_KNN_MAX_K 65536 /* k <= 512: wave-cooperative selection; larger k works, one lane per query with O(k) insertion */

int pcc_version(void);
/* thread-local message for the last non-OK status returned on this thread */
const char *pcc_last_error(void);
int pcc_device_count(int *count);

/* ---- index lifetime -------------------------------------------------------
 * replaces: pcl::KdTreeFLANN<T> ctor + setInputCloud (src/comparator.cpp:564-565),
 *           pcl::search::KdTree<T>::setInputCloud (src/segmentation.cpp:120-122)
 *           and the trees ICP / SOR / EC build internally
 *           (src/comparator.cpp:1096,1527,1541; src/segmentation.cpp:131).
 * Copies (uploads) the cloud; the caller may free `pts` after the call. */
int pcc_index_create(const void *pts, size_t n, size_t stride_bytes, int dim,
                     int mem, int device, int engine, pcc_index **out);
int pcc_index_destroy(pcc_index *index);
/* KdTreeFLANN::setInputCloud on an existing object (cleanup + rebuild):
 * replaces the indexed cloud, reusing the handle's device allocations.  On error
 * the index is left empty (searches return PCC_ERR_EMPTY). */
int pcc_index_set_input(pcc_index *index, const void *pts, size_t n, size_t stride_bytes,
                        int dim, int mem);
/* One index per device from one upload (every GPU holds the full reference cloud, queries are
 * sharded): the packed cloud of `src` is copied device-to-device (hipMemcpyPeerAsync over xGMI) into a new
 * handle on `device` and indexed there -- rebuilding the grid (~0.1 ms per million points) is cheaper than
 * shipping it.  Same cloud, same indices, same engine; `src` and `device` may be the same device (a second
 * handle with its own stream).  The reference is single-GPU code; this is what its one tree per search site
 * (src/comparator.cpp:564-565) becomes when the query loop is spread over several GPUs of a node. */
int pcc_index_clone_to_device(pcc_index *src, int device, pcc_index **out);
/* The same for `count` devices at once (an entry of devices[] may repeat, or name src's own device): every peer copy
 * is issued before any of them is waited for -- each goes over its own xGMI link --, the builds follow on the clones'
 * own streams, one join at the end.  out[count] receives the handles; on failure none is left behind.  Options, tie
 * order and the requested engine of `src` carry over.  (The reference cloud is "broadcast once" this way in the C++
 * host path; the Python bench uses torch.distributed.broadcast = RCCL for the same step.) */
int pcc_index_clone_to_devices(pcc_index *src, const int *devices, int count, pcc_index **out);
/* number of valid (finite) reference points == PCL total_nr_points_ */
int pcc_index_size(const pcc_index *index, size_t *n_valid);
/* run this index's work on a caller-owned hipStream_t (NULL = library stream) */
int pcc_index_set_stream(pcc_index *index, void *hip_stream);
int pcc_index_sync(pcc_index *index);
/* Device-memory calls (PCC_MEM_DEVICE) are enqueued on the index's stream and return at once.  A caller
 * that produces its inputs or consumes the outputs on ANOTHER stream of the same device orders the two
 * without blocking the host (hipEventRecord + hipStreamWaitEvent):
 *   pcc_index_wait_stream: work submitted to the index after this call starts only when everything
 *     submitted so far to `producer_stream` (a hipStream_t; NULL = the legacy default stream) has finished;
 *   pcc_stream_wait_index: work submitted to `consumer_stream` after this call waits for everything the
 *     index has been asked to do so far.
 * (The reference is single-threaded host code, src/comparator.cpp:571-577: this is what "the call has
 * returned, the vectors are filled" becomes for asynchronous device buffers.) */
int pcc_index_wait_stream(pcc_index *index, void *producer_stream);
int pcc_stream_wait_index(pcc_index *index, void *consumer_stream);
/* engine actually in use (PCC_ENGINE_BRUTE or PCC_ENGINE_GRID) */
int pcc_index_engine(const pcc_index *index, int *engine);
/* force the engine for subsequent searches on this index */
int pcc_index_set_engine(pcc_index *index, int engine);

int pcc_index_set_tie_order(pcc_index *index, int ties);

/* Tuning knobs of one handle.  None of them changes a result bit of a SEARCH (every mode is exact; PCC_OPT_ICP_SORTED is the
 * one knob that shows in a result -- the order a double sum is added up in, see there); they select between
 * implementations that the tests compare with each other and that measurements are taken with.  The PCC_*
 * environment variables of the same names give the DEFAULTS a new handle starts with; the library does not read
 * the environment anywhere else.  Options that shape the index (GRID_PPC, GRID_TRIM, SORT_MP_MIN)
 * take effect at the next pcc_index_set_input.  (The reference has no such surface -- PCL's KdTreeFLANN exposes
 * only setEpsilon / setSortedResults, src/comparator.cpp:564 uses neither.) */
enum pcc_option {
    PCC_OPT_GRID_PPC = 1,        /* mean references per cell the grid aims for (default 0.75) */
    PCC_OPT_GRID_TRIM = 2,       /* k of the trimmed bounding box the grid is laid over (default 3; 0 = plain box) */
    PCC_OPT_FAR_MODE = 3,        /* queries the cell walk leaves: -1 auto, 0 exhaustive kernel, 1 seed scan + ball walk */
    PCC_OPT_ICP_WARM = 4,        /* pcc_icp_align: passes start from the previous pass's neighbours (default 1) */
    PCC_OPT_ICP_DEVICE_LOOP = 5, /* pcc_icp_align: loop resident on the device (default 1; 0 = host-driven, same bits) */
    PCC_OPT_EC_CELLS = 6,        /* clustering over the clique-cell grid: 3 = union-find over the CELLS -- the runs of touching cells along a
                                    row joined by plain stores, one union per pair of neighbouring runs, the rest settled against flat
                                    roots through the caches (default); 4 = the same with one union per occupied cell and face (round 5);
                                    1 = one parent word per point, lanes over a cell's neighbour cells; 2 = the same with lanes over
                                    points; 0 = per-point ball scan on the search grid */
    PCC_OPT_SORT_MP_MIN = 7,     /* reference clouds from this size take the three-level cell sort */
    PCC_OPT_SORT_MP_MIN_Q = 8,   /* the same for query clouds */
    PCC_OPT_NN1_KERNEL = 9,      /* pruned k = 1 kernel: 0 one lane per query; 1 rows drained with lanes over candidates (default);
                                    2 / 3 the same with the open lanes always listed for a second kernel / always finished in place */
    PCC_OPT_FLANN_SPLIT = 10,    /* PCC_TIES_FLANN: split rule replayed, 0 = middleSplit_ (FLANN 1.8.x divideTree), 1 = middleSplit */
    PCC_OPT_NN1_DENSE_MIN = 11,  /* flat k = 1 kernel: a wave whose queries' own cells hold at least this many references on average
                                    takes its first bound from the own cell instead of the own row (default 4) */
    PCC_OPT_KNN_KERNEL = 12,     /* k-NN, k <= 512: 1 = selection by distance buckets, the merge network only for the queries it
                                    hands back (default); 0 = the merge network for every query */
    PCC_OPT_KNN_CACHE_K = 13,    /* 0 (default): off.  K > 0: the self k-NN rows behind pcc_normals / pcc_region_growing are searched
                                    with at least K neighbours and KEPT on the device until the next pcc_index_set_input; a later call
                                    that needs no more than the kept rows hold takes their prefix instead of searching again (the
                                    reference's default segmentation: normals with 50, then region growing with 100 neighbours of the
                                    same cloud -- one search instead of two).  Costs n x K x 8 bytes of device memory */
    PCC_OPT_NN1_OPEN_FLAT = 14,  /* flat k = 1 kernel, listed open lanes: 1 = their rows drained with lanes over candidates (default),
                                    0 = one lane per listed query (round 3) */
    PCC_OPT_SORT_STAGE1 = 15,    /* three-level cell sort, level 1: 1 = reference points leave in bucket-sorted LDS tiles, whole runs
                                    stored (default); 0 = one store per point; 2 = tiles for the queries' 8-byte pairs too */
    PCC_OPT_ICP_SORTED = 16,     /* pcc_icp_align: 1 = the source cloud is brought into the target grid's cell order once and every pass
                                    reads and writes it front to back (default); 0 = caller's order, gathered / scattered in every pass.
                                    (The one option whose setting shows in a result: the 17 double sums of a pass are added up in the
                                    working order, so T and fitness can differ between 0 and 1 in their last bits; every form of the
                                    loop -- device, host, sharded -- agrees to the bit under either.) */
    PCC_OPT_OVERLAP_PREP = 17,   /* pcc_nn1 called directly after pcc_index_set_input / pcc_index_create (the reference's pattern,
                                    src/comparator.cpp:564-577: setInputCloud, then the query loop): 1 = the queries are packed and
                                    sorted on a second stream of the library WHILE the build's cell sort runs (default); 0 = one stream,
                                    one kernel after the other.  Same kernels, same results; only their placement in time differs.
                                    It acts from 2M queries on (below that it hides nothing); 2 = at every size (tests).  Only on the
                                    library's own stream: after pcc_index_set_stream the caller's stream is the one order there is. */
    PCC_OPT_GRID_AXES = 18,      /* which coordinate of the cloud the grid's three axes -- along a row of cells, over the rows of a
                                    layer, over the layers -- follow: -1 = chosen per index from the cloud's extents (default: second
                                    shortest, shortest, longest: the rows and layers next to a query's row are then as close to it in
                                    memory as the cloud allows); -2 = the same whatever GRID_AXES_MIN_POINTS says; 0 = x, y, z (rounds 1-5); 1 xzy, 2 yxz, 3 yzx, 4 zxy, 5 zyx.  Takes
                                    effect at the next pcc_index_set_input.  No result bit depends on it. */
    PCC_OPT_XCD_RUN = 19,        /* k = 1 search: consecutive workgroups (128 cell-sorted queries each) steered to the same XCD,
                                    i.e. the stretch of the grid one L2 works on at a time (default 256) */
    PCC_OPT_FUSE_PARAMS = 20,    /* bits: 1 = index build: the grid (cell edge, dimensions, axes) is derived by the last workgroup of the
                                    pack kernel to finish instead of a kernel of its own behind it; 2 = a pass of pcc_icp_align is solved
                                    by the last workgroup of its sums kernel.  Default 0: see DESIGN.md 4.3 (both were measured).
                                    Clouds of up to 8192 points take the form of bit 1 whatever this option says while
                                    PCC_OPT_HOST_PIPE is 1, host and device clouds alike: the kernel of its own runs for them only
                                    with PCC_OPT_HOST_PIPE = 0 */
    PCC_OPT_HOST_PIPE = 21,      /* PCC_MEM_HOST clouds and results of 8 MB and more in PAGEABLE memory: 1 = staged by the library
                                    through two pinned chunk buffers by a few host threads (PCC_HOST_THREADS, default half the
                                    cores, at most 8), the DMA of a chunk running while the next is gathered; only x, y, z cross
                                    the link when the stride is 24 bytes or more (default); 0 = one hipMemcpyAsync of the raw
                                    array.  Memory the caller has pinned (hipHostMalloc / hipHostRegister) is always copied directly.
                                    Also the SMALL host calls (clouds and results up to 1 MB): 1 = kernels read the cloud from, and write
                                    the results into, the handle's pinned buffers, and a k = 1 query call against up to 4096
                                    exhaustively searched points is one launch; 0 = copies and the separate launches.
                                    While it is 1 the index build of every cloud of up to 8192 points, in host or device memory,
                                    derives its grid inside the pack kernel (PCC_OPT_FUSE_PARAMS bit 1) */
    PCC_OPT_SCAN_CHAINED = 22,   /* exclusive scans inside the sorts: 1 = one launch, workgroups hand their totals forward through tagged
                                    64-bit atomics (default); 0 = two launches (totals, then apply) that wait for nothing -- for
                                    environments where workgroups are not dispatched in order (preemption, shared devices) */
    PCC_OPT_KNN_RUN = 23,        /* k-NN selection (k <= 512): a wave takes this many consecutive queries of the cell-sorted order in a
                                    row; every query after the first of its run starts from a bound -- its predecessor's K-th distance
                                    plus their separation (the K-th neighbour distance is 1-Lipschitz) -- and skips the cube sizing,
                                    the bucket histogram and the compaction (default 16; 1 = every query on its own, round 5) */
    PCC_OPT_RIFT_LAYOUT = 24,    /* pcc_rift_descriptors, the histogram kernel: 1 = 32 lanes per row -- every lane computes one row entry's
                                    vote, then every lane adds, in row order, the shares of the bin it owns (default); 0 = one lane per row
                                    (PCL's loop as it stands).  Same bits either way. */
    PCC_OPT_SIFT_LAYOUT = 25,    /* pcc_sift_keypoints, the scale-space kernel: 1 = a wave per point -- every lane computes one row entry's
                                    Gaussian weights for all scales, then one lane per scale adds its shares in row order (default);
                                    0 = one lane per (point, scale) walking its row prefix.  Same bits either way. */
    PCC_OPT_RIFT_BATCH_BRUTE_MAX = 26, /* pcc_rift_descriptors_batch: clouds of up to this many points get their radius rows from the
                                    exhaustive builder that serves the whole batch at once (n^2 distance tests per cloud); larger
                                    clouds take the single path inside the same call, one by one, on a work handle kept in ctx
                                    (default 8192; PCC_RIFT_BATCH_BRUTE_MAX in the environment of a new handle).  No result bit
                                    depends on it. */
    PCC_OPT_SIFT_BATCH_BRUTE_MAX = 27, /* pcc_sift_keypoints_batch: clouds of up to this many points go through the batch kernels (one
                                    segmented voxel grid, one exhaustive row build and one 25-NN pass per octave for the whole
                                    batch); larger clouds take the single path inside the same call, one by one, on a work handle
                                    kept in ctx (PCC_SIFT_BATCH_BRUTE_MAX in the environment of a new handle).  Default 8192, chosen from
                                    profiles/sift_batch_exp.txt: a cloud ALONE is cheaper on the work handle from about 3000 points
                                    (2.4 against 2.0 ms at 4096), but beside others the batch kernels win up to the 8000 points
                                    measured -- 60 clusters of 701 ... 8000 points take 17.6 ms at 8192 and 54.8 ms at 4096, where
                                    21 of them pay the single path's waits one after the other; above 8192 only the lone cloud
                                    was measured (10.2 against 3.4 ms at 16 384).  No result bit depends on it. */
    PCC_OPT_RGB_BATCH_BRUTE_MAX = 28,  /* pcc_region_growing_rgb_batch: clouds of up to this many points (and nr_region_neighbours <= 128) get
                                    their k-NN rows from the segmented exhaustive kernel that serves the whole batch at once (n^2
                                    distance tests per cloud) and grow in one pass over the concatenation; every other cloud takes
                                    the single path inside the same call, one by one, on a work handle kept in ctx
                                    (PCC_RGB_BATCH_BRUTE_MAX in the environment of a new handle).  Default 8192, chosen from
                                    profiles/rgb_batch_exp.txt: 60 clusters of 11 ... 8000 points take 11.3 / 5.7 / 4.08 / 4.06 ms
                                    at 2048 / 4096 / 8192 / 16 384 (13 / 3 / 0 / 0 of them on the work handle); a cloud ALONE takes
                                    0.41 / 0.73 / 1.06 / 1.22 ms through the batch kernels against 0.52 / 0.89 / 1.06 / 1.21 ms on
                                    the work handle at 2048 / 4096 / 8192 / 16 384 points: the batch kernels never lose up to 8192
                                    and tie above it, where only the lone cloud was measured.  No result bit depends on it. */
    PCC_OPT_FPFH_LAYOUT = 29,    /* pcc_fpfh_descriptors, the SPFH and the weighting kernel: 1 = a wave per row -- every lane evaluates one row
                                    entry's pair features and the votes are counted in integers; in the weighting every lane adds, in row
                                    order, the shares of the bin it owns while three more lanes carry the running sums (default);
                                    0 = one lane per row (PCL's loops as they stand).  Same bits either way. */
    PCC_OPT_FPFH_BATCH_BRUTE_MAX = 30, /* pcc_fpfh_descriptors_batch: clusters of up to this many points get their radius rows from the
                                    exhaustive builder that serves the whole batch at once (n^2 distance tests per cluster); larger
                                    clusters take pcc_index_set_input + pcc_fpfh_descriptors inside the same call, one by one, on a
                                    work handle kept in ctx (PCC_FPFH_BATCH_BRUTE_MAX in the environment of a new handle).  Default
                                    8192.  Measured (profiles/fpfh_batch_exp.txt, device memory): 60 clusters of 20 ... 5000
                                    points take 4.02 / 2.24 / 1.49 / 1.49 ms at 2048 / 4096 / 8192 / 16 384 (10 / 3 / 0 / 0 of them on
                                    the work handle); a cluster ALONE takes 0.24 / 0.30 / 0.46 / 0.85 ms through the batch kernels
                                    against 0.34 / 0.37 / 0.48 / 0.69 ms on the work handle at 2048 / 4096 / 8192 / 16 384 points: the
                                    crossover lies between 8192 and 16 384.  Only these four sizes were measured.  No result bit
                                    depends on it. */
    PCC_OPT_VFH_BATCH_BRUTE_MAX = 31   /* pcc_vfh_descriptors_batch: clusters of 2 .. this many points go through the batch kernels (the
                                    exhaustive row builder over the whole batch, one chain wave per cluster, votes and bins of all
                                    clusters in one launch each); larger clusters take pcc_index_set_input + pcc_vfh_descriptor
                                    inside the same call, one by one, on a work handle kept in ctx (PCC_VFH_BATCH_BRUTE_MAX in the
                                    environment of a new handle).  Default 8192, range 0 .. 2^30; 0 sends every cluster to the work
                                    handle.  Measured (profiles/vfh_batch_exp.txt, device memory): 60 clusters of 20 ... 5000 points take
                                    2.12 / 0.98 / 0.45 / 0.45 ms at 2048 / 4096 / 8192 / 16 384 (10 / 3 / 0 / 0 of them on the work
                                    handle); a cluster ALONE takes 0.19 / 0.23 / 0.33 / 0.63 ms through the batch kernels against
                                    0.23 / 0.26 / 0.30 / 0.41 ms on the work handle at those sizes.  Only these four were measured.
                                    No result bit depends on it. */
};
int pcc_index_set_option(pcc_index *index, int option, double value);
int pcc_index_get_option(pcc_index *index, int option, double *value);

/* ---- k = 1 nearest neighbour ------------------------------------------------
 * replaces: N calls of KdTreeFLANN::nearestKSearch(pt, 1, idx, d2)
 *           (src/comparator.cpp:571-577; ICP determineCorrespondences and
 *           getFitnessScore reached from :1096,:1099).
 * idx[nq], d2[nq] live in the same memory space as the queries. */
int pcc_nn1(pcc_index *index, const void *queries, size_t nq, size_t stride_bytes,
            int mem, int32_t *idx, float *d2);

/* ---- k nearest neighbours ---------------------------------------------------
 * replaces: nearestKSearch(pt, k, ...) with k = mean_k+1 = 51 inside
 *           StatisticalOutlierRemoval (src/comparator.cpp:1523-1541).
 * Row i holds min(k, n_valid) results ascending by (d2, idx), padded with
 * idx=-1, d2=+inf.  1 <= k <= PCC_KNN_MAX_K. */
int pcc_knn(pcc_index *index, const void *queries, size_t nq, size_t stride_bytes,
            int mem, int k, int32_t *idx, float *d2);

/* ---- radius search ------------------------------------------------------------
 * replaces: KdTreeFLANN::radiusSearch(pt, radius, idx, d2, max_nn = 0) as used
 *           by pcl::extractEuclideanClusters (src/segmentation.cpp:125-131).
 * r2 = float(radius*radius) evaluated in double; the test is strict d2 < r2.
 * Two-pass CSR: count, caller prefix-sums into offsets[nq+1], fill.  With
 * sorted != 0 each row is ascending by (d2, idx) (PCL's sorted results). */
int pcc_radius_count(pcc_index *index, const void *queries, size_t nq,
                     size_t stride_bytes, int mem, double radius, int32_t *counts);
int pcc_radius_fill(pcc_index *index, const void *queries, size_t nq,
                    size_t stride_bytes, int mem, double radius, int sorted,
                    const int64_t *offsets, int32_t *idx, float *d2);
/* the same with radiusSearch's max_nn: 0, or anything from the number of FINITE indexed points on (PCL's
 * total_nr_points_), means "all" and is the pair above; a max_nn below that but beyond PCC_KNN_MAX_K is refused by both calls
 * (PCC_ERR_UNSUPPORTED); otherwise the count is min(count, max_nn) and the row holds the max_nn NEAREST neighbours within the radius,
 * ascending by (d2, idx) whatever `sorted` says (FLANN's KNNRadiusResultSet).  Served by the k-NN kernels with k = max_nn
 * cut at the radius: the reference's own call sites pass 0 (src/segmentation.cpp:125-131), this is for completeness. */
int pcc_radius_count_max(pcc_index *index, const void *queries, size_t nq, size_t stride_bytes, int mem, double radius,
                         unsigned int max_nn, int32_t *counts);
int pcc_radius_fill_max(pcc_index *index, const void *queries, size_t nq, size_t stride_bytes, int mem, double radius,
                        int sorted, unsigned int max_nn, const int64_t *offsets, int32_t *idx, float *d2);

/* ---- Euclidean clustering -----------------------------------------------------
 * replaces: pcl::EuclideanClusterExtraction::extract with
 *           setClusterTolerance/MinClusterSize/MaxClusterSize
 *           (src/segmentation.cpp:125-131): connected components of the graph
 *           d2(i,j) < float(double(float(tol))^2) over the indexed cloud,
 *           filtered to [min_size, max_size], ordered by size descending
 *           (ties: lowest member index first).
 * labels[n_original] (memory space `mem`): cluster id or -1.  sizes[] (host,
 * nullable) receives up to max_sizes cluster sizes.  *n_clusters (host). */
int pcc_euclidean_clusters(pcc_index *index, double tolerance, uint32_t min_size,
                           uint32_t max_size, int mem, int32_t *labels,
                           int32_t *n_clusters, int32_t *sizes, int max_sizes);

/* ---- statistical outlier removal ------------------------------------------------
 * replaces: pcl::StatisticalOutlierRemoval::filter, setMeanK / setStddevMulThresh
 *           (src/comparator.cpp:1523-1527, 1537-1541).  Self-query of the
 *           indexed cloud with k = mean_k+1; mean_dist[i] = float(sum_{j=1..k-1}
 *           sqrt(d2_j) / mean_k) (double sum); threshold = mean + mult*stddev
 *           (double, n-1); inlier[i] = mean_dist[i] <= threshold.
 * mean_dist / inlier have n_original entries in memory space `mem` (either may
 * be NULL); *threshold and *kept are host scalars. */
int pcc_sor(pcc_index *index, int mean_k, double stddev_mult, int mem,
            float *mean_dist, uint8_t *inlier, double *threshold, size_t *kept);
/* PCL adds the mean distances up in index order in double (sum, and sq_sum of float squares).  The library takes both sums,
 * the threshold and the mask on the device whenever no addition of that chain rounds (every order then gives PCL's bits);
 * otherwise it falls back to the in-order loop on the host.  *on_device = 1 when the last pcc_sor stayed on the device. */
int pcc_index_sor_on_device(const pcc_index *index, int *on_device);

/* ---- ICP building blocks ----------------------------------------------------------
 * replaces: pcl::IterativeClosestPoint::align / getFitnessScore
 *           (src/comparator.cpp:1091-1099).
 * pcc_icp_step: NN of every source point against the target index plus the
 *   double-precision sums Umeyama needs, fused in one pass.
 *   sums[0..2]=sum p, [3..5]=sum q, [6..14]=sum q p^T (row-major, q row, p col),
 *   [15]=sum d2, [16]=count.  idx/d2 may be NULL.  sums is a HOST array.
 * pcc_rigid_from_sums: the rigid transform (rotation + translation, no scaling; Horn's quaternion form of
 *   the Umeyama/Kabsch solution, solved in double, returned as a row-major float 4x4) those sums determine.
 *   Pure host arithmetic, needs no handle: a caller that shards the SOURCE cloud over several GPUs adds up the
 *   sums of all shards (one all-reduce of 17 doubles per iteration) and gets the same transform on every rank.
 *   Returns PCC_ERR_INVALID when fewer than 3 correspondences contributed.  The sums are about the ORIGIN: for a small
 *   cloud at large coordinates (geo-referenced scans) sum q p^T - n pm qm^T cancels -- shift both clouds by a common
 *   offset first.  pcc_icp_align does the equivalent itself (it sums about a point of the source cloud).
 * pcc_transform: dst = T * src with PCL's transformPointCloud rounding
 *   ((m0*x + m1*y) + m2*z) + m3; T row-major 4x4 (host); dst may alias src.
 * pcc_icp_align: the whole loop on the device (source stays resident):
 *   max_iter iterations (early exit on |mse-prev| < 1e-12 unless fixed != 0).  In both modes the loop lives on the
 *   device: every pass is search -> sums -> one-workgroup solve (transform, running product, convergence criteria) ->
 *   transform, enqueued in chunks without a host round trip (5 passes per host look with the criteria active, up to 32
 *   with a fixed count); the sums are taken about the first valid source point.  PCC_OPT_ICP_DEVICE_LOOP = 0 selects the
 *   host-driven loop (same bits).
 *   final transform T (host, row-major), *fitness = mean squared NN distance of
 *   the finally transformed source, *converged as PCL's hasConverged(). */
int pcc_rigid_from_sums(const double sums[17], float T[16]);
int pcc_icp_step(pcc_index *target, const void *src, size_t n, size_t stride_bytes,
                 int mem, int32_t *idx, float *d2, double sums[17]);
/* The same two with the sums taken about `center` (sum (p - c), sum (q - c), sum (q - c)(p - c)^T; NULL = origin):
 * what a multi-GPU ICP loop over a geo-referenced cloud should use -- every rank MUST pass the identical center bits
 * (any point of the cloud, e.g. its first, broadcast once), adds up the sums of all ranks and solves with that center. */
int pcc_rigid_from_sums_about(const double sums[17], const double center[3], float T[16]);
int pcc_icp_step_about(pcc_index *target, const void *src, size_t n, size_t stride_bytes, int mem,
                       const double center[3], int32_t *idx, float *d2, double sums[17]);
int pcc_transform(pcc_index *ctx, const float T[16], const void *src, size_t n,
                  size_t src_stride, void *dst, size_t dst_stride, int mem);
int pcc_icp_align(pcc_index *target, const void *src, size_t n, size_t stride_bytes,
                  int mem, int max_iter, int fixed, float T[16], double *fitness,
                  int *iterations, int *converged);

/* ---- descriptor correspondence ------------------------------------------------------
 * replaces: matchRIFTFeaturesKnn (src/comparator.cpp:560-588): index built on
 *   descriptors1, one k=1 query per element of descriptors2, a match is kept
 *   when d2 < threshold (0.05f in the reference).  out[0] = 0 is the dummy
 *   element the reference's vector starts with (:568); *out_size = 1 + matches.
 *   out is a HOST array of at least n2+1 ints. */
int pcc_match_knn(pcc_index *index_des1, const void *des2, size_t n2,
                  size_t stride_bytes, int mem, float threshold, int32_t *out,
                  int32_t *out_size);
/* The same for EVERY cluster pair of a comparison at once -- replaces the calls of the cluster-matching loop
 *   (src/comparator.cpp:1296-1365, call at :1322): per cluster of cloud 1 the three nearest clusters of cloud 2 behind
 *   two size gates, none depending on an earlier result.  One upload, one search launch, one wait for all pairs (one
 *   more of each when PCC_TIES_FLANN meets a tied query), whatever n_pairs is.
 *   ctx: any index handle; it supplies device, stream, scratch, the tie order (pcc_index_set_tie_order) and
 *     PCC_OPT_FLANN_SPLIT, as for pcc_voxel_grid.  The cloud it indexes is neither read nor changed.  pcc_index_stats
 *     afterwards reports the batch's totals in [1] (queries), [5] (tied) and [6] (indices the FLANN walk changed).
 *   Pair p searches the n2[p] records of des2[p] against the n1[p] records of des1[p]; per pair the result is what
 *     pcc_index_create(des1[p], ..., PCC_ENGINE_AUTO) + pcc_match_knn(des2[p]) returns under the same tie order, bit
 *     for bit.  Its row is out[out_offsets[p] .. out_offsets[p + 1]): the dummy 0 of :568, then one index into des1[p]
 *     per query with d2 < threshold, in query order.  A pair with n1 == 0, n2 == 0 or no finite record in des1[p]
 *     yields the dummy alone (the single path answers PCC_ERR_EMPTY there); n_pairs == 0 touches no device.
 *   out: HOST array of at least sum(n2) + n_pairs ints; out_offsets: n_pairs + 1 entries.  mem must be PCC_MEM_HOST
 *     (PCC_MEM_DEVICE: PCC_ERR_UNSUPPORTED).  The arrays, the stride and the totals (below 2^31) are checked before
 *     the handle is looked at. */
int pcc_match_knn_batch(pcc_index *ctx, size_t n_pairs,
                        const void *const *des1, const size_t *n1,
                        const void *const *des2, const size_t *n2,
                        size_t stride_bytes, int mem, float threshold,
                        int32_t *out, size_t *out_offsets);
/* The same on the first `dim` floats of every record, dim = 1 ... 32 -- matching on the descriptor itself.  The reference's
 *   PCL searches three bins of a RIFT32 (pcl::Histogram<32> has no point representation of its own; recalled, SURVEY.md
 *   3.2 / 9.1), which is what dim = 3 and pcc_match_knn_batch do; dim = 32 matches on the whole histogram (the calls of
 *   src/comparator.cpp:560-588 made from :1296-1365, as above).  N-dimensional search exists for descriptor matching
 *   only: pcc_index_create and pcc_index_set_input keep refusing dim != 3, and no index is built over N-D records.
 *   Everything is as for pcc_match_knn_batch (rows, the dummy 0, d2 < threshold strict, out_offsets, ctx as context only,
 *   host arrays only) except:
 *   distance: FLANN's L2_Simple over dim terms in float32, every operation rounded on its own, in index order:
 *     d = d0 * d0; d = d + d1 * d1; ... d = d + d(dim-1) * d(dim-1).  The order is part of the result.
 *   validity: a record is valid when its first dim floats are all finite (PCL's isValid over nr_dimensions); floats at dim
 *     and beyond are never read.  An invalid reference takes part in no search, an invalid query finds nothing, a distance
 *     that overflowed to +inf is no neighbour.
 *   stride_bytes: a multiple of 4 and >= 4 * dim; of the last record of an array only 4 * dim bytes are read.
 *   out_d2 (nullable): parallel to out -- the squared distance of every kept match, 0.0f at each row's dummy.
 *   dim == 3: the search of pcc_match_knn_batch itself, bit for bit, PCC_TIES_FLANN and pcc_index_stats [1]/[5]/[6]
 *     included.
 *   dim != 3, exact ties: among references at exactly the same distance the LOWEST INDEX wins, whatever tie order the
 *     handle has -- FLANN's tree is built here in three dimensions only, so an N-dimensional FLANN visit order could not
 *     be checked against anything.  pcc_index_stats [5] still reports the number of tied queries; [6] is 0.
 *   Refused before the handle is looked at, in this order: dim outside 1 ... 32 (PCC_ERR_UNSUPPORTED), a bad stride
 *     (PCC_ERR_INVALID), then everything pcc_match_knn_batch refuses, a null handle last.  A refused call writes nothing. */
int pcc_match_knn_batch_dims(pcc_index *ctx, size_t n_pairs,
                             const void *const *des1, const size_t *n1,
                             const void *const *des2, const size_t *n2,
                             size_t stride_bytes, int dim, int mem, float threshold,
                             int32_t *out, float *out_d2 /* nullable */, size_t *out_offsets);
/* The same on the 33 bins of a pcl::FPFHSignature33, from host or from device memory -- replaces matchFPFH
 *   (src/comparator.cpp:877-910): a FLANN index on descriptors1, one k = 1 query per element of descriptors2, a match kept when
 *   d2 < 0.25f (:901).  pcc_fpfh_descriptors produces the descriptors, this call consumes them.  Everything is as for
 *   pcc_match_knn_batch_dims at dim != 3 (rows, the dummy 0 -- here :889 --, d2 < threshold strict, out_offsets, ctx as context
 *   only: it supplies device, stream and scratch, its cloud and kept rows are neither read nor changed) except:
 *   record: the first 33 floats of each element (pcl::FPFHSignature33::histogram).  stride_bytes is a multiple of 4 and
 *     >= 132; of the last record of an array only 132 bytes are read, floats at 33 and beyond never.
 *   validity: a record is valid when all 33 floats are finite.  An invalid reference takes part in no search, an invalid query
 *     finds nothing, a distance that overflowed to +inf is no neighbour.  (The reference tests histogram[0] of a query alone,
 *     :895, and leaves the rest to an assert inside PCL; pcc::matchFPFH prints its "Found NaN in FPFH descriptors" line, this
 *     call prints nothing.)
 *   distance: FLANN's L2_Simple over 33 terms in float32, every operation rounded on its own, in index order:
 *     d = d0 * d0; d = d + d1 * d1; ... d = d + d32 * d32.  The order is part of the result.
 *   out_d2 (nullable): parallel to out -- the squared distance of every kept match, 0.0f at each row's dummy.
 *   exact ties: among references at exactly the same distance the LOWEST INDEX wins, whatever tie order the handle has --
 *     FLANN's tree is built here in three dimensions only, so an N-dimensional FLANN visit order could not be checked against
 *     anything.  pcc_index_stats afterwards: [1] the number of queries, [5] the number of tied queries, [6] is 0.
 *   mem: PCC_MEM_HOST, or PCC_MEM_DEVICE: des1[p] and des2[p] are then device pointers (4-byte aligned, PCC_ERR_INVALID
 *     otherwise) -- the [n][33] output of pcc_fpfh_descriptors(mem = PCC_MEM_DEVICE), stride 132, goes in as it is.  The arrays
 *     of pointers and counts, out, out_d2 and out_offsets are HOST arrays in either memory space.
 *   A pair with n1 == 0, n2 == 0 or no valid record in des1[p] yields the dummy alone; n_pairs == 0 touches no device.  One
 *     upload, one pack launch (device memory only), one search launch, one read-back and one wait, whatever n_pairs is.
 *   Refused before the handle is looked at, in this order: a bad memory space (PCC_ERR_INVALID), a bad stride
 *     (PCC_ERR_INVALID), then everything pcc_match_knn_batch refuses (null arrays, totals of 2^31 records and more) and a
 *     misaligned device pointer, a null handle last.  A refused call writes nothing. */
int pcc_match_fpfh_batch(pcc_index *ctx, size_t n_pairs,
                         const void *const *des1, const size_t *n1,
                         const void *const *des2, const size_t *n2,
                         size_t stride_bytes, int mem, float threshold,
                         int32_t *out, float *out_d2 /* nullable */, size_t *out_offsets);

/* ---- voxel-grid down-sampling -----------------------------------------------------------------------
 * replaces: pcl::VoxelGrid<PointXYZRGB> with setLeafSize(l, l, l) + filter, the first step of both
 *   segmentation paths (src/segmentation.cpp:69-74 and :224-229, l = 0.025f).  Every occupied voxel
 *   of the world-aligned leaf lattice (index floor(p/leaf) - min_b, as PCL computes it) is replaced
 *   by the centroid of its points; with has_rgb != 0 the packed rgb word at byte offset 16 is
 *   averaged per channel and truncated, as PCL does.  Output order: ascending voxel index.
 *   Non-finite points are ignored.  `ctx` is any index handle (supplies device, stream, scratch).
 * out: caller-allocated, capacity n elements of out_stride bytes (x, y, z at 0 [, rgb at 16]);
 * *out_n (host) = number of voxels written.  Centroid coordinates are accumulated in double and
 * rounded once (PCL: float sums in sort order), i.e. equal to PCL's within float rounding.
 * What is written: rows 0 .. *out_n - 1, and of each x, y, z at 0, 1.0f at 12 when out_stride >= 16, the
 *   colour word at 16 with has_rgb (its top byte 0).  Rows from *out_n on keep the caller's bytes.  The
 *   other bytes of a written row (from 16 on without colour, from 20 on with it) keep the caller's bytes
 *   when out is device memory and are ZERO when out is host memory (whole rows of a zeroed staging buffer
 *   are copied).  A cloud without a finite point: PCC_OK, *out_n = 0, nothing written.
 * Colour: channel sums are integers, exact up to 2^32 / 255 points in a voxel, divided in float as PCL
 *   does.  PCL sums the channels in float: up to 65 793 points in a voxel (2^24 / 255) both are exact and
 *   equal; beyond that PCL's own word depends on the order its sort left the points in.
 * Refused with PCC_ERR_UNSUPPORTED ("leaf size %g too small for this cloud"), *out_n = 0 and out untouched:
 *   more than 2^26 voxels in the lattice of the finite bounding box, or a bound of that box whose voxel
 *   coordinate floor(bound * (1 / leaf)) is not finite or not below 2^31 in magnitude -- PCL converts it to
 *   int, which is undefined there (a far cloud with a tiny leaf; a subnormal leaf, whose inverse is
 *   infinite).  Decided on the host in floating point before anything is sorted.  The segmentation, ground
 *   and SIFT entry points, which start with this step, refuse alike (pcc_sift_keypoints_batch names the cloud). */
int pcc_voxel_grid(pcc_index *ctx, const void *pts, size_t n, size_t stride_bytes, int mem,
                   float leaf, int has_rgb, void *out, size_t out_stride, size_t *out_n);

/* ---- RANSAC plane segmentation ---------------------------------------------------------------------
 * replaces: pcl::SACSegmentation<PointXYZRGB> with setModelType(SACMODEL_PLANE), setMethodType(SAC_RANSAC),
 *   setOptimizeCoefficients(true), setMaxIterations(100), setDistanceThreshold(0.02), segment(inliers,
 *   coefficients) -- the plane-removal loop in front of the Euclidean clustering
 *   (src/segmentation.cpp:79-99; the ExtractIndices steps :103-116 are index bookkeeping on the host).
 *   PCL's RANSAC is deterministic (fixed-seed mt19937, see sac.hip): the same 3-point samples are drawn,
 *   every candidate plane's support |a x + b y + c z + d| < threshold is counted on the GPU (32 candidates
 *   per pass over the cloud), PCL's best-model / adaptive iteration-count logic runs on the counts, and the
 *   inliers are selected on the GPU in ascending index order.  optimize != 0 adds PCL's least-squares
 *   refit over the inliers and a second selection with the refined plane.
 * inliers[] (memory space `mem`, capacity n); *n_inliers, coefficients[4] (a, b, c, d) and *iterations
 *   (RANSAC iterations PCL would have run; may be NULL) are host values.  n_inliers == 0: no model
 *   (PCL: "Could not estimate a planar model").  `ctx` is any index handle. */
int pcc_sac_plane(pcc_index *ctx, const void *pts, size_t n, size_t stride_bytes, int mem,
                  int max_iterations, double distance_threshold, double probability, int optimize,
                  int32_t *inliers, size_t *n_inliers, float coefficients[4], int *iterations);

/* ---- the plane-removal loop around it, the cloud staged once -------------------------------------------
 * replaces: the whole loop of src/segmentation.cpp:79-117 -- "segment the largest plane, extract its inliers, keep the
 *   rest" until at most stop_fraction (0.3 there) of the input cloud remains.  The result is that of
 *
 *     cur = the n input points; p = 0
 *     while ((double)|cur| > stop_fraction * (double)n) {                      (:91, the comparison in double)
 *         (inliers, coeff, its) = pcc_sac_plane(cur, max_iterations, distance_threshold, probability, optimize)
 *         if (|inliers| == 0) { *ended_without_model = 1; break; }             (:95-100)
 *         plane p = (coeff, |inliers|, its); cur = cur without the inliers, order kept (ExtractIndices, negative); ++p
 *     }
 *
 *   bit for bit: every turn is a fresh segment() (generator seeded again, sampling over the current cloud).  The cloud is
 *   uploaded and packed once; a turn compacts it on the device and brings only what pcc_sac_plane brings to the host.
 *   Non-finite points are never inliers: they stay in the cloud to the end, count in its size and can be drawn as samples.
 * out_coefficients[max_planes][4], out_plane_sizes[max_planes], out_iterations[max_planes] (may be NULL), *n_planes,
 *   *ended_without_model (may be NULL) and *n_remaining are HOST values.
 * out_plane_of_point[n] (space `mem`, may be NULL): the turn that removed input point i, -1 if it remains.
 * out_remaining_index[n] (space `mem`, may be NULL): the first *n_remaining entries are the input indices of the remaining
 *   points, ascending.
 * out_points (space `mem`, may be NULL; capacity n records of out_stride_bytes, not overlapping pts): for the j-th remaining
 *   point the first record_bytes of its input record, verbatim, at out_points + j * out_stride_bytes -- what
 *   pcc_index_set_input(..., *n_remaining, out_stride_bytes, mem) takes next.  record_bytes is a multiple of 4 with
 *   12 <= record_bytes <= min(stride_bytes, out_stride_bytes), out_stride_bytes a multiple of 4; record_bytes must be
 *   readable in every input record (32 for pcl::PointXYZRGB carries the colour word).
 * max_planes: when the loop condition still holds after max_planes planes the call returns PCC_ERR_OVERFLOW with
 *   *n_planes = max_planes, those planes in the host tables and *n_remaining = the points then left; the arrays in space
 *   `mem` are unspecified.  0 is accepted when no turn runs (stop_fraction >= 1, n == 0).
 * Refused before any device is touched, nothing written: what pcc_sac_plane refuses (same messages); stop_fraction negative
 *   or not finite; a NULL n_planes or n_remaining; NULL out_coefficients or out_plane_sizes with max_planes > 0; a bad
 *   record_bytes or out_stride_bytes with out_points given; a null handle last.
 * `ctx` is any index handle (device, stream, scratch), as for pcc_sac_plane.  Afterwards pcc_index_stats reports in [0] the
 *   planes removed and in [1] the turns that took a host copy of the current cloud (a degenerate sample, see sac.hip). */
int pcc_plane_removal(pcc_index *ctx, const void *pts, size_t n, size_t stride_bytes, int mem,
                      double stop_fraction, int max_iterations, double distance_threshold, double probability, int optimize,
                      size_t max_planes, float *out_coefficients, uint32_t *out_plane_sizes, int *out_iterations,
                      size_t *n_planes, int *ended_without_model, int32_t *out_plane_of_point,
                      int32_t *out_remaining_index, size_t *n_remaining, void *out_points, size_t out_stride_bytes,
                      size_t record_bytes);

/* ---- normals + region growing (default segmentation path) --------------------------------------
 * pcc_normals replaces: pcl::NormalEstimation<PointXYZRGB, pcl::Normal> with setSearchMethod(tree),
 *   setKSearch(k), compute (src/segmentation.cpp:232-241, k = 50; viewpoint left at (0,0,0)).
 *   Per point of the index: its k nearest neighbours (itself first), PCL's single-pass float
 *   mean/covariance in neighbour order, the smallest eigenpair in closed form (pcl::eigen33),
 *   curvature = |lambda_0 / trace|, normal flipped towards the viewpoint.
 * out[n][4] floats (memory space `mem`): nx, ny, nz, curvature.  NaN for non-finite points and when
 *   fewer than 3 neighbours exist.  viewpoint may be NULL (= origin).
 * pcc_region_growing replaces: pcl::RegionGrowing<PointXYZRGB, pcl::Normal> with setSearchMethod,
 *   setNumberOfNeighbours(k), setSmoothnessThreshold, setCurvatureThreshold, setMin/MaxClusterSize,
 *   setInputCloud / setInputNormals, extract (src/segmentation.cpp:259-271: 50, 1000000, k = 100,
 *   3/180*pi, 1.0).  The k-neighbour rows of every point are searched on the GPU in one batch
 *   (PCL: findPointNeighbours, one nearestKSearch per point).  The result is PCL's: seeds by
 *   ascending curvature, breadth first through the rows while |n_current . n_neighbour| >=
 *   cos(smoothness), a neighbour continues the walk when its curvature is <= curvature_threshold.
 *   The regions are computed on the GPU in an equivalent order-free form: the label of a point is the
 *   lowest-ranked (curvature, index) point that reaches it along valid edges, where a point above the
 *   curvature threshold passes labels on only if it is a seed itself (region.hip).
 * normals[n][4] as pcc_normals writes them (memory space `mem`); labels[n] (memory space `mem`):
 *   index of the kept cluster, in PCL's output order (creation order), or -1;
 *   *n_clusters (host) = clusters.size().  Equal curvatures are taken in index order (PCL:
 *   std::sort, unspecified). */
int pcc_normals(pcc_index *index, int k, const float viewpoint[3], int mem, float *out);
/* the same with setRadiusSearch(radius) instead of setKSearch (the normals of the RIFT pipeline,
 * src/comparator.cpp:628-635, radius 0.03): the neighbourhood is the sorted radiusSearch result
 * (d2 < float(radius^2), ascending (d2, index)); NaN where it holds fewer than 3 points. */
int pcc_normals_radius(pcc_index *index, double radius, const float viewpoint[3], int mem, float *out);

/* ---- labels -> one cloud per cluster -----------------------------------------------------------------------
 * replaces: the loop both segmentation paths of the reference end with (src/segmentation.cpp:133-152 and :290-318): for every
 *   cluster, in order, a new cloud of cloud[j] for every index j of the cluster.  With the clusters given as labels[n]
 *   (pcc_region_growing, pcc_euclidean_clusters): for c = 0 .. n_clusters - 1, in that order, the points i with
 *   labels[i] == c in ASCENDING i -- what `for i: clusters[labels[i]].push_back(i)` gives, the order of
 *   np.argsort(labels, kind="stable") without the -1 entries, the same on every run (a stable radix partition on the
 *   device, segment.hip).
 * out_offsets[n_clusters + 1] (HOST): cluster c is the slice out_offsets[c] .. out_offsets[c + 1] of
 *   out_index[n] (space `mem`, may be NULL): the indices i (entries from out_offsets[n_clusters] on are unspecified), and of
 *   out_records (space `mem`, may be NULL; capacity n records of out_stride_bytes, not overlapping records): the first
 *   record_bytes of record i, verbatim, at slot j * out_stride_bytes; the rest of a slot is not touched.
 * A label of -1 is left out; a cluster no point carries is an empty slice; a label outside [-1, n_clusters) gives
 *   PCC_ERR_INVALID -- found on the device (no table is indexed by such a label) and reported after the call's one wait;
 *   nothing is promised about the outputs then.  n == 0 or n_clusters == 0: PCC_OK, every offset 0.
 * records (read only with out_records), labels, out_records and out_index are in space `mem`.  record_bytes is a multiple of 4
 *   with 12 <= record_bytes <= min(stride_bytes, out_stride_bytes), both strides multiples of 4 (pcc_plane_removal's rules).
 * Refused before any device is touched, nothing written: a bad memory space, 2^31 points or more (PCC_ERR_UNSUPPORTED), a
 *   negative n_clusters, NULL labels with n > 0, a NULL out_offsets, with out_records a NULL records or a bad stride or
 *   record_bytes; a null handle last.  `ctx` is any index handle (device, stream, scratch), as for pcc_plane_removal. */
int pcc_extract_clusters(pcc_index *ctx, const void *records, size_t n, size_t stride_bytes, size_t record_bytes,
                         const int32_t *labels, int32_t n_clusters, int mem,
                         void *out_records, size_t out_stride_bytes, int32_t *out_index, size_t *out_offsets);

/* ---- the default segmentation path in one call -----------------------------------------------------------
 * replaces: region_growing_segmentation (src/segmentation.cpp:218-327): VoxelGrid leaf (0.025, :224-229) -> NormalEstimation
 *   K = normal_k (50, :232-241) -> RegionGrowing K = k (100, :259-271) -> one cloud per cluster (:290-318).  Every output is
 *   bit for bit what this sequence of calls gives, and where a step of it fails the call returns that step's status:
 *
 *     pcc_voxel_grid(ctx, pts, n, stride_bytes, mem, leaf, has_rgb, F, out_stride_bytes, &nv)   -> out_points, *n_filtered
 *     H = pcc_index_create(F, nv, out_stride_bytes, ...)            (a fresh handle, default tie order)
 *     pcc_normals(H, normal_k, NULL, ...)                                                         -> out_normals[0 .. nv)
 *     pcc_region_growing(H, normals, k, smoothness, curvature_threshold, min_size, max_size, ...) -> out_labels[0 .. nv), *n_clusters
 *     pcc_extract_clusters(ctx, F, nv, out_stride_bytes, out_stride_bytes, labels, *n_clusters, ...) -> out_offsets, out_cluster_*
 *
 *   but the filtered cloud, its index, its k-NN rows (searched once with max(normal_k, k) neighbours), its normals and its
 *   labels stay on the device from the raw cloud to the cluster clouds.  Only scalars cross to the host inside the call: the
 *   voxel grid's block statistics and count, region growing's words per sweep and its seed list, the offsets.
 * out_points (space `mem`, capacity n records of out_stride_bytes): the filtered cloud, *n_filtered (HOST) records; the bytes
 *   of a record pcc_voxel_grid does not write are zero in both memory spaces.  out_normals[n][4], out_labels[n] (space `mem`,
 *   may be NULL): their first *n_filtered rows.  *n_clusters (HOST).  out_offsets[max_clusters + 1] (HOST): its first
 *   *n_clusters + 1 entries, as pcc_extract_clusters writes them over the filtered cloud.  out_cluster_points (space `mem`,
 *   may be NULL, capacity n records of out_stride_bytes): whole filtered records, cluster by cluster.  out_cluster_index[n]
 *   (space `mem`, may be NULL): their indices in the filtered cloud.
 * No finite point (or n == 0): PCC_OK, *n_filtered = *n_clusters = 0, out_offsets[0] = 0.
 * *n_clusters > max_clusters: PCC_ERR_OVERFLOW with *n_clusters set and *n_filtered, out_points, out_normals, out_labels
 *   valid; the cluster outputs are unspecified (as max_planes of pcc_plane_removal).
 * Refused before any device is touched, nothing written: what pcc_voxel_grid refuses (same messages); a NULL n_filtered,
 *   n_clusters or out_offsets; out_cluster_points or out_cluster_index with max_clusters == 0; a smoothness or curvature
 *   threshold that is not finite; normal_k or k outside [1, PCC_KNN_MAX_K] (PCC_ERR_UNSUPPORTED); a null handle last.
 * `ctx` is any index handle: the cloud it indexes, its tie order and its kept rows are neither read nor changed.  The filtered
 *   cloud is indexed on a work handle kept in `ctx` (under ctx's options, PCC_OPT_KNN_CACHE_K = max(normal_k, k)) and freed
 *   with it.  Afterwards pcc_index_stats reports in [0] the filtered points, [1] the clusters, [2] the clustered points and
 *   [7] region growing's sweeps. */
int pcc_region_growing_segmentation(pcc_index *ctx, const void *pts, size_t n, size_t stride_bytes, int mem,
                                    float leaf, int has_rgb, int normal_k, int k, float smoothness, float curvature_threshold,
                                    uint32_t min_size, uint32_t max_size,
                                    void *out_points, size_t out_stride_bytes, size_t *n_filtered,
                                    float *out_normals, int32_t *out_labels,
                                    size_t max_clusters, int32_t *n_clusters, size_t *out_offsets,
                                    void *out_cluster_points, int32_t *out_cluster_index);
/* ---- the -e segmentation path in one call ------------------------------------------------------------------
 * replaces: euclidean_cluster_segmentation (src/segmentation.cpp:64-156): VoxelGrid leaf (0.025, :69-74) -> the plane-removal
 *   loop (:79-117) -> EuclideanClusterExtraction (0.05, 100, 250000, :122-131) -> one cloud per cluster (:133-152).  Every output
 *   is bit for bit what this sequence of calls gives, and where a step of it fails the call returns that step's status:
 *
 *     pcc_voxel_grid(ctx, pts, n, stride_bytes, mem, leaf, has_rgb, F, out_stride_bytes, &nv)      -> *n_filtered = nv
 *     pcc_plane_removal(ctx, F, nv, out_stride_bytes, mem, stop_fraction, max_iterations, distance_threshold, probability,
 *                       optimize, max_planes, ..., R, out_stride_bytes, record_bytes = out_stride_bytes)
 *                                        -> the plane tables, *n_planes, *ended_without_model, *n_remaining = nr, out_points = R
 *     H = pcc_index_create(R, nr, out_stride_bytes, ...)            (a fresh handle, default tie order)
 *     pcc_euclidean_clusters(H, tolerance, min_size, max_size, ...)                                 -> out_labels[0 .. nr), *n_clusters
 *     pcc_extract_clusters(ctx, R, nr, out_stride_bytes, out_stride_bytes, labels, *n_clusters, ...) -> out_offsets, out_cluster_*
 *
 *   but the filtered cloud, the cloud that remains, its index and its labels stay on the device from the raw cloud to the cluster
 *   clouds.  Only scalars cross to the host inside the call: the voxel grid's block statistics and count, what the plane fit
 *   brings per turn (pcc_plane_removal), the cluster count, the offsets.  Up to 2048 clusters are numbered on the device; with
 *   more, the cluster list takes pcc_euclidean_clusters' host sort.
 * out_points (space `mem`, capacity n records of out_stride_bytes): the cloud that remains after the planes (the reference's
 *   cloud_filtered at :119), *n_remaining (HOST) whole voxel-grid records; the bytes of a record pcc_voxel_grid does not write are
 *   zero in both memory spaces.  *n_filtered (HOST): the points after the voxel grid.  out_labels[n] (space `mem`, may be NULL):
 *   its first *n_remaining entries.  out_offsets[max_clusters + 1] (HOST), out_cluster_points (space `mem`, may be NULL, capacity n
 *   records of out_stride_bytes), out_cluster_index[n] (space `mem`, may be NULL): as in pcc_region_growing_segmentation, over
 *   the remaining cloud.  out_coefficients, out_plane_sizes, out_iterations, *n_planes, *ended_without_model, max_planes: as in
 *   pcc_plane_removal; its PCC_ERR_OVERFLOW leaves *n_filtered valid and the arrays in space `mem` unspecified.
 * *n_clusters > max_clusters: PCC_ERR_OVERFLOW with *n_clusters, *n_filtered, *n_remaining, the plane outputs, out_points and
 *   out_labels valid; the cluster outputs are unspecified.
 * No finite point (or n == 0): PCC_OK, every count 0, out_offsets[0] = 0.  Nothing remaining after the planes: PCC_OK, 0 clusters.
 * Refused before any device is touched, nothing written, in this order: what pcc_voxel_grid refuses (same messages); what
 *   pcc_plane_removal refuses about its own parameters and tables (same messages); a tolerance that is negative or NaN; a NULL
 *   n_filtered, n_remaining, n_clusters or out_offsets; out_cluster_points or out_cluster_index with max_clusters == 0; a null
 *   handle last.
 * `ctx` is any index handle: the cloud it indexes, its tie order and its kept rows are neither read nor changed.  The remaining
 *   cloud is indexed on the work handle pcc_region_growing_segmentation keeps in `ctx` (under ctx's options), freed with it.
 *   Afterwards pcc_index_stats reports in [0] the filtered points, [1] the clusters, [2] the clustered points, [3] the planes
 *   removed and [4] the turns that took a host copy of the current cloud. */
int pcc_euclidean_cluster_segmentation(pcc_index *ctx, const void *pts, size_t n, size_t stride_bytes, int mem,
                                       float leaf, int has_rgb,
                                       double stop_fraction, int max_iterations, double distance_threshold, double probability,
                                       int optimize, size_t max_planes, float *out_coefficients, uint32_t *out_plane_sizes,
                                       int *out_iterations, size_t *n_planes, int *ended_without_model,
                                       double tolerance, uint32_t min_size, uint32_t max_size,
                                       void *out_points, size_t out_stride_bytes, size_t *n_filtered, size_t *n_remaining,
                                       int32_t *out_labels,
                                       size_t max_clusters, int32_t *n_clusters, size_t *out_offsets,
                                       void *out_cluster_points, int32_t *out_cluster_index);
/* ---- the morphological ground filter ------------------------------------------------------------------
 * replaces: ground_segmentation (src/segmentation.cpp:330-387): pcl::VoxelGrid<PointXYZ> (leaf 0.01) ->
 *   pcl::ProgressiveMorphologicalFilter (max window 20, slope 1, initial distance 0.5, max distance 3; PCL's defaults cell
 *   size 1, base 2, exponential) -> pcl::ExtractIndices, positive and negative.  PCL 1.7's filter and its
 *   applyMorphologicalOperator are restated from the published source as recalled; parity with PCL itself is unpinned.
 * All arithmetic is float32, every operation rounded on its own, unless it says double. */
enum pcc_morph_op { PCC_MORPH_DILATE = 0, PCC_MORPH_ERODE = 1, PCC_MORPH_OPEN = 2, PCC_MORPH_CLOSE = 3 };
#define PCC_PMF_MAX_WINDOWS 64
/* The window table of ProgressiveMorphologicalFilter::extract (src/segmentation.cpp:330-387 sets its parameters at :352-358).
 * Host arithmetic, no handle:
 *     it = 0; w = 0.0f
 *     while (w < (float)max_window_size):
 *         w = exponential ? float((double)cell_size * (2.0 * pow((double)base, it) + 1.0))
 *                         : float((double)cell_size * (2.0 * (it + 1) * (double)base + 1.0))
 *         h = it == 0 ? initial_distance : ((slope * (w - windows[it - 1])) * cell_size) + initial_distance
 *         if (h > max_distance) h = max_distance
 *         windows[it] = w; thresholds[it] = h; ++it
 *   (the last window may exceed max_window_size: 3, 5, 9, 17, 33 for the reference's parameters).
 * out_windows, out_thresholds: `capacity` floats each; *n_windows: the table's length.  A longer table than `capacity` or than
 *   PCC_PMF_MAX_WINDOWS: PCC_ERR_OVERFLOW, *n_windows set (PCC_PMF_MAX_WINDOWS + 1 stands for any greater length), the first
 *   min(capacity, PCC_PMF_MAX_WINDOWS) entries written.
 * PCC_ERR_INVALID: a null output; a slope, distance, cell size or base that is not finite; cell_size <= 0; base <= 1 with
 *   exponential; base <= 0 without (PCL loops forever on the last three). */
int pcc_pmf_windows(int max_window_size, float slope, float initial_distance, float max_distance, float cell_size, float base,
                    int exponential, size_t capacity, float *out_windows, float *out_thresholds, size_t *n_windows);
/* pcl::applyMorphologicalOperator (the operator ground_segmentation's filter runs twice per window, src/segmentation.cpp:330-387)
 * over all n points, with window `window`:
 *   half = window / 2.0f; the box of point i is lo_x = x_i - half, hi_x = x_i + half and the same in y; point j lies in B(i) when
 *   lo_x <= x_j && x_j <= hi_x && lo_y <= y_j && y_j <= hi_y -- both ends inclusive, the edges computed exactly as written; z
 *   takes no part.  A point with a non-finite coordinate enters no box and its output is its input z.
 *   PCC_MORPH_ERODE: out_i = min z_j over B(i); DILATE: max; OPEN: e = ERODE(z), out_i = max e_j over B(i); CLOSE: its dual.
 *   The results are exact by value (a zero's sign is unspecified: min / max of floats depend on the order in nothing else).
 * out_z[n]: space `mem`.  n == 0: PCC_OK.  Device memory: enqueued, no wait.  Host memory: one wait, at the end.
 * How: the points are binned into an xy lattice (cell side window / 8, doubled until the table has at most max(16384, n) and
 *   at most 2^20 cells), sorted by cell, and
 *   every cell's min / max is reduced once; a point takes the aggregates of the cells strictly inside its cell range and tests
 *   the points of the rim cells with the comparisons above.  The binning is monotone, so the result does not depend on the
 *   lattice.  A window whose boxes all hold the whole cloud is one global min / max.
 * Refused before any device is touched, in this order: a bad memory space, point pointer, stride or 2^31 points and more (as
 *   everywhere); a null out_z with n > 0; an op outside pcc_morph_op; a window that is not finite and positive
 *   (PCC_ERR_INVALID); a null handle last.
 * `ctx` is any index handle: the cloud it indexes, its tie order and its kept rows are neither read nor changed. */
int pcc_morphological_operator(pcc_index *ctx, const void *pts, size_t n, size_t stride_bytes, int mem, float window, int op,
                               float *out_z);
/* pcl::ProgressiveMorphologicalFilter::extract (src/segmentation.cpp:330-387, the filter between the voxel grid and
 * ExtractIndices): the window table of pcc_pmf_windows, then
 *     ground = all indices, ascending
 *     for each (w, h):  o = OPEN over the points of `ground` alone;  keep i when (z_i - o_i) < h  (strict);  the order stays
 * One deviation from PCL: a point with a non-finite coordinate is never ground (PCL lets one with finite z through; the
 *   reference's voxel grid drops such points first).
 * out_ground[n] (space `mem`): the original indices of the ground points, ascending, *n_ground (HOST) of them.
 * out_pass_sizes (HOST, may be NULL): the survivors after each window, min(windows, max_passes) entries.
 * The cloud goes up once, the survivors are compacted on the device between windows, and the host waits once per window (for
 *   the survivor count): launches and waits do not depend on n.  n == 0 or no finite point: PCC_OK, *n_ground = 0.
 * Refused before any device is touched, in this order: what pcc_morphological_operator refuses about the cloud; a null
 *   out_ground with n > 0 or a null n_ground; what pcc_pmf_windows refuses (a table longer than PCC_PMF_MAX_WINDOWS is
 *   PCC_ERR_OVERFLOW); a null handle last. */
int pcc_progressive_morphological_filter(pcc_index *ctx, const void *pts, size_t n, size_t stride_bytes, int mem,
                                         int max_window_size, float slope, float initial_distance, float max_distance,
                                         float cell_size, float base, int exponential,
                                         int32_t *out_ground, size_t *n_ground, size_t *out_pass_sizes, size_t max_passes);
/* ground_segmentation (src/segmentation.cpp:330-387) in one call.  Every output is, bit for bit, what this sequence gives:
 *     pcc_voxel_grid(ctx, pts, n, stride_bytes, mem, leaf, has_rgb = 0, F, out_stride_bytes, &nv)      -> out_points, *n_filtered
 *     pcc_progressive_morphological_filter(ctx, F, nv, out_stride_bytes, mem, ...)                      -> out_ground_index, *n_ground
 *     out_ground_points = the records of F at out_ground_index; out_object_points = those of every other index, ascending
 *   but the filtered cloud stays on the device throughout.
 * out_points, out_ground_points, out_object_points (space `mem`; capacity n records of out_stride_bytes; the last two may be
 *   NULL): whole voxel-grid records, the bytes pcc_voxel_grid does not write zero in both memory spaces; *n_ground of them in
 *   out_ground_points (the reference's <name>_ground cloud), *n_filtered - *n_ground in out_object_points.  out_ground_index[n]
 *   (space `mem`, may be NULL).  *n_filtered, *n_ground: HOST.
 * n == 0 or no finite point: PCC_OK, both counts 0.
 * Refused before any device is touched, in this order: what pcc_voxel_grid refuses (same messages); a null n_filtered or
 *   n_ground; what pcc_pmf_windows refuses; a null handle last. */
int pcc_ground_segmentation(pcc_index *ctx, const void *pts, size_t n, size_t stride_bytes, int mem, float leaf,
                            int max_window_size, float slope, float initial_distance, float max_distance,
                            float cell_size, float base, int exponential,
                            void *out_points, size_t out_stride_bytes, size_t *n_filtered,
                            int32_t *out_ground_index, size_t *n_ground, void *out_ground_points, void *out_object_points);
/* ---- RIFT descriptors of the indexed cloud ---------------------------------------------------------
 * replaces: processRIFT (src/comparator.cpp:590-684) for one cloud: pcl::PointCloudXYZRGBtoXYZI, pcl::NormalEstimation
 *   (setRadiusSearch 0.03, :628-635), removeNaNNormalsFromPointCloud (:637-646), pcl::IntensityGradientEstimation
 *   (setRadiusSearch 0.03), pcl::RIFTEstimation (setRadiusSearch 0.05, 4 distance x 8 gradient bins) and the removal of
 *   descriptors whose first bin is not finite (:676-682).  The PCL stages are restated from the published algorithms
 *   ([recalled]): parity with PCL 1.7 itself is unpinned.
 * Every neighbourhood is the sorted radius row of the library (d2 < float(r^2), ascending (d2, index), the point itself
 * included), taken among the points that are still in the cloud at that stage:
 *   intensity  0.299f r + 0.587f g + 0.114f b of the bytes, left to right;
 *   normals    pcc_normals_radius at normal_radius, viewpoint origin; points without a finite normal leave (cloud2);
 *   gradient   per point of cloud2, rows of cloud2 at gradient_radius: fewer than 3 entries -> NaN, else the least-squares
 *              slope of the intensity about the row's centroid (3 x 3 normal equations, column-pivoted Householder QR)
 *              projected onto the tangent plane of the point's normal;
 *   RIFT       per point of cloud2, rows of cloud2 at rift_radius: every entry votes its gradient magnitude into the
 *              (distance, angle) bins bilinearly, in row order; the histogram is divided by its 2-norm; a NaN gradient
 *              anywhere in the row makes the histogram NaN (PCL's behaviour); those leave.
 * rgb: PCL's packed colour word of point i (bytes b, g, r, a from the low byte: offset 16 of pcl::PointXYZRGB) at
 *   rgb + i * rgb_stride_bytes, memory space `mem`, 4-byte aligned, one per point of the indexed cloud.
 * out_histograms[n][32] (word g_bin * 4 + d_bin, as pcl::Histogram<32> holds it) and out_point_index[n] (the ORIGINAL index
 *   of every kept descriptor, ascending -- PCL does not return it), memory space `mem`, sized by the caller for all n points
 *   of the indexed cloud; the first *n_out (host) rows are written.
 * Only nr_distance_bins = 4, nr_gradient_bins = 8 is built: anything else is PCC_ERR_UNSUPPORTED.  Null arguments, radii
 * that are not positive and finite, a bad stride or memory space are refused before any device is touched. */
int pcc_rift_descriptors(pcc_index *index, const void *rgb, size_t rgb_stride_bytes, int mem, double normal_radius,
                         double gradient_radius, double rift_radius, int nr_distance_bins, int nr_gradient_bins,
                         float *out_histograms, int32_t *out_point_index, size_t *n_out);
/* The same for EVERY cluster of a comparison at once -- replaces the per-cluster descriptor loop of the comparison
 *   (src/comparator.cpp:1224-1272: processRIFT, :590-684, or processRIFTwithSIFT ending in it, once per cluster of both
 *   scenes; no call depends on an earlier one).  The clouds of a call are concatenated on the device and every stage runs
 *   once over all of them: one upload, one CSR build per radius, one pass of each stage.  Launches and host waits do not
 *   depend on n_clouds: one wait per CSR (two; three when gradient_radius != normal_radius), one for the slice bounds and
 *   one for the rows coming back.
 *   ctx: any index handle, as for pcc_match_knn_batch and pcc_voxel_grid: it supplies device, stream and scratch; the cloud
 *     it indexes is neither read nor changed.
 *   Cloud c is the n[c] points at pts[c] + i * stride_bytes (x, y, z) with PCL's packed colour word of each at
 *     rgb[c] + i * rgb_stride_bytes; for 32-byte pcl::PointXYZRGB records rgb[c] = pts[c] + 16 with the same stride.  Its
 *     result is, bit for bit and in order, what pcc_index_create(pts[c], ...) + pcc_rift_descriptors(...) returns for that
 *     cloud alone: its histograms are rows out_offsets[c] .. out_offsets[c + 1] of out_histograms, its point indices --
 *     LOCAL to the cloud, ascending -- the same rows of out_point_index.  No point of another cloud enters a neighbourhood,
 *     however the clouds overlap in space.  A cloud with n[c] == 0 or without a finite point yields an empty slice (the
 *     single path answers PCC_ERR_EMPTY there).
 *   out_histograms[sum(n)][32], out_point_index[sum(n)], out_offsets[n_clouds + 1]: HOST arrays.  mem must be PCC_MEM_HOST
 *     (PCC_MEM_DEVICE: PCC_ERR_UNSUPPORTED).  n_clouds == 0: PCC_OK, out_offsets[0] = 0, no device is touched.
 *   Clouds above PCC_OPT_RIFT_BATCH_BRUTE_MAX points take the single path inside the call (same bits).  pcc_index_stats
 *     afterwards reports in [0] the points whose rows the batch kernels built and in [1] the points of the clouds sent
 *     through the work handle.
 *   Refused before the handle is looked at, with pcc_rift_descriptors' messages where it has one: null arrays, a null
 *     pts[c] or rgb[c] with n[c] > 0, a bad stride or alignment, radii that are not positive and finite, bins other than
 *     4 x 8 (PCC_ERR_UNSUPPORTED), sum(n) >= 2^31 (PCC_ERR_UNSUPPORTED).  A CSR of 2^32 entries or more over the whole batch
 *     is PCC_ERR_OVERFLOW. */
int pcc_rift_descriptors_batch(pcc_index *ctx, size_t n_clouds,
                               const void *const *pts, const size_t *n, size_t stride_bytes,
                               const void *const *rgb, size_t rgb_stride_bytes, int mem,
                               double normal_radius, double gradient_radius, double rift_radius,
                               int nr_distance_bins, int nr_gradient_bins,
                               float *out_histograms, int32_t *out_point_index, size_t *out_offsets);
/* ---- FPFH descriptors of the indexed cloud ---------------------------------------------------------
 * replaces: processFPFH (src/comparator.cpp:824-875) for one cloud: pcl::NormalEstimation (setRadiusSearch 0.03),
 *   removeNaNNormalsFromPointCloud, and pcl::FPFHEstimation (setRadiusSearch 0.05, 11 + 11 + 11 bins) over the points that
 *   are left.  The PCL stages are restated from the published algorithm ([recalled]): PCL 1.7 is not
 *   available to compare against, parity with it is unpinned.
 * Every neighbourhood is the sorted radius row of the library (d2 < float(r^2), ascending (d2, index), the point itself
 * included), taken among the points of cloud2 -- the points with a finite normal; no compacted cloud is built before the
 * final output, the stages skip the entries of the others:
 *   normals    pcc_normals_radius at normal_radius, viewpoint origin; points without a finite normal leave (cloud2);
 *   pair       pcl::computePairFeatures of (p, q): dp = q - p, f4 = |dp| (0: no pair); a1 = n_p.dp / f4, a2 = n_q.dp / f4;
 *              acosf|a1| > acosf|a2| exchanges p and q, negates dp and sets f3 = -a2, else f3 = a1; v = dp x n_1 (|v| = 0: no
 *              pair), v /= |v|, w = n_1 x v, f2 = v.n_2, f1 = atan2f(w.n_2, n_1.n_2);
 *   SPFH       computePointSPFHSignature per point p of cloud2 over its fpfh_radius row: incr = 100.0f / float(row_len - 1),
 *              row_len counting the cloud2 entries, p itself included; every entry other than p that has a pair adds incr to
 *              bin floor(11 (f1 + pi) / (2 pi)) of the first eleven, floor(11 (f2 + 1) / 2) of the second and
 *              floor(11 (f3 + 1) / 2) of the third (evaluated in double, clamped to 0 .. 10);
 *   weighting  weightPointSPFHSignature per point p of cloud2 over the same row, in row order: every entry q with d2 != 0
 *              adds spfh[q][b] * (1.0f / d2) to bin b and, entry by entry and bin by bin, to the running sum of b's feature;
 *              each feature's eleven bins are then multiplied by float(100.0 / sum) (a zero sum: by 0).
 * out_histograms[n][33] (the f1 bins, then f2, then f3, as pcl::FPFHSignature33 holds them) and out_point_index[n] (the
 *   ORIGINAL index of every descriptor's point, ascending: the points of cloud2 -- processFPFH keeps exactly these and
 *   removes nothing afterwards), memory space `mem`, sized by the caller for all n points of the indexed cloud; the first
 *   *n_out (host) rows are written.  No colour is read.
 * Refused before the handle is looked at, in this order: a bad memory space; a null output or n_out; a radius that is not
 *   positive and finite; bins other than 11, 11, 11 (PCC_ERR_UNSUPPORTED); a null handle last.  A refused call writes
 *   nothing.  Host waits: the row totals of the two CSRs (one when the radii are equal) and the count.
 * PCC_OPT_FPFH_LAYOUT chooses between two forms of the two kernels; no result bit depends on it. */
int pcc_fpfh_descriptors(pcc_index *index, int mem, double normal_radius, double fpfh_radius,
                         int nr_bins_f1, int nr_bins_f2, int nr_bins_f3,
                         float *out_histograms, int32_t *out_point_index, size_t *n_out);
/* ---- SHOT352 descriptors of the indexed cloud -------------------------------------------------------
 * replaces: processSHOT (src/comparator.cpp:941-986) for one cloud: pcl::NormalEstimation (setRadiusSearch 0.05),
 *   removeNaNNormalsFromPointCloud, and pcl::SHOTEstimation<PointXYZRGB, Normal, SHOT352> (setRadiusSearch 0.04) over the
 *   points that are left.  Lines 915-939 of processSHOT -- the SIFT keypoints, the rand() % total draw and the snap of the
 *   drawn keypoints to the cloud -- stay with the caller: pcc_sift_keypoints and pcc_first_within cover the two library
 *   steps, the draw is the caller's business.  The PCL stages are restated from the published source of PCL 1.7
 *   (shot.hpp, shot_lrf.hpp; DESIGN.md 4.31, every stage below [recalled]): PCL is not available to compare against,
 *   parity with it is unpinned.
 * Every neighbourhood is the sorted radius row of the library at shot_radius (d2 < float(r^2), ascending (d2, index), the
 * point itself included), taken among the points of cloud2 -- the points with a finite normal; no compacted cloud is built
 * before the final output, the stages skip the entries of the others.  When shot_radius <= normal_radius one CSR is built
 * (at normal_radius) and the SHOT stages walk the prefix of each row with d2 < float(shot_radius^2); otherwise two.
 *   normals    [recalled, unpinned] pcc_normals_radius at normal_radius, viewpoint origin; points without a finite normal
 *              (a non-finite point among them) leave (cloud2);
 *   frame      [recalled, unpinned] SHOTLocalReferenceFrameEstimation::getLocalRF with lrf_radius = shot_radius, per point p
 *              over its row in order, skipping entries with d2 == 0: v = q - p in float per component, promoted to double;
 *              w = double(shot_radius) - sqrtf(d2) (the root in float, then promoted); cov_ij += w * (v_i * v_j) and
 *              sum += w in double, entry by entry in row order; valid = the entries used, valid < 5: the frame is nine NaN;
 *              cov_ij / sum, a division per entry.  Eigenvectors: cyclic Jacobi in double from + - * / sqrt alone; a sweep
 *              rotates the pairs (0,1), (0,2), (1,2) in this order, skipping an off-diagonal that is exactly 0.0 and
 *              setting one to 0.0 without a rotation when |a_pp| + |a_pq| == |a_pp| and |a_qq| + |a_pq| == |a_qq|, with
 *              theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), sign(0) = +1,
 *              c = 1 / sqrt(t^2 + 1), s = t c; it stops when all three off-diagonals are exactly 0.0, at the latest after
 *              32 sweeps.  x = the eigenvector of the largest eigenvalue, z = of the smallest, chosen by PCL's if-chain
 *              over the eigenvalues e0, e1, e2 in the solver's order with strict '>' throughout:
 *              e0 > e1 ? (e0 > e2 ? x = 0, z = (e1 > e2 ? 2 : 1) : x = 2, z = 1) : (e1 > e2 ? x = 1, z = (e0 > e2 ? 2 : 0)
 *              : x = 2, z = 0) -- among equal eigenvalues the later column counts as the larger.  An eigenvalue that is not
 *              finite: nine NaN.  Sign of x over the valid entries in row order, dots in double ((v0 x0 + v1 x1) + v2 x2):
 *              plus = the count of v . x >= 0, s = 2 plus - valid; s < 0 negates x; s == 0 takes the five entries
 *              valid / 2 - 2 .. valid / 2 + 2 of that list and negates x when fewer than 3 of them have v . x > 0.  The same
 *              for z.  rf rows: float(x), y = z cross x in float, float(z);
 *   bins       [recalled, unpinned] computePointSHOT + interpolateSingleChannel, 32 volumes x 11 bins.  A row of fewer than 5
 *              cloud2 entries (p included) or a NaN frame: 352 NaN.  Else per entry q in row order: distance =
 *              double(sqrtf(d2)), skipped when |distance| < 1e-15; cosine = double(n_q . z) (a float dot), clamped to +-1,
 *              bin = (1 + cosine) * 10 / 2; xF, yF, zF = double(delta . x / y / z), float dots of delta = q - p, each set to 0
 *              when |.| < 1e-30; desc_index: bit4 = yF > 0 || (yF == 0 && xF < 0), bit3 = (xF > 0 || (xF == 0 && yF > 0)) ?
 *              !bit4 : bit4, index = (bit4 << 3 + bit3 << 2) << 1; the 45 degree half: xF yF > 0 || xF == 0 ? (|xF| >= |yF| ?
 *              0 : 4) : (|xF| > |yF| ? 4 : 0); + 1 for zF > 0; + 2 for distance > r / 2.  step = floor(bin + 0.5),
 *              bin -= step, and the contributions are added in this order, each a float add of float(|.|) into a float bin:
 *              (1) |bin| to bin (step +- 1) mod 10 of the same volume (+ for bin > 0); (2) the radial neighbour volume
 *              desc_index -+ 2 at step: (distance - 3r/4) / (r/2) in the outer husk when distance <= 3r/4,
 *              (distance - r/4) / (r/2) in the inner husk when distance >= r/4; (3) the inclination neighbour volume
 *              desc_index +- 1 at step: inclination = acos(clamp(zF / distance)); above 90 degrees (or within 1e-30 of it
 *              with zF <= 0) (inclination - 135) / 90 when inclination <= 135, else (inclination - 45) / 90 when
 *              inclination >= 45; (4) when xF or yF is not 0 the azimuth neighbour volume (desc_index +- 4) mod 32 at
 *              step: (atan2(yF, xF) - (-7 pi / 8 + (pi / 4) (desc_index >> 2))) / (pi / 4) clamped to +-0.5 (+ 4 when it is
 *              > 0); (5) the centre bin desc_index * 11 + step gets float(weight), weight = the sum of 1 - |d| over the four
 *              interpolations in double.  acos and atan2 are the library's own (csrc/libm_f64.hpp: fdlibm's e_acos.c,
 *              s_atan.c and e_atan2.c restated from + - * / sqrt: the same bits on the device and on a host).  The order of
 *              the adds, entry by entry, is part of the result.  Then norm = sqrt(sum of double(b) * double(b)) over the
 *              bins in index order, one chain in double, and every bin is divided by float(norm).  The constants are PCL's
 *              PST_* literals.
 * out_descriptors[n][352] (pcl::SHOT352::descriptor), out_rf[n][9] (pcl::SHOT352::rf: x, y, z axis; nullable) and
 *   out_point_index[n] (the ORIGINAL index of every descriptor's point, ascending: the points of cloud2 -- processSHOT
 *   keeps exactly these), memory space `mem`, sized by the caller for all n points of the indexed cloud; the first *n_out
 *   (host) rows are written.  NaN rows stay: the reference keeps them and matchSHOT tests descriptor[0].  No colour is read.
 * Refused before the handle is looked at, in this order: a bad memory space; a null out_descriptors, out_point_index or
 *   n_out; a radius that is not positive and finite ("bad radius"); a null handle last.  A refused call writes nothing.
 *   Host waits: the row totals of the CSRs (one when shot_radius <= normal_radius) and the count; neither launches nor
 *   waits depend on n. */
int pcc_shot_descriptors(pcc_index *index, int mem, double normal_radius, double shot_radius,
                         float *out_descriptors /* mem, [n][352] */, float *out_rf /* mem, [n][9], nullable */,
                         int32_t *out_point_index /* mem, [n] */, size_t *n_out /* host */);
/* The same for EVERY cluster of a segmentation at once -- the producer of pcc_match_fpfh_batch's descriptor arrays.  The
 *   clusters of a call are concatenated on the device and every stage runs once over all of them; launches and host waits
 *   do not depend on n_clusters.
 *   ctx: any index handle, as for the other batch calls: it supplies device, stream and scratch; its cloud, tie order and
 *     kept rows are neither read nor changed.
 *   Cluster c is the points offsets[c] .. offsets[c + 1] of pts (records stride_bytes apart, x, y, z first, memory space
 *     `mem`; no colour is read): pcc_cluster_descriptors' input, what pcc_region_growing_segmentation and
 *     pcc_euclidean_cluster_segmentation write as out_cluster_points / out_offsets.  offsets is a HOST array.
 *   Its result is, bit for bit and in order, what pcc_index_create on that cluster alone + pcc_fpfh_descriptors returns:
 *     rows out_offsets[c] .. out_offsets[c + 1] of out_histograms and out_point_index, the point indices LOCAL to the
 *     cluster and ascending.  No point of another cluster enters a row, however the clusters overlap in space.  An empty
 *     cluster, or one without a finite point, yields an empty slice.
 *   out_histograms[offsets[n_clusters] - offsets[0]][33] and out_point_index (as many rows) are in memory space `mem`;
 *     out_offsets[n_clusters + 1] is a HOST array in either space.  With PCC_MEM_DEVICE the descriptors are written where
 *     they stay: out_histograms + 33 * out_offsets[c] with stride 132 is a valid des1[p] / des2[p] of
 *     pcc_match_fpfh_batch(mem = PCC_MEM_DEVICE), and no descriptor crosses to the host between the two calls.
 *   normal_radius <= fpfh_radius (the reference's 0.03 / 0.05): ONE CSR is built, at fpfh_radius -- a sorted row at
 *     normal_radius is the prefix of it with d2 < float(normal_radius^2), and the plane fit walks that prefix.  Otherwise two.
 *   Clusters above PCC_OPT_FPFH_BATCH_BRUTE_MAX points take the single path inside the call, on a work handle kept in ctx, in
 *     the caller's memory space (same bits); their slices are spliced in cluster order.  pcc_index_stats afterwards reports in
 *     [0] the points the batch kernels served, in [1] the points sent through the work handle and in [2] the CSRs the batch
 *     route built (0, 1 or 2).
 *   Host waits with no cluster above the limit: one per CSR built, one for the slice bounds and, for a host caller, one for
 *     the rows.
 *   n_clusters == 0: PCC_OK, out_offsets[0] = 0, no device is touched.  Refused before the handle is looked at, in this
 *     order: a bad memory space; a null offsets or out_offsets, or null pts / out_histograms / out_point_index while a
 *     cluster holds a point; a bad stride, or pts / outputs that are not 4-byte aligned; offsets that decrease
 *     (PCC_ERR_INVALID), then 2^31 points or clusters and more (PCC_ERR_UNSUPPORTED); a radius that is not positive and
 *     finite, then bins other than 11, 11, 11 (PCC_ERR_UNSUPPORTED), with pcc_fpfh_descriptors' messages; a null handle
 *     last.  A refused call writes nothing.  A CSR of 2^32 entries or more over the whole batch is PCC_ERR_OVERFLOW. */
int pcc_fpfh_descriptors_batch(pcc_index *ctx,
                               const void *pts, size_t stride_bytes,
                               const size_t *offsets /* HOST [n_clusters + 1] */, size_t n_clusters, int mem,
                               double normal_radius, double fpfh_radius,
                               int nr_bins_f1, int nr_bins_f2, int nr_bins_f3,
                               float *out_histograms /* mem, [offsets[n_clusters] - offsets[0]][33] */,
                               int32_t *out_point_index /* mem, same rows */,
                               size_t *out_offsets /* HOST [n_clusters + 1] */);
/* ---- VFH descriptor of the indexed cloud -------------------------------------------------------------
 * replaces: processVHF (src/comparator.cpp:482-516) for one cloud: pcl::NormalEstimation (setRadiusSearch 0.03) and
 *   pcl::VFHEstimation<PointXYZRGB, Normal, VFHSignature308> with setNormalizeBins(true) and setNormalizeDistance(false) --
 *   the reference's only GLOBAL descriptor: one 308-bin histogram for the whole cloud.  normalize-bins on, normalize-distance
 *   off, no size component and the viewpoint (0, 0, 0) are constants of the call.  The PCL stage is restated from the
 *   published algorithm ([recalled]): PCL 1.7 is not available to compare against, parity with it is unpinned.
 *   normals    pcc_normals_radius at normal_radius, viewpoint origin.  A point whose row has fewer than 3 entries keeps a NaN
 *              normal; processVHF does NOT remove such points (unlike processFPFH): they stay in the cloud and vote;
 *   centroids  xyz: three float chains from 0.0f over the n points in index order, each divided by float(n).  Normals: three
 *              float chains from 0.0f in index order over the cp points whose normal has three finite components, each divided
 *              by float(cp) (cp == 0: 0 / 0 = NaN, and the arithmetic below runs with it);
 *   d_vp_p     d = 0.0f - centroid, d / sqrtf(d . d) (a true division);
 *   pair       per point i in index order pcl::computePairFeatures(centroid, normal centroid, p_i, n_i) as pcc_fpfh_descriptors
 *              states it, with whatever the normal holds.  No pair (the point AT the centroid, or the connecting line along
 *              the source's normal): no vote.  Otherwise one vote each into bin floor(45 (f1 + pi) / (2 pi)) of the first 45
 *              bins, floor(45 (f2 + 1) / 2) of the second and floor(45 (f3 + 1) / 2) of the third (evaluated in double, clamped
 *              to 0 .. 44; anything that is not >= 0, a NaN included, is bin 0 -- so a point with a NaN normal votes bin 0 of
 *              f1 and f2 and its real f3 bin).  Every vote adds 100.0f / float(n - 1); a bin with `count` votes holds that
 *              increment added count times in float;
 *   f4         bins 135 .. 179: the distance component's increment is 0, every bin is +0.0f;
 *   viewpoint  bins 180 .. 307, every point (NaN normals included): alpha = (double(n_i . d_vp_p) + 1.0) * 0.5, bin
 *              floor(alpha * 128.0) clamped to 0 .. 127 (NaN: 0); every vote adds float(100.0 / double(n)).
 * out_histogram[308] in memory space `mem`: f1[45], f2[45], f3[45], f4[45], viewpoint[128], as pcl::VFHSignature308 holds them.
 *   *n_out (host): 1, or 0 for a cloud of fewer than 2 points (PCL's initCompute fails and the reference gets an empty
 *   cloud): PCC_OK, nothing is written.  Votes are counted in integers and every bin is rebuilt from its count: the result
 *   does not depend on the order the points arrive in, no float atomic takes part.  No colour is read.
 * A cloud with a non-finite point is refused (PCC_ERR_UNSUPPORTED): the reference strips such points when it loads a cloud
 *   (:1144-1148), processVHF never sees one.
 * Refused before the handle is looked at, in this order: a bad memory space; a null output or n_out; a radius that is not
 *   positive and finite; a null handle last.  A refused call writes nothing.  Host waits: the row total of the CSR, and the
 *   results of a caller in host memory; neither launches nor waits depend on n. */
int pcc_vfh_descriptor(pcc_index *index, int mem, double normal_radius,
                       float *out_histogram /* mem, [308] */, size_t *n_out /* 1, or 0 */);
/* matchVHF (src/comparator.cpp:471-480) for every pair of two arrays of VFH descriptors:
 *   out_dist[i * n2 + j] = sqrt(sum over k = 0 .. 307, in order, of (double)(hist1[i][k] - hist2[j][k])^2)
 *   -- the subtraction in float, the square (pow(x, 2) of a promoted float: exact) and the running sum in double, the root in
 *   double.  The reference compares element 0 of two clouds: n1 = n2 = 1.  A NaN bin gives a NaN distance.
 * hist1[n1][308], hist2[n2][308] and out_dist[n1 * n2] (row-major) in memory space `mem`; ctx lends device, stream and
 *   scratch, the cloud it indexes is neither read nor changed.  n1 == 0 or n2 == 0: PCC_OK, nothing is written.
 * Refused before the handle is looked at, in this order: a bad memory space; a null array (with n1 and n2 both > 0); more
 *   than 2^31 - 1 pairs (PCC_ERR_UNSUPPORTED); a null handle last. */
int pcc_match_vfh(pcc_index *ctx, const float *hist1, size_t n1, const float *hist2, size_t n2, int mem,
                  double *out_dist /* mem, [n1 * n2] */);
/* pcc_vfh_descriptor for EVERY cluster of a segmentation at once -- the producer of pcc_match_vfh's descriptor arrays.  The
 *   clusters of a call are concatenated on the device; the row builder, the plane fit, the centroid chains (one wave per
 *   cluster, side by side), the votes and the bins each run in one launch over all of them: neither launches nor host waits
 *   depend on n_clusters.
 *   ctx: any index handle, as for the other batch calls: it supplies device, stream and scratch; its cloud, tie order and
 *     kept rows are neither read nor changed.
 *   Cluster c is the records offsets[c] .. offsets[c + 1] of pts (stride_bytes apart, x, y, z first, memory space `mem`; no
 *     colour is read): pcc_fpfh_descriptors_batch's input, what pcc_region_growing_segmentation and
 *     pcc_euclidean_cluster_segmentation write as out_cluster_points / out_offsets.  offsets is a HOST array.
 *   Its result is, bit for bit, what pcc_index_create on that cluster alone + pcc_vfh_descriptor returns: rows
 *     out_offsets[c] .. out_offsets[c + 1] of out_histograms -- one row for a cluster of 2 points and more, none for a cluster
 *     of 0 or 1 points.  No point of another cluster enters a row of the CSR, a centroid chain or a counter, however the
 *     clusters overlap in space.  Votes are counted in integers: no float atomic takes part.
 *   out_offsets[n_clusters + 1] (HOST in either space) depends on the cluster sizes alone: it is computed on the host before
 *     anything is launched and no host wait exists for it.  out_histograms holds one row of 308 floats per cluster at most, in
 *     memory space `mem`.  With PCC_MEM_DEVICE every descriptor is written where it stays, whichever route its cluster takes:
 *     rows out_offsets[c] of two such arrays are valid hist1 / hist2 of pcc_match_vfh(mem = PCC_MEM_DEVICE), and no descriptor
 *     crosses to the host between the calls.  The rows of a host caller are staged and copied down in merged runs.
 *   Clusters above PCC_OPT_VFH_BATCH_BRUTE_MAX points take the single call inside this one, on a work handle kept in ctx, in
 *     the caller's memory space, straight into their row (same bits).  pcc_index_stats afterwards reports in [0] the points
 *     the batch kernels served, in [1] the points sent through the work handle and in [2] the descriptors written.
 *   Non-finite points: a cluster of fewer than 2 points is never read and yields no row whatever it holds (the single call
 *     WOULD look at such a cloud, and refuse it for a non-finite point).  A cluster of 2 points and more that holds a
 *     non-finite point fails the call with PCC_ERR_UNSUPPORTED, the message naming one such cluster ("non-finite"):
 *     out_offsets is not written then, the contents of out_histograms are unspecified, the handle stays usable.  From host
 *     memory such a cluster on the batch route is refused before any launch, the lowest-numbered one named; from device
 *     memory the pack kernel flags it and the word is read after the wait of the CSR build.
 *   Host waits with no cluster above the limit: one for the CSR's total and, for a host caller, one for the rows.
 *   n_clusters == 0: PCC_OK, out_offsets[0] = 0, no device is touched.  Refused before the handle is looked at, in this
 *     order: a bad memory space; a null offsets or out_offsets, or a null pts / out_histograms while a cluster holds a point;
 *     a bad stride, or pts / out_histograms that are not 4-byte aligned; offsets that decrease (PCC_ERR_INVALID), then 2^31
 *     points or clusters and more (PCC_ERR_UNSUPPORTED); a radius that is not positive and finite; a null handle
 *     last.  A refused call writes nothing.  A CSR of 2^32 entries or more over the whole batch is PCC_ERR_OVERFLOW. */
int pcc_vfh_descriptors_batch(pcc_index *ctx,
                              const void *pts, size_t stride_bytes,
                              const size_t *offsets /* HOST [n_clusters + 1] */, size_t n_clusters, int mem,
                              double normal_radius,
                              float *out_histograms /* mem, [n_clusters][308] at most */,
                              size_t *out_offsets   /* HOST [n_clusters + 1] */);
/* ---- SIFT keypoints of a coloured cloud ---------------------------------------------------------------
 * replaces: processSift (src/comparator.cpp:435-469): pcl::SIFTKeypoint<PointXYZRGB, PointWithScale> with
 *   setScales(0.005f, 5, 5) and setMinimumContrast(0.001f), the detector in front of the keypoint snap (pcc_first_within)
 *   and of the RIFT stage (pcc_rift_descriptors) in processRIFTwithSIFT (:686-822).  The PCL stage is restated from the
 *   published algorithm ([recalled]): parity with PCL 1.7 itself is unpinned.
 * ctx: any index handle, as for pcc_voxel_grid: it supplies device, stream and scratch; the cloud it indexes is neither read
 *   nor changed.  The octave clouds are indexed on a work handle the library keeps inside ctx (reused across calls, freed
 *   with ctx).
 * pts / rgb: n points (x, y, z at pts + i * stride_bytes) and PCL's packed colour word of each (bytes b, g, r, a from the
 *   low byte) at rgb + i * rgb_stride_bytes, memory space `mem`; for 32-byte pcl::PointXYZRGB records rgb = pts + 16 with the
 *   same stride.
 * PCL 1.7 SIFTKeypoint::detectKeypoints, float32 throughout, every operation rounded on its own, sums in row order.  Per
 * octave o, scale = min_scale * 2^o (a float, doubled per octave):
 *   1. the current cloud (the input for the first octave) through pcc_voxel_grid with leaf = scale, colour averaged per
 *      channel and truncated; the octave cloud is in ascending voxel-index order, non-finite points drop out here;
 *   2. fewer than 25 points end the loop (PCL's min_nr_points);
 *   3. scales[i] = scale * powf(2.0f, (float(i) - 1.0f) / float(nr_scales_per_octave)), i = 0 .. nr_scales_per_octave + 2;
 *   4. intensity float(299 r + 587 g + 114 b) / 1000.0f of the averaged bytes;
 *   5. scale space, per point: the sorted radius row over the octave cloud at 3.0f * scales.back() (d2 < float(r^2),
 *      ascending (d2, index), the point itself first); per scale sigma2 = powf(s, 2.0f); the row is walked while
 *      d2 <= 9 * sigma2: w = expf(-0.5f * d2 / sigma2), num += value * w, den += w; response = num / den;
 *      dog(point, i - 1) = response_i - response_{i-1};
 *   6. extrema, per point: min_val / max_val of every DoG column over its min(25, n) nearest neighbours (self included);
 *      for the columns s = 1 .. nr_columns - 2 with v = dog(point, s) and fabs(v) >= min_contrast, a keypoint when
 *      v == min_val[s] && v < min_val[s-1] && v < min_val[s+1], or the mirrored maximum test holds:
 *      (x, y, z of the octave cloud's point, scales[s]);
 *   7. keypoints in order of octave, then point index within the octave cloud, then s (PCL's loop order).
 * out_keypoints[capacity][4] (x, y, z, scale) in memory space `mem`; *n_out (host) = the number of keypoints.  More than
 *   capacity: PCC_ERR_OVERFLOW, nothing written, *n_out = the number needed.  n == 0 or no finite point: *n_out = 0, PCC_OK.
 * Null arguments, a bad stride, alignment or memory space, a min_scale that is not positive and finite, a negative or NaN
 * min_contrast and nr_octaves < 1 are refused before any device is touched; so is nr_scales_per_octave outside 1 .. 13
 * (PCC_ERR_UNSUPPORTED: the kernels are built for up to 16 scales).  A first-octave lattice of more than 2^26 voxels is
 * pcc_voxel_grid's PCC_ERR_UNSUPPORTED (min_scale too small for the cloud's extent). */
int pcc_sift_keypoints(pcc_index *ctx, const void *pts, size_t n, size_t stride_bytes, const void *rgb,
                       size_t rgb_stride_bytes, int mem, float min_scale, int nr_octaves, int nr_scales_per_octave,
                       float min_contrast, float *out_keypoints /* [capacity][4]: x, y, z, scale */, size_t capacity,
                       size_t *n_out);
/* The same for EVERY cluster of a comparison at once, with the keypoint snap behind it -- replaces the front of
 *   processRIFTwithSIFT (src/comparator.cpp:686-822: processSift, :435-469, then every keypoint snapped to the first cluster
 *   point within 0.05, :696-713), which the reference runs once per cluster above 700 points of both scenes (:1228-1231,
 *   :1264-1265); no call depends on an earlier one.  The clouds of a call are concatenated on the device and every stage runs
 *   once per octave over all clouds still in the batch: launches and host waits depend on nr_octaves (three waits per octave
 *   round and one at the end), on the clouds above the brute limit and on buffer growth, never on n_clouds.
 *   ctx: any index handle, as for pcc_rift_descriptors_batch: it supplies device, stream and scratch; the cloud it indexes is
 *     neither read nor changed.
 *   Cloud c is described as in pcc_rift_descriptors_batch.  Its slice, rows out_offsets[c] .. out_offsets[c + 1] of
 *     out_keypoints, is bit for bit and in order (octave, point of the octave cloud, scale) what pcc_sift_keypoints returns for
 *     that cloud alone with the same four parameters.  No point of another cloud enters a voxel, a radius row or a 25-NN row,
 *     however the clouds overlap in space.  A cloud with n[c] == 0, without a finite point, or that stops at the 25-point gate
 *     in its first octave yields an empty slice; a cloud that falls below 25 points at a later octave is finished (PCL's
 *     break), the others go on.
 *   out_snap_index (nullable; snap_radius must then be positive and finite, else it is ignored): row by row the lowest LOCAL
 *     index j of the keypoint's own cloud with sqrt(dx^2 + dy^2 + dz^2) < snap_radius in pcc_first_within's arithmetic
 *     (differences in float, squares, sum and sqrt in double, strict compare), -1 when there is none: what
 *     pcc_index_create(cloud c) + pcc_first_within gives for those keypoints.
 *   out_keypoints[capacity][4], out_snap_index[capacity], out_offsets[n_clouds + 1]: HOST arrays; mem must be PCC_MEM_HOST
 *     (PCC_MEM_DEVICE: PCC_ERR_UNSUPPORTED).  More than capacity keypoints in total: PCC_ERR_OVERFLOW, out_offsets holds the
 *     offsets that would have been returned (out_offsets[n_clouds] = the number needed), nothing else is written.
 *     n_clouds == 0: PCC_OK, out_offsets[0] = 0, no device is touched.
 *   Clouds above PCC_OPT_SIFT_BATCH_BRUTE_MAX points take the single path inside the call (same bits).  pcc_index_stats
 *     afterwards reports in [0] the points that went through the batch kernels, in [1] the points of the clouds sent through
 *     the work handle and in [2] the octave rounds the batch route ran.
 *   Refused before the handle is looked at, with pcc_sift_keypoints' messages where it has one: null arrays, a null pts[c] or
 *     rgb[c] with n[c] > 0, a bad stride or alignment, bad values of the four SIFT parameters, sum(n) >= 2^31
 *     (PCC_ERR_UNSUPPORTED), and a first-octave lattice above 2^26 voxels for some cloud (PCC_ERR_UNSUPPORTED for the whole
 *     call; the message names the cloud). */
int pcc_sift_keypoints_batch(pcc_index *ctx, size_t n_clouds,
                             const void *const *pts, const size_t *n, size_t stride_bytes,
                             const void *const *rgb, size_t rgb_stride_bytes, int mem,
                             float min_scale, int nr_octaves, int nr_scales_per_octave, float min_contrast,
                             double snap_radius,
                             float *out_keypoints /* [capacity][4] */, int32_t *out_snap_index /* [capacity], nullable */,
                             size_t capacity, size_t *out_offsets /* [n_clouds + 1] */);
/* The per-cluster descriptor loop of a comparison in one call -- replaces the loop of src/comparator.cpp:1224-1290: a cluster
 *   above 700 points takes processRIFTwithSIFT (:686-822), the others processRIFT (:590-684), and every cluster's centroid is
 *   taken on the way (:1235-1247).  The clusters are staged once and stay on the device: the SIFT rounds, the keypoint snap, the
 *   gather of the snapped clouds, RIFT and the centroids; neither keypoints nor snap indices nor snapped clouds cross to the host.
 *   ctx: any index handle, as for the other batch calls: it supplies device, stream and scratch; its cloud, tie order and kept
 *     rows are neither read nor changed.
 *   Cluster c is points offsets[c] .. offsets[c + 1] of pts / rgb (records stride_bytes apart, x, y, z first; colour words
 *     rgb_stride_bytes apart), both in memory space `mem`, PCC_MEM_HOST or PCC_MEM_DEVICE -- what
 *     pcc_region_growing_segmentation and pcc_euclidean_cluster_segmentation write as out_cluster_points / out_offsets (32-byte
 *     records: rgb = pts + 16, same stride).  offsets (HOST, n_clusters + 1) is non-decreasing and spans fewer than 2^31 points.
 *   Its slice, rows out_offsets[c] .. out_offsets[c + 1] of out_histograms / out_point_index, bit for bit and in order:
 *     n_c <= sift_above (the dense route): what pcc_rift_descriptors_batch returns for that cluster alone.
 *     n_c > sift_above (the SIFT route): K = the cluster's keypoints from pcc_sift_keypoints_batch with the four SIFT parameters
 *       and snap_radius; S = their snap indices >= 0 in keypoint order, duplicates kept (:696-713); Q = the cluster's points and
 *       colours at S; (H, J) = what pcc_rift_descriptors_batch returns for Q.  The slice is H with point indices S[J]: the
 *       cluster-local index of the snapped point each descriptor was computed at.  No keypoints, or none snapped: empty.
 *     sift_above = SIZE_MAX sends every cluster the dense route.  No point of another cluster enters a voxel, a row or a
 *     neighbourhood.
 *   out_n_keypoints[c] (nullable): |K|; 0 on the dense route.
 *   out_centroids[c] (nullable): three float accumulators from 0.0f, += x / y / z of every point of the cluster in index order
 *     (non-finite points included), each divided by float(n_c); an empty cluster gives NaN.  The order of the additions is part
 *     of the result (pointcloudcomparator_amd/host/report.hpp: centroidOf).
 *   out_histograms[capacity][32], out_point_index[capacity], out_offsets[n_clusters + 1], out_n_keypoints[n_clusters],
 *     out_centroids[n_clusters][3]: HOST arrays.  More than capacity descriptors: PCC_ERR_OVERFLOW, out_offsets holds the offsets
 *     that would have been returned, nothing else is written.  n_clusters == 0: PCC_OK, out_offsets[0] = 0, no device is touched.
 *   SIFT-route clusters above PCC_OPT_SIFT_BATCH_BRUTE_MAX points take pcc_sift_keypoints' path and pcc_first_within on a work
 *     handle; dense clusters or snapped clouds above PCC_OPT_RIFT_BATCH_BRUTE_MAX take pcc_rift_descriptors on it (same bits).
 *     Launches and host waits depend on nr_octaves, on the clusters above the limits and on buffer growth, never on n_clusters.
 *     pcc_index_stats afterwards: [0] dense-route points, [1] SIFT-route points, [2] octave rounds, [3] keypoints, [4] snapped
 *     points, [5] points sent through the work handle.
 *   Refused before the handle is looked at, in this order: 1. a bad memory space; 2. null arrays; 3. a bad stride or alignment;
 *     4. offsets that decrease (PCC_ERR_INVALID) or span 2^31 points and more (PCC_ERR_UNSUPPORTED); 5. the SIFT parameters
 *     (pcc_sift_keypoints' checks); 6. the radii and bins (pcc_rift_descriptors' checks); 7. a snap_radius that is not positive
 *     and finite; 8. a null handle. */
int pcc_cluster_descriptors(pcc_index *ctx,
                            const void *pts, size_t stride_bytes, const void *rgb, size_t rgb_stride_bytes,
                            const size_t *offsets /* HOST [n_clusters + 1] */, size_t n_clusters, int mem,
                            size_t sift_above,
                            float min_scale, int nr_octaves, int nr_scales_per_octave, float min_contrast, double snap_radius,
                            double normal_radius, double gradient_radius, double rift_radius, int nr_distance_bins, int nr_gradient_bins,
                            float *out_histograms /* HOST [capacity][32] */, int32_t *out_point_index /* HOST [capacity] */, size_t capacity,
                            size_t *out_offsets /* HOST [n_clusters + 1] */,
                            uint32_t *out_n_keypoints /* HOST [n_clusters], nullable */,
                            float *out_centroids /* HOST [n_clusters][3], nullable */);
/* The cluster-matching loop of a comparison in one call -- replaces the loop of src/comparator.cpp:1296-1366: per cluster of
 *   scene 1 the three nearest free centroids of scene 2 (closestCentroid, :1069-1087), two gates, matchRIFTFeaturesKnn
 *   (:560-588) for every pair that passes them, and the acceptance rule on the NUMBER of correspondences (:1327-1357; the
 *   indices are never read).  The result is bit for bit what report::clusterSections (pointcloudcomparator_amd/host/report.hpp)
 *   computes with pcc_match_knn_batch_dims.  Candidates, gates and acceptance are host arithmetic; the searches of all pairs are
 *   one pass on the device that tracks the smallest distance per (pair, query) alone: every cluster that takes part is packed
 *   once, no index, no second minimum, no tie order, no FLANN tree.  One upload, one wait and one read-back of
 *   3 * n_clusters1 words per call, whatever the number of clusters or pairs; device memory adds none.
 *   ctx: any index handle, as for the other batch calls: it supplies device, stream and scratch; its cloud, tie order and kept
 *     rows are neither read nor changed.
 *   The descriptors of cluster c of scene s are records offsets_s[c] .. offsets_s[c + 1] of des_s, stride_bytes apart; both
 *     arrays in memory space `mem`, PCC_MEM_HOST or PCC_MEM_DEVICE.  With stride 128 that is what pcc_cluster_descriptors writes
 *     as out_histograms / out_offsets; centroids and point counts are what it and the segmentation calls return.  The first
 *     `dim` = 1 ... 32 floats of every record are read, as in pcc_match_knn_batch_dims.  offsets_s (HOST, n_clusters_s + 1) is
 *     non-decreasing and spans fewer than 2^31 records.
 *   out_candidates[i][k], k = 0, 1, 2: the nearest centroid of scene 2 not among candidates 0 .. k - 1 of i: differences
 *     in float, squares and their sum in double, the sum rounded to float, a float square root, strict < against a start value
 *     of 1e12f.  -1 when nothing qualifies (fewer than three clusters, a NaN centroid, a distance of 1e12 or more); among equal
 *     distances the lowest index.
 *   out_state[i][k]: 0 no candidate; 1 gated out by the descriptor counts (both must exceed 3; evaluated first); 2 gated out by
 *     size (the pair passes only when points2[j] / points1[i] == 1 as size_t division; points1[i] == 0 is gated out, not divided
 *     by); 3 searched.
 *   out_correspondences[i][k]: in state 3, 1 + the number of valid records q of scene-2 cluster j whose smallest distance to a
 *     valid record of scene-1 cluster i is a neighbour and < threshold (strict); else 0.  That is the length of the row
 *     pcc_match_knn_batch_dims returns for (des1 = cluster i, des2 = cluster j) with the same dim and threshold, under either
 *     tie order.  Distance: FLANN's L2_Simple in index order, every operation rounded on its own; a record is valid when its
 *     first dim floats are all finite; an overflowed distance is no neighbour; a cluster without a valid reference gives 1.
 *   out_matches[i]: -1 and best = 0 to start with; for k = 0, 1, 2 in state 3, corr = out_correspondences[i][k] and denom = the
 *     larger of the two descriptor counts: accepted when corr / denom >= 1 in integer division and corr > best; then best = corr
 *     and out_matches[i] = j.
 *   All four outputs, offsets, centroids and point counts are HOST arrays.  n_clusters1 == 0: PCC_OK without a handle or a
 *     device.  No pair in state 3: the tables are filled, PCC_OK, no device is touched.  pcc_index_stats afterwards: [0] the
 *     searched pairs, [1] the queries over all searched pairs.
 *   Refused before the handle is looked at, in this order: 1. dim outside 1 ... 32 (PCC_ERR_UNSUPPORTED); 2. a bad memory space;
 *     3. null arrays (a scene's arrays may be null while it has no cluster -- the outputs go with scene 1 --, its descriptor
 *     array while none of its clusters holds a record); 4. a stride that is not a multiple of 4 or below 4 * dim, or a
 *     descriptor pointer that is not 4-byte aligned; 5. offsets that decrease (PCC_ERR_INVALID) or span 2^31 records and more
 *     (PCC_ERR_UNSUPPORTED); 6. what pcc_match_knn_batch_dims refuses about the threshold (nothing: a NaN threshold counts
 *     nothing); 7. a null handle.  A refused call writes nothing. */
int pcc_cluster_matching(pcc_index *ctx,
                         const void *des1, const size_t *offsets1 /* HOST [n_clusters1 + 1] */, size_t n_clusters1,
                         const void *des2, const size_t *offsets2 /* HOST [n_clusters2 + 1] */, size_t n_clusters2,
                         size_t stride_bytes, int dim, int mem,
                         const float *centroids1 /* HOST [n_clusters1][3] */, const float *centroids2 /* HOST [n_clusters2][3] */,
                         const size_t *points1 /* HOST [n_clusters1] */, const size_t *points2 /* HOST [n_clusters2] */,
                         float threshold,
                         int32_t *out_candidates /* HOST [n_clusters1][3] */, int32_t *out_state /* HOST [n_clusters1][3] */,
                         uint32_t *out_correspondences /* HOST [n_clusters1][3] */, int32_t *out_matches /* HOST [n_clusters1] */);
int pcc_region_growing(pcc_index *index, const float *normals, int mem, int k, float smoothness,
                       float curvature_threshold, uint32_t min_size, uint32_t max_size,
                       int32_t *labels, int32_t *n_clusters);
/* ---- colour region growing -----------------------------------------------------------------------------
 * replaces: pcl::RegionGrowingRGB<PointXYZRGB>::extract as color_growing_segmentation configures it (src/segmentation.cpp:161-216:
 *   setDistanceThreshold(10), setPointColorThreshold(6), setRegionColorThreshold(5), setMinClusterSize(200), PCL's defaults of 30
 *   growing and 100 region neighbours; called twice per accepted match, src/comparator.cpp:1456-1495).  Nothing about normals or
 *   curvature is built: the reference never sets them.  The PCL stages are restated ([recalled]; the test
 *   oracle and pcc::RegionGrowingRGB are the same restatement): parity with PCL 1.7 itself is unpinned.
 * rows     the self k-NN rows of the indexed cloud, K = min(nr_region_neighbours, finite points), ascending (d2, index), the point
 *          itself first (PCL: findPointNeighbours); they stay on the device;
 * growing  edge u -> v is valid when v is among the first min(nr_neighbours, K) entries of u's row and the squared colour
 *          distance of the two (integer, cast to float) is <= point_color_threshold * point_color_threshold (a float product);
 *          the segment of v is the lowest index that reaches v along valid edges -- what PCL's queue computes with seeds in index
 *          order (region_rgb.hip) --, segments numbered by ascending seed index;
 * segment neighbours  for each ordered pair (s, t != s) the smallest row distance from a point of s to a point of t over all K
 *          entries; per s the nr_region_neighbours smallest by (d, t), handed on in descending (d, t);
 * merging  PCL's applyRegionMergingAlgorithm: mean colours float(sum) / float(count) truncated, the channel sums in unsigned int;
 *          segments within distance_threshold^2 whose means differ by less than region_color_threshold^2 join a region; regions
 *          below min_size fold into the region of their nearest neighbouring segment (stable sort of equal distances); clusters
 *          outside [min_size, max_size] are dropped.
 * rgb: PCL's packed colour word of point i (bytes b, g, r, a from the low byte) at rgb + i * rgb_stride_bytes, memory space `mem`,
 *   4-byte aligned, one per point of the indexed cloud -- as pcc_rift_descriptors takes it.
 * labels[n_original] (memory space `mem`): index of the point's cluster in PCL's output order, or -1; *n_clusters (host).
 *   Non-finite points of the indexed cloud take part in nothing and get -1; the finite points get what the NaN-stripped cloud
 *   would (the reference strips first, :164).
 * Only the per-segment records (16 bytes each) and the segment pair list (12 bytes each) cross to the host, where the merging
 *   runs; pcc_index_stats afterwards reports the grown segments in [0], the distinct ordered segment pairs in [1] and the label
 *   sweeps of the growing stage in [7].
 * Refused before any device is touched: a bad memory space, null rgb / labels / n_clusters, a bad stride or alignment, a threshold
 *   that is negative or not finite (PCC_ERR_INVALID); nr_neighbours == 0, nr_region_neighbours == 0 or > PCC_KNN_MAX_K
 *   (PCC_ERR_UNSUPPORTED); a null handle last.  An index without a finite point: PCC_ERR_EMPTY. */
int pcc_region_growing_rgb(pcc_index *index, const void *rgb, size_t rgb_stride_bytes, int mem,
                           float distance_threshold, float point_color_threshold, float region_color_threshold,
                           uint32_t min_size, uint32_t max_size,
                           unsigned int nr_neighbours, unsigned int nr_region_neighbours,
                           int32_t *labels, int32_t *n_clusters);
/* The same for EVERY cluster of a comparison at once -- replaces the two color_growing_segmentation calls per accepted match
 *   (src/comparator.cpp:1456-1495; body src/segmentation.cpp:161-216): all matches are known before the first is reported and
 *   no segmentation depends on another.  The clouds of a call are concatenated on the device and every stage runs once over
 *   all of them: one upload, one segmented k-NN pass, one pass of each growing stage, one sorted pair list cut per cloud on the
 *   host.  Launches and host waits do not depend on n_clouds: one wait per label sweep -- the sweeps end when no label moves in
 *   ANY cloud -- and four more (the segment count with the clouds' first ids, the pair count, the pair list, the labels).
 *   ctx: any index handle, as for pcc_rift_descriptors_batch: it supplies device, stream and scratch; the cloud it indexes,
 *     its tie order and its kept k-NN rows are neither read nor changed.
 *   Cloud c is described as in pcc_rift_descriptors_batch.  Its labels are rows sum(n[0..c)) .. sum(n[0..c]) of out_labels, its
 *     cluster count is out_n_clusters[c]; both are bit for bit what pcc_index_create(pts[c], ...) + pcc_region_growing_rgb(...)
 *     give on a fresh handle with the same seven parameters.  No point of another cloud enters a row, a segment or a segment
 *     pair, however the clouds overlap in space.  Non-finite points get -1 and take part in nothing.  A cloud with n[c] == 0
 *     writes nothing and reports 0 clusters; a cloud without a finite point gets all -1 and 0 clusters (the single path answers
 *     PCC_ERR_EMPTY there).
 *   out_labels[sum(n)], out_n_clusters[n_clouds]: HOST arrays.  mem must be PCC_MEM_HOST (PCC_MEM_DEVICE: PCC_ERR_UNSUPPORTED).
 *     n_clouds == 0: PCC_OK, no device is touched.
 *   Clouds above PCC_OPT_RGB_BATCH_BRUTE_MAX points, and every cloud when nr_region_neighbours > 128, take the single path
 *     inside the call on a work handle kept in ctx (reused across calls, freed with ctx; same bits).  pcc_index_stats afterwards
 *     reports, for the batch route, the grown segments in [0], the distinct ordered segment pairs in [1] and the label sweeps in
 *     [7]; in [2] the points that went through the batch kernels and in [3] the points of the clouds sent through the work handle.
 *   Refused before the handle is looked at, with pcc_region_growing_rgb's messages where it has one: null arrays, a null pts[c]
 *     or rgb[c] with n[c] > 0, a bad stride or alignment, a threshold that is negative or not finite, nr_neighbours == 0,
 *     nr_region_neighbours == 0 or > PCC_KNN_MAX_K (PCC_ERR_UNSUPPORTED), sum(n) >= 2^31 (PCC_ERR_UNSUPPORTED).  A batch route
 *     whose rows would hold 2^32 entries or more (points on the route x nr_region_neighbours) is PCC_ERR_UNSUPPORTED: split
 *     the call. */
int pcc_region_growing_rgb_batch(pcc_index *ctx, size_t n_clouds,
                                 const void *const *pts, const size_t *n, size_t stride_bytes,
                                 const void *const *rgb, size_t rgb_stride_bytes, int mem,
                                 float distance_threshold, float point_color_threshold, float region_color_threshold,
                                 uint32_t min_size, uint32_t max_size,
                                 unsigned int nr_neighbours, unsigned int nr_region_neighbours,
                                 int32_t *out_labels /* [sum(n)] */, int32_t *out_n_clusters /* [n_clouds] */);
/* The colour counts of a comparison's match loop in one call -- replaces, for all accepted matches at once, the two
 *   color_growing_segmentation calls of the match loop (src/comparator.cpp:1379-1509; the calls :1456-1495, the body
 *   src/segmentation.cpp:161-216), of which the loop keeps colors_segments_pcl1.size() and colors_segments_pcl2.size() alone.
 *   Where pcc_region_growing_rgb_batch takes one host pointer per cloud and brings every label back, this call takes the
 *   clusters as the segmentation calls write them -- records behind one another with offsets, in host or device memory -- and
 *   the match table pcc_cluster_matching writes, and returns the counts.  Every distinct (scene, cluster) the table names is
 *   segmented ONCE, however many matches name it (closestCentroid's exclusion set is per cluster of scene 1, so several
 *   clusters of scene 1 can be matched to one cluster of scene 2).  The named clusters are packed on the device into one
 *   concatenation (one launch, which also counts the finite points of every cluster) and pcc_region_growing_rgb_batch's row
 *   kernel and stages run once over it, without their label half.  Launches and waits depend on the label sweeps, not on the
 *   number of clusters or matches.
 *   ctx: any index handle, as for the other batch calls: it supplies device, stream and scratch; its cloud, tie order and kept
 *     rows are neither read nor changed.
 *   Cluster c of scene s is records offsets_s[c] .. offsets_s[c + 1] of pts_s, stride_bytes apart with x, y, z first; PCL's
 *     packed colour word of record i sits at rgb_s + i * rgb_stride_bytes.  All four arrays are in memory space `mem`,
 *     PCC_MEM_HOST or PCC_MEM_DEVICE: what pcc_region_growing_segmentation and pcc_euclidean_cluster_segmentation write as
 *     out_cluster_points / out_offsets (32-byte records: rgb = pts + 16, the same stride).  offsets_s (HOST, n_clusters_s + 1)
 *     is non-decreasing and spans fewer than 2^31 records.
 *   matches[i] (HOST): the cluster of scene 2 matched to cluster i of scene 1, or -1: pcc_cluster_matching's out_matches.
 *   out_elements[i] (HOST): {-1, -1} when matches[i] == -1; else [0] the colour-element count of cluster i of scene 1 and [1]
 *     that of cluster matches[i] of scene 2.  The count of a cluster with at most min_points finite points is 0 -- the
 *     reference's gate, size() > 10 after removeNaNFromPointCloud (src/segmentation.cpp:164-167); an empty cluster and one
 *     without a finite point fall under it.  Otherwise it is, bit for bit, the *n_clusters that pcc_index_create(cluster) +
 *     pcc_region_growing_rgb(...) give on a fresh handle with the same seven parameters.  Non-finite points take part in
 *     nothing; no point of another cluster enters a row, a segment or a segment pair.
 *   To the host cross, inside the call: what the stages of pcc_region_growing_rgb bring (three words per label sweep, the
 *     segment records, the pair list, the clusters' first segment ids) and one finite count per segmented cluster, in the first
 *     sweep's wait.  No label is downloaded.  From PCC_MEM_DEVICE no point or colour crosses in either direction; from
 *     PCC_MEM_HOST the records of the named clusters go up once, in the copy that carries the tables.
 *   Clusters above PCC_OPT_RGB_BATCH_BRUTE_MAX records, and every cluster when nr_region_neighbours > 128, take
 *     pcc_index_set_input + pcc_region_growing_rgb on a work handle kept in ctx (reused across calls, freed with ctx; same
 *     bits), one by one, straight from the device array (host memory: from what went up), their labels to device scratch.
 *   pcc_index_stats afterwards: [0] grown colour segments, [1] distinct ordered segment pairs and [7] label sweeps of the
 *     batch route; [2] points through the batch kernels, [3] points through the work handle, [4] distinct clusters segmented,
 *     [5] segmentations the deduplication saved.
 *   Refused before the handle is looked at, in this order: 1. a bad memory space; 2. null arrays (offsets_2 may be null while
 *     scene 2 has no cluster; matches and out_elements go with scene 1; a scene's pts and rgb may be null while no matched
 *     cluster of it holds a record); 3. a bad stride or alignment, by pcc_region_growing_rgb_batch's rules and messages;
 *     4. offsets that decrease (PCC_ERR_INVALID) or span 2^31 records and more (PCC_ERR_UNSUPPORTED); 5. a matches[i] outside
 *     [-1, n_clusters2) (PCC_ERR_INVALID; the message names i); 6. what pcc_region_growing_rgb refuses about thresholds and
 *     neighbour counts; 7. a null handle.  A refused call writes nothing.  n_clusters1 == 0, and a table without an entry
 *     >= 0 (out_elements is then -1 throughout), are PCC_OK without a handle or a device.  A batch route of 2^31 points and
 *     more, or one whose rows would hold 2^32 entries and more, is PCC_ERR_UNSUPPORTED: split the call. */
int pcc_match_colour_elements(pcc_index *ctx,
                              const void *pts1, const void *rgb1, const size_t *offsets1 /* HOST [n_clusters1 + 1] */, size_t n_clusters1,
                              const void *pts2, const void *rgb2, const size_t *offsets2 /* HOST [n_clusters2 + 1] */, size_t n_clusters2,
                              size_t stride_bytes, size_t rgb_stride_bytes, int mem,
                              const int32_t *matches /* HOST [n_clusters1] */, size_t min_points,
                              float distance_threshold, float point_color_threshold, float region_color_threshold,
                              uint32_t min_size, uint32_t max_size, unsigned int nr_neighbours, unsigned int nr_region_neighbours,
                              int32_t *out_elements /* HOST [n_clusters1][2] */);

/* ---- first point within a radius ----------------------------------------------------------------
 * replaces: the O(S*N) linear scan in processRIFTwithSIFT (src/comparator.cpp:696-713) that snaps
 *   every SIFT keypoint to the FIRST cloud point j (lowest index) with
 *   sqrt(pow(kx - px, 2) + pow(ky - py, 2) + pow(kz - pz, 2)) < radius  -- differences in float,
 *   squares / sum / sqrt in double, strict compare against the double radius (0.05 there).
 * idx[nq] (memory space `mem`): that lowest index, or -1 when no point qualifies. */
int pcc_first_within(pcc_index *index, const void *queries, size_t nq, size_t stride_bytes,
                     int mem, double radius, int32_t *idx);

/* ---- multi-GPU: RCCL over xGMI ---------------------------------------------
 * The path shards by independent queries: every GPU holds the whole reference cloud and its own index (one pcc_index per
 * device), queries are split into contiguous shards and searched with the calls above -- no exchange inside a search.
 * Exchanged are: the reference cloud, once (broadcast); the 17 sums of every ICP pass when the SOURCE cloud is sharded
 * (all-reduce on the handle's stream, inside the device-resident loop); SOR's statistics when the cloud's points are
 * sharded.  Clustering does not shard (global union-find): replicas only.
 * replaces: the single pcl::KdTreeFLANN / pcl::IterativeClosestPoint / pcl::StatisticalOutlierRemoval object per call site
 *   (src/comparator.cpp:564-577, 1089-1110, 1523-1541) when a node's GPUs share one cloud pair.
 * A pcc_comm is one rank of an RCCL communicator: one per (process, GPU).  librccl.so.1 is loaded when the first one is
 * made (dlopen); libpcc_nn.so does not depend on it otherwise.
 * The calls marked "collective" must be made by EVERY rank of the communicator.  A failure on ONE rank -- a shard outside
 * the cloud, an empty shard, an allocation that is refused, a cloud the root cannot index -- does not leave the others
 * waiting: before every data collective the ranks agree on one status word (all-reduce MIN), and every rank returns the
 * failing rank's code (pcc_last_error on the others: "another rank of the communicator failed").  Only a rank that never
 * makes the call (or passes no communicator) can still stall its peers, as in any RCCL program. */
typedef struct pcc_comm pcc_comm;
#define PCC_COMM_ID_BYTES 128
/* one process per GPU: rank 0 makes the id (PCC_COMM_ID_BYTES bytes), hands it to the other ranks over whatever launched
 * them, every rank then calls pcc_comm_create_rank (collective: it returns when all `world` ranks have called) */
int pcc_comm_unique_id(void *id, size_t bytes);
int pcc_comm_create_rank(const void *id, size_t bytes, int world, int rank, int device, pcc_comm **out);
/* one process driving several GPUs: out[k] is rank k on devices[k] (distinct devices).  Collective calls on these handles
 * must be issued from one thread per device (every rank blocks until the others have joined) */
int pcc_comm_create_local(const int *devices, int count, pcc_comm **out);
int pcc_comm_destroy(pcc_comm *comm);
int pcc_comm_info(const pcc_comm *comm, int *rank, int *world, int *device);
/* the reference cloud of rank `root` indexed on EVERY rank: root indexes (points, n, stride, mem) as pcc_index_create does,
 * the packed cloud (16 B per point) is broadcast once over RCCL, every other rank builds its own index over the copy
 * (0.5 ms at 10M points: cheaper than shipping the index).  Collective; points / n are read on the root only;
 * *n_out (nullable): the number of points of the cloud, on every rank. */
int pcc_index_create_broadcast(pcc_comm *comm, int root, const void *points, size_t n, size_t stride_bytes, int mem,
                               int engine, pcc_index **out, size_t *n_out);
/* pcc_icp_align with the SOURCE cloud sharded over the ranks (each rank: its shard, its handle over the same target).  Per
 * pass the 17 double sums are all-reduced (136 bytes) before the solver runs, so every rank applies the same transform;
 * fitness is the mean squared distance over ALL shards.  With one rank: pcc_icp_align's result, bit for bit.  Collective. */
int pcc_icp_align_sharded(pcc_index *index, pcc_comm *comm, const void *source_shard, size_t n, size_t stride_bytes, int mem,
                          int max_iterations, int fixed_iterations, float T[16], double *fitness, int *iterations,
                          int *converged);
/* SOR over a shard [start, start + count) of the indexed cloud: the shard's mean distances (memory space `mem`, nullable)
 * and its share of PCL's statistics -- sums[0] = sum of the means, [1] = sum of their float squares, [2] / [3] = bit
 * patterns (as doubles) of the smallest positive term of either sum.  Combine over shards with (+, +, min, min), then
 * pcc_sor_threshold (host arithmetic, no handle): *exact = 0 means PCL's in-order additions would round, i.e. the combined
 * sums need not carry PCL's last bits (pcc_sor_sharded and pcc_sor then take the sums in index order). */
int pcc_sor_partial(pcc_index *index, size_t start, size_t count, int mean_k, int mem, float *mean_dist, double sums[4]);
int pcc_sor_threshold(const double sums[4], uint64_t n_valid, int mean_k, double stddev_mult, double *threshold, int *exact);
/* pcc_sor over the ranks of `comm`: this rank filters the points [start, start + count) (the ranks' shards tile the cloud);
 * the statistics are PCL's over the WHOLE cloud (one all-reduce of the sums, one of the smallest terms, one of the kept
 * count).  mean_dist / inlier: `count` entries in memory space `mem`; *threshold, *kept_total: same on every rank. */
int pcc_sor_sharded(pcc_index *index, pcc_comm *comm, size_t start, size_t count, int mean_k, double stddev_mult, int mem,
                    float *mean_dist, uint8_t *inlier, double *threshold, size_t *kept_total);

/* ---- change detection -----------------------------------------------------------------
 * pcc_change_detection: the points of cloud B that lie in voxels cloud A leaves empty.
 * replaces: spatial_change_detection (src/comparator.cpp:54-110, called from both verdict branches of main, :1687-1698):
 *   pcl::octree::OctreePointCloudChangeDetector -- setInputCloud(A), addPointsFromInputCloud, switchBuffers,
 *   setInputCloud(B), addPointsFromInputCloud, getPointIndicesFromNewVoxels.  Restated from the published algorithm; parity
 *   with PCL 1.7 itself is not pinned.  The contract:
 * Points that take part: those whose first three floats are finite.  Non-finite points of A mark nothing, non-finite
 *   points of B are never reported.
 * The lattice: PCL grows the octree's box in whole multiples of the resolution, so the first point that takes part fixes
 *   it.  p = the first finite point of A in index order, or of B if A has none; res = resolution, eps = (double)FLT_EPSILON;
 *   per axis, in double, in this order:  mn = p - res/2;  mx = p + res/2;  side = 2*res - eps;  over = (side - (mx - mn)) / 2;
 *   a = mn - over  (PCL's first box: side 2*res - eps, centred on p).  The voxel of x is k = floor(((double)x - a) / res) per
 *   axis: IEEE double subtraction, then division, no contraction, no reciprocal.
 * Reported: a voxel is NEW if at least one finite point of B lies in it and no finite point of A does.  The result is every
 *   finite point i of B whose voxel is new and holds at least min_points_per_leaf finite points of B (PCL's default: 0).
 *   Indices come back ASCENDING.  Deviation: PCL returns them in octree traversal order, which depends on how the box
 *   happened to grow; the reference only copies them into a cloud for display, and ascending order is what every other
 *   index output of this library gives.
 * Range: the three voxel coordinates share one 64-bit key, so over the finite points of both clouds max k - min k + 1 must be
 *   at most 2^21 per axis, and every ((double)x - a) / res below 2^31 in magnitude (PCL's own limit is 2^32 voxels per axis).
 *   Both are decided in floating point before any conversion to an integer.  Beyond: PCC_ERR_UNSUPPORTED, the message names
 *   the axis and the span, *n_out = 0 and no output array is written.
 * ctx supplies device, stream and scratch, as for pcc_voxel_grid and pcc_sac_plane; the cloud it indexes is not looked at.
 * mem applies to a, b, out_index and out_records; n_out is always on the host.  out_index: n_b entries, the first *n_out are
 *   written.  out_records: NULL, or n_b * b_stride_bytes bytes: record out_index[j] of b is copied WHOLE to slot j (host memory:
 *   b must then be readable to the end of its last record).  With PCC_MEM_DEVICE the call is asynchronous on the handle's
 *   stream apart from its one read-back of (status word, count), as pcc_rift_descriptors reads its count.
 * Neither cloud has a finite point: PCC_OK, *n_out = 0.  The voxel table (open addressing, a power of two of at least
 *   2 * (n_a + n_b) slots, cleared by every call) is handle scratch; a probe that runs through all of it -- ruled out by
 *   its size -- ends the call with PCC_ERR_INTERNAL instead of waiting.
 * Refused before any device is touched, nothing written: a null a, b, out_index or n_out; a bad memory space; n_a == 0 or
 *   n_b == 0 (PCC_ERR_EMPTY); a stride below 12 or not a multiple of 4; 2^31 points or more (PCC_ERR_UNSUPPORTED); a pointer
 *   that is not 4-byte aligned; a resolution that is not positive and finite; min_points_per_leaf < 0; a null handle last. */
int pcc_change_detection(pcc_index *ctx, const void *a, size_t n_a, size_t a_stride_bytes, const void *b, size_t n_b,
                         size_t b_stride_bytes, int mem, double resolution, int min_points_per_leaf, int32_t *out_index,
                         void *out_records, size_t *n_out);

/* ---- instrumentation ------------------------------------------------------------------
 * counters of the last search on this index (host):
 *  stats[0] queries resolved by the GRID engine, [1] queries sent to the BRUTE
 *  fallback, [2] reference points valid, [3] grid cells, [4] distances evaluated by the pruned kernels (k = 1, k-NN,
 *  radius, clustering, tie flags) since the previous pcc_index_stats call, process-wide -- counted by the PROFILING build
 *  only (libpcc_nn_prof.so, `make prof`; pcc_counts_pairs() == 1), 0 in libpcc_nn.so, [5] queries flagged as tied and [6] indices changed by
 *  the FLANN walk (PCC_TIES_FLANN, last search), [7] queries the 3x3x3 cube of the pruned k = 1 kernel left open
 *  (last search that listed them: from 2M queries on, or PCC_OPT_NN1_KERNEL = 2).
 *  After pcc_rift_descriptors_batch on the handle: [0] points whose radius rows the batch kernels built, [1] points of the
 *  clouds sent through the work handle (above PCC_OPT_RIFT_BATCH_BRUTE_MAX).
 *  After pcc_fpfh_descriptors_batch on the handle: [0] points the batch kernels served, [1] points of the clusters sent
 *  through the work handle (above PCC_OPT_FPFH_BATCH_BRUTE_MAX), [2] CSRs the batch route built (0, 1 or 2).
 *  After pcc_vfh_descriptors_batch on the handle: [0] points the batch kernels served, [1] points of the clusters sent
 *  through the work handle (above PCC_OPT_VFH_BATCH_BRUTE_MAX), [2] descriptors written.
 *  After pcc_sift_keypoints_batch on the handle: [0] points that went through the batch kernels, [1] points of the clouds sent
 *  through the work handle (above PCC_OPT_SIFT_BATCH_BRUTE_MAX), [2] octave rounds the batch route ran.
 *  After pcc_cluster_descriptors on the handle: [0] dense-route points, [1] SIFT-route points, [2] octave rounds, [3] keypoints,
 *  [4] snapped points, [5] points sent through the work handle (above either batch limit).
 *  After pcc_cluster_matching on the handle: [0] searched pairs, [1] queries over all searched pairs.
 *  After pcc_region_growing_rgb on the handle: [0] grown colour segments, [1] distinct ordered segment pairs (s, t) with a row
 *  entry leading from s to t, [7] label sweeps of the growing stage.
 *  After pcc_region_growing_rgb_batch on the handle: [0] grown colour segments, [1] distinct ordered segment pairs and [7] label
 *  sweeps of the batch route (all its clouds together), [2] points that went through the batch kernels, [3] points of the
 *  clouds sent through the work handle (above PCC_OPT_RGB_BATCH_BRUTE_MAX, or nr_region_neighbours > 128).
 *  After pcc_match_colour_elements on the handle: [0], [1], [7] as after pcc_region_growing_rgb_batch, [2] points that went through
 *  the batch kernels, [3] points of the clusters sent through the work handle, [4] distinct clusters segmented (the profiling
 *  build reports its pair counter there instead), [5] segmentations the deduplication saved. */
int pcc_index_stats(const pcc_index *index, uint64_t stats[8]);
/* 1 when this library was built with the pair counter (-DPCC_COUNT_PAIRS: the profiling build), else 0 */
int pcc_counts_pairs(void);
/* test hook: the nth device allocation the library makes from now on (process-wide, nth >= 1) fails as an exhausted
 * hipMalloc does -- PCC_ERR_NOMEM from whichever call needed it; 0 disarms.  The reference maps every failure to a return
 * code (src/comparator.cpp:1123,1134,1179); this is how the tests reach the library's allocation-failure paths, the
 * collective ones above all (a rank that cannot allocate must take its peers out of the call, not leave them waiting). */
int pcc_debug_fail_alloc(int nth);
/* test hook: the blocks the library holds at this moment, process-wide and over every handle and communicator: live[0] device
 * allocations, live[1] pinned host allocations.  Counted where a block is taken and where it is given back, so the figures
 * after pcc_index_destroy equal those before the handle was made, exactly: this is how the tests see that a handle -- whatever
 * was called on it, whichever allocation was refused on the way -- gives back everything it took. */
int pcc_debug_live_buffers(uint64_t live[2]);
/* HIP-event timing of the library's own kernels, recorded on the index's stream
 * (events of another stream would not see them).  After enabling, every
 * set_input / search records events into a 64-call ring without synchronising;
 * pcc_index_timing synchronises the stream and returns the AVERAGE milliseconds
 * over the calls recorded since enabling (ms[7] = number of main-kernel samples):
 *  ms[0] main search kernel (GRID ring search, or the exhaustive kernel under
 *        ENGINE_BRUTE), ms[1] exhaustive fallback pass of the GRID engine,
 *  ms[2] whole last search call (first to last kernel), ms[3] whole last
 *  set_input/build, ms[4] query sort (GRID), ms[5..6] reserved. */
/* on: 0 off; 1 only the main search kernel (two events per call -- what a timed region can
 * afford: every recorded event costs a few microseconds of stream time); 2 full breakdown */
int pcc_index_enable_timing(pcc_index *index, int on);
int pcc_index_timing(pcc_index *index, float ms[8]);

#ifdef __cplusplus
}
#endif
#endif
