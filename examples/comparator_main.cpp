// examples/comparator_main.cpp -- an EXAMPLE of the integration INTEGRATION.md describes, not product source: the
// reference's own call sites (its two segmentation functions, its option parsing, its printed lines) re-pointed at the
// pcc:: shim, so that the drop-in claim can be exercised end to end (tests/test_cli_gpu.py).  What follows mirrors the
// reference statement by statement on purpose -- that is what "the maintainer changes the namespace and nothing else"
// looks like.  The product is include/ + pointcloudcomparator_amd/csrc/ + host/ply_io.hpp + host/report.hpp.
//
// The `./comparator [-n] [-v] [-i] [-e] scene1.ply scene2.ply` front end of the
// reference (src/comparator.cpp:1641-1705 main, :1112-1636 computeSimilarity) for the stages that sit
// on the nearest-neighbour path this repository accelerates:
//   load 2 PLY (:1119,:1130; -2 on failure) -> NaN strip (:1144-1148) -> [-i] ICP gate (:1152-1186, -1
//   when it does not converge) -> [-e] Euclidean clustering (src/segmentation.cpp:119-156) -> point /
//   cluster counts (:1199-1205) -> [-n] noise pass (:1520-1568) -> results file.
// Same flags, banner lines, section strings and exit code (always 1, :1704).  NOT part of this build
// (out of scope): the viewer (-v is accepted and ignored).  The RIFT
// descriptors of the clusters come from files (--descriptors1/2) or, with --rift, from pcc::processRIFT (:590-684), dense
// for every cluster; with --sift as well, clusters above 700 points go through SIFT keypoints first as in the reference
// (pcc::processRIFTwithSIFT, :686-822, chosen at :1228-1231 and :1264-1265).  Both segmentation paths run: region growing (default, src/segmentation.cpp:218-327) and
// Euclidean clustering (-e, :64-156), each behind the VoxelGrid the reference applies first.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <algorithm>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "pcc/comparator_nn.hpp"
#include "pcc/multi_device.hpp"
#include "pcc/rift.hpp"
#include "pcc/sift.hpp"
#include "pcc/descriptors.hpp"
#include "pcc/octree.hpp"
#include "ply_io.hpp"
#include "report.hpp"

using namespace pcc;

static bool seeClusters = false, noise = false, euclidean = false, icp = false;
// not in the reference: --gpus N (the two clouds are segmented / filtered as replicas on two devices),
// --descriptors1/2 FILE (precomputed RIFT32 descriptors per cluster: the descriptor pipeline itself is out of scope),
// --dump-clusters PREFIX (the clusters as PLY files, so that descriptors can be computed for them elsewhere),
// --rift (clusters of a scene without a descriptor file get their descriptors from pcc::processRIFT),
// --sift (with --rift: clusters above 700 points take pcc::processRIFTwithSIFT, the reference's own choice),
// --rift-loop (with --rift: one call per cluster as in the reference, :1224-1272, instead of one pcc::processRIFTBatch for all),
// --descriptors-device (with --rift: the whole descriptor loop of both scenes in one pcc::clusterDescriptors call),
// --dump-descriptors PREFIX (the descriptors in use, as PREFIX_<scene>.txt in the format --descriptors1/2 read),
// --descriptor-dims N (the bins of a descriptor the cluster matching searches on),
// --rgb-device (the colour segmentation of matched clusters, :1456-1495, as one pcc_region_growing_rgb call each: same report),
// --rgb-batch (the same for the clusters of ALL accepted matches in one pcc_region_growing_rgb_batch call: same report),
// --colours-device (the colour-element counts of ALL accepted matches from one pcc_match_colour_elements call: same report)
static int n_gpus = 1, descriptor_dims = 3;
static bool rgb_device = false, rgb_batch = false, colours_device = false;
// --planes-device (with -e): the plane-removal loop runs in one library call (pcc_plane_removal through removePlanes): same lines
static bool planes_device = false;
// --segment-device (without -e): the whole default segmentation runs in one library call (pcc_region_growing_segmentation through
// regionGrowingSegmentation): same lines, same clusters
static bool segment_device = false;
// --euclidean-device (with -e): the whole -e segmentation runs in one library call (pcc_euclidean_cluster_segmentation through
// euclideanClusterSegmentation): same lines, same clusters
static bool euclidean_device = false;
static bool rift = false, sift = false, rift_loop = false;
// --descriptors-device (with --rift): the descriptor loop over the clusters of BOTH scenes runs in one library call
// (pcc_cluster_descriptors through clusterDescriptors; without --sift its gate is "never"): same lines, same descriptors
static bool descriptors_device = false;
// --matching-device: the cluster-matching loop (:1296-1366) runs in one library call (pcc_cluster_matching through matchClusters):
// same lines, same matches
static bool matching_device = false;
static std::string descriptors_path[2], dump_prefix, dump_descriptors_prefix;
// --changes RES: after verdict 1 or 2 the reference's spatial_change_detection (:54-110, called at :1687-1698 with a resolution of
// 32) runs at resolution RES: its sentence and the number of points of the richer cloud in voxels the other leaves empty;
// --dump-changes FILE.ply: those points, with their colours
static double changes_resolution = 0;
static std::string dump_changes_path;

static void printUsage() {
    std::cout << "\n\nUsage: [options] </pathToScene1.ply> </pathToScene2.ply>\n\n"
              << "Options:\n" << "-------------------------------------------\n"
              << "-n activate noise analysis \n"
              << "-v activate visualization of clusters and matches\n"
              << "-i activate ICP algorithm to know if both point clouds are enough similar \n"
              << "-e activate euclidean cluster segmentation as main segmentation algorithm; region growing segmentation is default\n"
              << "-h show this help\n"
              << "--gpus N           (this build) N devices: ICP source sharded, the two clouds segmented / filtered as replicas\n"
              << "--descriptors1 F   (this build) precomputed RIFT32 descriptors of the clusters of scene 1\n"
              << "--descriptors2 F   (this build) ... of scene 2\n"
              << "--dump-clusters P  (this build) write the clusters as P_<scene>_<cluster>.ply\n"
              << "--rift             (this build) RIFT descriptors of every cluster of a scene without a descriptor file are computed\n"
              << "                   (processRIFT: normals 0.03, intensity gradient 0.03, RIFT 0.05, 4 x 8 bins), DENSE for every\n"
              << "                   cluster: the reference's SIFT keypoint stage for clusters above 700 points is not part of --rift alone\n"
              << "--sift             (this build, with --rift) clusters above 700 points take the reference's processRIFTwithSIFT instead:\n"
              << "                   SIFT keypoints (scales 0.005, 5, 5; minimum contrast 0.001), each snapped to the first cluster point\n"
              << "                   within 0.05, RIFT descriptors of the snapped cloud\n"
              << "--rift-loop        (this build, with --rift) one library call per cluster, as the reference's loop does; without it\n"
              << "                   every cluster of both scenes goes through ONE processRIFTBatch call (same descriptors)\n"
              << "--descriptors-device  (this build, with --rift) the descriptor loop -- SIFT keypoints and their snap for the clusters\n"
              << "                   above 700 points (with --sift), RIFT for every cluster -- runs in ONE library call for both scenes\n"
              << "                   (pcc_cluster_descriptors: keypoints and snapped clouds stay on the GPU): the same descriptors\n"
              << "--dump-descriptors P  (this build) write the descriptors in use as P_<scene>.txt (the format of --descriptors1/2)\n"
              << "--descriptor-dims N  (this build) the cluster matching searches on the first N bins of every descriptor, 1 ... 32\n"
              << "                   (default 3: what the reference's PCL does with a 32-bin histogram -- recalled, not re-checked;\n"
              << "                   32 matches on the whole histogram; exact ties then go to the lowest index)\n"
              << "--matching-device  (this build) the cluster-matching loop -- three nearest centroids, the two gates, the descriptor\n"
              << "                   search of every gated pair, the acceptance rule -- runs in ONE library call (pcc_cluster_matching:\n"
              << "                   every cluster packed once, only the correspondence counts come back): the same lines, the same matches\n"
              << "--rgb-device       (this build) the colour segmentation of every matched cluster runs in the library, rows and growing on\n"
              << "                   the GPU (pcc_region_growing_rgb), instead of on the host over downloaded rows: the same report\n"
              << "--rgb-batch        (this build) the colour segmentations of ALL accepted matches run in one library call\n"
              << "                   (pcc_region_growing_rgb_batch) before the match sections are written: the same report\n"
              << "--colours-device   (this build) the colour-element counts of ALL accepted matches come from one library call\n"
              << "                   (pcc_match_colour_elements: the clusters of both scenes and the match table go in, every distinct\n"
              << "                   cluster is segmented once, only the counts come back): the same report\n"
              << "--planes-device    (this build, with -e) the plane-removal loop in front of the clustering runs in ONE library call\n"
              << "                   (pcc_plane_removal: the cloud uploaded once, compacted on the GPU) instead of one call and one\n"
              << "                   host compaction per plane: the same lines, the same clusters\n"
              << "--segment-device   (this build, without -e) the default segmentation -- voxel grid, normals, region growing, one cloud\n"
              << "                   per cluster -- runs in ONE library call (pcc_region_growing_segmentation: the filtered cloud, its\n"
              << "                   index, normals and labels stay on the GPU): the same lines, the same clusters; ignored with -e\n"
              << "--euclidean-device (this build, with -e) the -e segmentation -- voxel grid, plane removal, Euclidean clustering, one\n"
              << "                   cloud per cluster -- runs in ONE library call (pcc_euclidean_cluster_segmentation: the filtered\n"
              << "                   cloud, what remains after the planes, its index and labels stay on the GPU): the same lines, the\n"
              << "                   same clusters; ignored without -e\n"
              << "--results F        (this build) results file (default ../../PointCloudComparatorResults/results.txt)\n"
              << "--changes RES      (this build) after the verdict \"first\" or \"second\" the reference's spatial_change_detection runs at a\n"
              << "                   voxel resolution of RES (pcc_change_detection): the sentence of that branch and the number of points\n"
              << "                   of the richer cloud in voxels the other cloud leaves empty; nothing after \"same information\"\n"
              << "--dump-changes F.ply  (this build, with --changes) those points, with their colours, as a PLY file\n" << "\n\n";
}

// src/segmentation.cpp:64-156 euclidean_cluster_segmentation: VoxelGrid 0.025 (:69-76) -> RANSAC plane
// removal until <= 30 % of the points remain (:79-117) -> KdTree + EuclideanClusterExtraction (:119-156)
static std::vector<PointCloud<PointXYZRGB>::Ptr> euclidean_cluster_segmentation(const PointCloud<PointXYZRGB>::Ptr& point_cloud_ptr) {
    if (euclidean_device) {
        RemovedPlanes planes;
        size_t n_filtered = 0;
        std::vector<PointCloud<PointXYZRGB>::Ptr> found = euclideanClusterSegmentation<PointXYZRGB>(
            point_cloud_ptr, 0.025f, 0.3, 100, 0.02, true, 0.05, 100, 250000, planes, nullptr, &n_filtered);
        std::cout << "PointCloud after filtering has: " << n_filtered << " data points." << std::endl;
        for (std::uint32_t size : planes.sizes)
            std::cout << "PointCloud representing the planar component: " << size << " data points." << std::endl;
        if (planes.ended_without_model) std::cout << "Could not estimate a planar model for the given dataset." << std::endl;
        for (const PointCloud<PointXYZRGB>::Ptr& c : found)
            std::cout << "PointCloud representing the Cluster: " << c->points.size() << " data points." << std::endl;
        return found;
    }
    VoxelGrid<PointXYZRGB> vg;
    PointCloud<PointXYZRGB>::Ptr cloud_filtered(new PointCloud<PointXYZRGB>);
    vg.setInputCloud(point_cloud_ptr);
    vg.setLeafSize(0.025f, 0.025f, 0.025f);
    vg.filter(*cloud_filtered);
    std::cout << "PointCloud after filtering has: " << cloud_filtered->points.size() << " data points." << std::endl;
    SACSegmentation<PointXYZRGB> seg;
    std::shared_ptr<PointIndices> inliers(new PointIndices);
    ModelCoefficients coefficients;
    PointCloud<PointXYZRGB>::Ptr cloud_plane(new PointCloud<PointXYZRGB>), cloud_f(new PointCloud<PointXYZRGB>);
    seg.setOptimizeCoefficients(true);
    seg.setModelType(SACMODEL_PLANE);
    seg.setMethodType(SAC_RANSAC);
    seg.setMaxIterations(100);
    seg.setDistanceThreshold(0.02);
    const int nr_points = (int)cloud_filtered->points.size();
    if (planes_device) {
        RemovedPlanes planes;
        cloud_filtered = removePlanes<PointXYZRGB>(cloud_filtered, planes, 0.3, 100, 0.02, true);
        for (std::uint32_t size : planes.sizes)
            std::cout << "PointCloud representing the planar component: " << size << " data points." << std::endl;
        if (planes.ended_without_model) std::cout << "Could not estimate a planar model for the given dataset." << std::endl;
    } else
    while (cloud_filtered->points.size() > 0.3 * nr_points) {
        seg.setInputCloud(cloud_filtered);
        seg.segment(*inliers, coefficients);
        if (inliers->indices.size() == 0) {
            std::cout << "Could not estimate a planar model for the given dataset." << std::endl;
            break;
        }
        ExtractIndices<PointXYZRGB> extract;
        extract.setInputCloud(cloud_filtered);
        extract.setIndices(inliers);
        extract.setNegative(false);
        extract.filter(*cloud_plane);
        std::cout << "PointCloud representing the planar component: " << cloud_plane->points.size() << " data points." << std::endl;
        extract.setNegative(true);
        extract.filter(*cloud_f);
        // the reference assigns *cloud_filtered = *cloud_f; a fresh cloud keeps the pointer-keyed caches honest
        cloud_filtered.reset(new PointCloud<PointXYZRGB>(*cloud_f));
    }
    search::KdTree<PointXYZRGB>::Ptr tree(new search::KdTree<PointXYZRGB>);
    tree->setInputCloud(cloud_filtered);
    std::vector<PointIndices> cluster_indices;
    EuclideanClusterExtraction<PointXYZRGB> ec;
    ec.setClusterTolerance(0.05);
    ec.setMinClusterSize(100);
    ec.setMaxClusterSize(250000);
    ec.setSearchMethod(tree);
    ec.setInputCloud(cloud_filtered);
    ec.extract(cluster_indices);
    std::vector<PointCloud<PointXYZRGB>::Ptr> clusters_pcl;
    for (const PointIndices& it : cluster_indices) {
        PointCloud<PointXYZRGB>::Ptr cloud_cluster(new PointCloud<PointXYZRGB>);
        for (int pit : it.indices) cloud_cluster->points.push_back(cloud_filtered->points[pit]);
        cloud_cluster->width = (std::uint32_t)cloud_cluster->points.size();
        cloud_cluster->height = 1;
        cloud_cluster->is_dense = true;
        std::cout << "PointCloud representing the Cluster: " << cloud_cluster->points.size() << " data points." << std::endl;
        clusters_pcl.push_back(cloud_cluster);
    }
    return clusters_pcl;
}

// src/segmentation.cpp:218-327 region_growing_segmentation: VoxelGrid 0.025 -> NormalEstimation K = 50 ->
// RegionGrowing (50..1000000 points, 100 neighbours, 3 degrees, curvature 1)
static std::vector<PointCloud<PointXYZRGB>::Ptr> region_growing_segmentation(const PointCloud<PointXYZRGB>::Ptr& point_cloud_ptr) {
    if (segment_device) {
        PointCloud<PointXYZRGB>::Ptr filtered;
        std::vector<PointCloud<PointXYZRGB>::Ptr> found = regionGrowingSegmentation<PointXYZRGB>(
            point_cloud_ptr, 0.025f, 50, 100, (float)(3.0 / 180.0 * M_PI), 1.0f, 50, 1000000, &filtered);
        std::cout << "PointCloud after filtering has: " << filtered->points.size() << " data points." << std::endl;
        std::cout << "Number of clusters is equal to " << found.size() << std::endl;
        return found;
    }
    VoxelGrid<PointXYZRGB> vg;
    PointCloud<PointXYZRGB>::Ptr cloud_filtered(new PointCloud<PointXYZRGB>);
    vg.setInputCloud(point_cloud_ptr);
    vg.setLeafSize(0.025f, 0.025f, 0.025f);
    vg.filter(*cloud_filtered);
    std::cout << "PointCloud after filtering has: " << cloud_filtered->points.size() << " data points." << std::endl;
    search::KdTree<PointXYZRGB>::Ptr tree(new search::KdTree<PointXYZRGB>);
    tree->setOption(PCC_OPT_KNN_CACHE_K, 100);  // normals (50) and region growing (100) share one 100-neighbour search
    PointCloud<Normal>::Ptr normals(new PointCloud<Normal>);
    NormalEstimation<PointXYZRGB, Normal> normal_estimator;
    normal_estimator.setSearchMethod(tree);
    normal_estimator.setInputCloud(cloud_filtered);
    normal_estimator.setKSearch(50);
    normal_estimator.compute(*normals);
    RegionGrowing<PointXYZRGB, Normal> reg;
    reg.setMinClusterSize(50);
    reg.setMaxClusterSize(1000000);
    reg.setSearchMethod(tree);
    reg.setNumberOfNeighbours(100);
    reg.setInputCloud(cloud_filtered);
    reg.setInputNormals(normals);
    reg.setSmoothnessThreshold(3.0 / 180.0 * M_PI);
    reg.setCurvatureThreshold(1);
    std::vector<PointIndices> clusters;
    reg.extract(clusters);
    std::cout << "Number of clusters is equal to " << clusters.size() << std::endl;
    std::vector<PointCloud<PointXYZRGB>::Ptr> clusters_pcl;
    for (const PointIndices& c : clusters) {
        PointCloud<PointXYZRGB>::Ptr cloud_cluster(new PointCloud<PointXYZRGB>);
        for (int j : c.indices) cloud_cluster->points.push_back(cloud_filtered->points[j]);
        cloud_cluster->width = (std::uint32_t)cloud_cluster->points.size();
        cloud_cluster->height = 1;
        cloud_cluster->is_dense = true;
        clusters_pcl.push_back(cloud_cluster);
    }
    return clusters_pcl;
}

// src/comparator.cpp:54-110 spatial_change_detection: both files loaded again (as they are: the indices are the files'), the points
// of cloudB in voxels cloudA leaves empty; the reference shows them in a viewer, here their number is printed
static void spatial_change_detection(const std::string& filename, const std::string& filename2) {
    PointCloud<PointXYZRGB>::Ptr cloudA(new PointCloud<PointXYZRGB>), cloudB(new PointCloud<PointXYZRGB>);
    if (io::loadPLYFile(filename, *cloudA) == -1) { std::cerr << "Was not able to open file \"" << filename << "\".\n"; return; }
    if (io::loadPLYFile(filename2, *cloudB) == -1) { std::cerr << "Was not able to open file \"" << filename2 << "\".\n"; return; }
    const PointCloud<PointXYZRGB>::Ptr cloudDiff = spatialChangeDetection<PointXYZRGB>(cloudA, cloudB, changes_resolution);
    std::cout << cloudDiff->points.size() << " points" << std::endl;
    if (!dump_changes_path.empty() && io::savePLYFileBinary(dump_changes_path, *cloudDiff) == -1)
        std::cerr << "Was not able to write file \"" << dump_changes_path << "\".\n";
}

static double computeSimilarity(const std::string& file1, const std::string& file2, const std::string& results_path) {
    PointCloud<PointXYZRGB>::Ptr point_cloud1_ptr(new PointCloud<PointXYZRGB>), point_cloud2_ptr(new PointCloud<PointXYZRGB>);
    if (io::loadPLYFile(file1, *point_cloud1_ptr) == -1) {
        std::cerr << "Was not able to open file \"" << file1 << "\".\n";
        return -2;
    }
    if (io::loadPLYFile(file2, *point_cloud2_ptr) == -1) {
        std::cerr << "Was not able to open file \"" << file2 << "\".\n";
        return -2;
    }
    report::Writer out(results_path);
    std::ofstream& myfile = out.file();
    out.header(file1, file2);
    std::vector<int> indices2;
    io::removeNaNFromPointCloud(*point_cloud1_ptr, indices2);
    io::removeNaNFromPointCloud(*point_cloud2_ptr, indices2);

    if (icp) {
        // --gpus N: the source cloud of the ICP gate is sharded over the devices (17 sums all-reduced per pass over RCCL)
        std::vector<int> icp_devices;
        for (int d = 0; d < std::min(n_gpus, deviceCount()); ++d) icp_devices.push_back(d);
        const bool icp_ok = icp_devices.size() > 1 ? performICP(point_cloud1_ptr, point_cloud2_ptr, icp_devices)
                                                   : performICP(point_cloud1_ptr, point_cloud2_ptr);
        if (!icp_ok) {
            myfile << "----------------------------" << "\n\n";
            myfile << "ICP could not match the point clouds. They are probably too dissimilar.\n Brief comparison:\n";
            const size_t n1 = point_cloud1_ptr->points.size(), n2 = point_cloud2_ptr->points.size();
            if (n1 > n2) {
                std::cout << "PCL1 has more points: " << n1 << " over: " << n2 << std::endl;
                myfile << "PCL1 has more points: " << n1 << " over: " << n2 << "\n";
            } else if (n2 > n1) {
                std::cout << "PCL2 has more points: " << n2 << " over: " << n1 << std::endl;
                myfile << "PCL2 has more points: " << n2 << " over: " << n1 << "\n";
            } else {
                std::cout << "Both PCL have the same number of points" << std::endl;
                myfile << "Both PCL have the same number of points" << "\n";
            }
            myfile.close();
            return -1;
        } else {
            std::cout << "ICP has converged. Point clouds segmentation is as follows" << std::endl;
            myfile << "ICP has converged. Point clouds segmentation is as follows: \n";
        }
    }

    // the two clouds are independent until the cluster matching: replicas, one device each when there are several
    // (clustering itself does not shard).  With one device the two jobs run one after the other, in
    // the reference's order, so its printed lines keep their order.
    std::vector<int> devices;
    for (int d = 0; d < std::max(1, std::min(n_gpus, deviceCount())); ++d) devices.push_back(d);
    std::vector<PointCloud<PointXYZRGB>::Ptr> clusters[2];
    const PointCloud<PointXYZRGB>::Ptr clouds[2] = {point_cloud1_ptr, point_cloud2_ptr};
    auto segment = [&](int k) { clusters[k] = euclidean ? euclidean_cluster_segmentation(clouds[k]) : region_growing_segmentation(clouds[k]); };
    if (devices.size() > 1) onDevices(2, devices, segment);
    else { segment(0); segment(1); }
    std::vector<PointCloud<PointXYZRGB>::Ptr>&clusters_pcl_1 = clusters[0], &clusters_pcl_2 = clusters[1];

    report::Writer& w = out;
    w.counts(point_cloud1_ptr->points.size(), point_cloud2_ptr->points.size(), clusters_pcl_1.size(), clusters_pcl_2.size());
    if (!dump_prefix.empty())
        for (int k = 0; k < 2; ++k)
            for (size_t j = 0; j < clusters[k].size(); ++j) {
                std::ostringstream name;
                name << dump_prefix << "_" << k + 1 << "_" << j << ".ply";
                io::savePLYFileBinary(name.str(), *clusters[k][j]);
            }

    // descriptors per cluster: from files, computed (--rift), or none
    std::vector<report::DescPtr> des[2];
    bool have_descriptors = true;
    std::vector<PointCloud<PointXYZRGB>::Ptr> batch_clouds;  // --rift without --rift-loop: every cluster of both scenes that needs descriptors
    bool batch_scene[2] = {false, false};
    // --sift without --rift-loop: the clusters above 700 points of both scenes (reference :1228-1231, :1264-1265) through ONE
    // siftSnappedCloudBatch call; the loop below takes the snapped clouds in the order it meets their clusters
    std::vector<PointCloud<PointXYZRGB>::Ptr> sift_snapped;
    std::vector<size_t> sift_found;
    size_t sift_at = 0;
    if (rift && descriptors_device) {
        // every cluster of the scenes without a descriptor file through ONE clusterDescriptors call
        std::vector<PointCloud<PointXYZRGB>::Ptr> all;
        for (int k = 0; k < 2; ++k)
            if (descriptors_path[k].empty()) all.insert(all.end(), clusters[k].begin(), clusters[k].end());
        const ClusterDescriptors cd = clusterDescriptors(all, sift ? SIFT_ABOVE : SIFT_NEVER);
        size_t at = 0;
        for (int k = 0; k < 2; ++k) {
            if (!descriptors_path[k].empty()) continue;
            for (const PointCloud<PointXYZRGB>::Ptr& c : clusters[k]) {
                if (sift && c->points.size() > SIFT_ABOVE) std::cout << "Computed " << cd.n_keypoints[at] << " SIFT Keypoints\n";  // reference :467
                des[k].push_back(cd.descriptors[at++]);
            }
        }
    }
    if (rift && sift && !rift_loop && !descriptors_device) {
        std::vector<PointCloud<PointXYZRGB>::Ptr> large;
        for (int k = 0; k < 2; ++k)
            if (descriptors_path[k].empty())
                for (const PointCloud<PointXYZRGB>::Ptr& c : clusters[k])
                    if (c->points.size() > 700) large.push_back(c);
        if (!large.empty()) sift_snapped = siftSnappedCloudBatch(large, &sift_found);
    }
    for (int k = 0; k < 2; ++k) {
        if (descriptors_path[k].empty() && rift && descriptors_device) {
            // (filled above)
        } else if (descriptors_path[k].empty() && rift && !rift_loop) {
            // the clouds the RIFT pipeline runs over, in cluster order; one processRIFTBatch call for both scenes below
            for (const PointCloud<PointXYZRGB>::Ptr& c : clusters[k]) {
                if (sift && c->points.size() > 700) {
                    batch_clouds.push_back(sift_snapped[sift_at]);
                    std::cout << "Computed " << sift_found[sift_at++] << " SIFT Keypoints\n";  // reference :467
                } else {
                    batch_clouds.push_back(c);
                }
            }
            batch_scene[k] = true;
        } else if (descriptors_path[k].empty() && rift) {
            for (const PointCloud<PointXYZRGB>::Ptr& c : clusters[k]) {
                if (sift && c->points.size() > 700) {  // reference :1228-1231, :1264-1265
                    size_t n_keypoints = 0;
                    des[k].push_back(processRIFTwithSIFT(c, nullptr, &n_keypoints));
                    std::cout << "Computed " << n_keypoints << " SIFT Keypoints\n";  // reference :467
                } else {
                    des[k].push_back(processRIFT(c));
                }
            }
        } else if (descriptors_path[k].empty()) {
            have_descriptors = false;
            des[k].assign(clusters[k].size(), report::DescPtr());
            for (report::DescPtr& d : des[k]) d.reset(new PointCloud<RIFT32>);
        } else if (!report::loadDescriptors(descriptors_path[k], clusters[k].size(), des[k])) {
            std::cerr << "Was not able to read descriptors \"" << descriptors_path[k] << "\".\n";
            return -2;
        }
    }
    if (!batch_clouds.empty()) {
        const std::vector<PointCloud<RIFT32>::Ptr> batch = processRIFTBatch(batch_clouds);
        size_t at = 0;
        for (int k = 0; k < 2; ++k)
            if (batch_scene[k])
                for (size_t j = 0; j < clusters[k].size(); ++j) des[k].push_back(batch[at++]);
    }
    if (!dump_descriptors_prefix.empty())
        for (int k = 0; k < 2; ++k) {
            std::ostringstream name;
            name << dump_descriptors_prefix << "_" << k + 1 << ".txt";
            std::ofstream df(name.str().c_str());
            df.precision(9);
            df << "pcc_descriptors 1\n";
            for (size_t j = 0; j < des[k].size(); ++j) {
                df << "cluster " << j << " " << des[k][j]->size() << "\n";
                for (const RIFT32& d : des[k][j]->points) {
                    for (int b = 0; b < 32; ++b) df << (b ? " " : "") << d.histogram[b];
                    df << "\n";
                }
            }
        }
    std::vector<int> matches;
    const report::Scores scores = report::clusterSections(w, clusters_pcl_1, clusters_pcl_2, des[0], des[1], matches, descriptor_dims, rgb_device, rgb_batch,
                                                          matching_device, colours_device);

    if (noise) {
        PointCloud<PointXYZRGB> nonoise[2];
        auto filter = [&](int k) {
            StatisticalOutlierRemoval<PointXYZRGB> sor;
            sor.setInputCloud(clouds[k]); sor.setMeanK(50); sor.setStddevMulThresh(1.5); sor.filter(nonoise[k]);
        };
        if (devices.size() > 1) onDevices(2, devices, filter);
        else { filter(0); filter(1); }
        // size_t integer division, as in the reference (:1533-1535): the ratio is always 0
        double noise1 = (point_cloud1_ptr->points.size() - nonoise[0].points.size()) / point_cloud1_ptr->points.size();
        double noise2 = (point_cloud2_ptr->points.size() - nonoise[1].points.size()) / point_cloud2_ptr->points.size();
        std::cout << "Noise pass removed " << point_cloud1_ptr->points.size() - nonoise[0].points.size() << " / "
                  << point_cloud2_ptr->points.size() - nonoise[1].points.size() << " points" << std::endl;
        myfile << "----------------------------------------\n Noise analysis: \n";
        if (noise1 > noise2) {
            std::cout << "PCL1 has more noisy points: (%) " << noise1 * 100 << " over: (%) " << noise2 * 100 << std::endl;
            myfile << "\tPCL1 has more noisy points: (%) " << noise1 * 100 << " over: (%) " << noise2 * 100 << "\n";
        } else if (noise1 < noise2) {
            std::cout << "PCL2 has more noisy points: (%) " << noise2 * 100 << " over: (%) " << noise1 * 100 << std::endl;
            myfile << "\tPCL2 has more noisy points: (%) " << noise2 * 100 << " over: (%) " << noise1 * 100 << "\n";
        } else {
            std::cout << "Both pcl have the same percentage of noisy points: " << noise1 * 100 << std::endl;
            myfile << "Both pcl have the same percentage of noisy points: " << noise1 * 100 << "\n";
        }
    }
    const int verdict = report::scoreSections(w, scores, clusters_pcl_2.size());
    if (!have_descriptors) {
        // nothing was scored: saying "same information" would report a comparison that never happened
        myfile << "\n(no descriptor files given: clusters could not be matched, no verdict)\n";
        w.close();
        return -3;
    }
    w.close();
    return verdict;
}

int main(int argc, char** argv) {
    std::cout << "------------------------------------" << std::endl;
    std::vector<std::string> plys;
    std::string results_path = "../../PointCloudComparatorResults/results.txt";  // reference :1138
    bool help = false;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "-h") help = true;
        else if (a == "-v") seeClusters = true;
        else if (a == "-n") noise = true;
        else if (a == "-i") icp = true;
        else if (a == "-e") euclidean = true;
        else if (a == "--results" && i + 1 < argc) results_path = argv[++i];
        else if (a == "--gpus" && i + 1 < argc) n_gpus = std::atoi(argv[++i]);
        else if (a == "--descriptors1" && i + 1 < argc) descriptors_path[0] = argv[++i];
        else if (a == "--descriptors2" && i + 1 < argc) descriptors_path[1] = argv[++i];
        else if (a == "--dump-clusters" && i + 1 < argc) dump_prefix = argv[++i];
        else if (a == "--rift") rift = true;
        else if (a == "--sift") sift = true;
        else if (a == "--rift-loop") rift_loop = true;
        else if (a == "--descriptors-device") descriptors_device = true;
        else if (a == "--dump-descriptors" && i + 1 < argc) dump_descriptors_prefix = argv[++i];
        else if (a == "--descriptor-dims" && i + 1 < argc) descriptor_dims = std::atoi(argv[++i]);
        else if (a == "--matching-device") matching_device = true;
        else if (a == "--rgb-device") rgb_device = true;
        else if (a == "--rgb-batch") rgb_batch = true;
        else if (a == "--colours-device") colours_device = true;
        else if (a == "--planes-device") planes_device = true;
        else if (a == "--segment-device") segment_device = true;
        else if (a == "--euclidean-device") euclidean_device = true;
        else if (a == "--changes" && i + 1 < argc) changes_resolution = std::atof(argv[++i]);
        else if (a == "--dump-changes" && i + 1 < argc) dump_changes_path = argv[++i];
        else if (a.size() > 4 && a.substr(a.size() - 4) == ".ply") plys.push_back(a);
    }
    if (help) { printUsage(); return 1; }
    if (sift && !rift) { std::cerr << "--sift needs --rift\n"; printUsage(); return 1; }
    if (descriptors_device && !rift) { std::cerr << "--descriptors-device needs --rift\n"; printUsage(); return 1; }
    if (descriptor_dims < 1 || descriptor_dims > 32) { std::cerr << "--descriptor-dims takes 1 ... 32\n"; printUsage(); return 1; }
    std::cout << (seeClusters ? "Visualization of clusters is on." : "Visualization of clusters is off.") << std::endl;
    std::cout << (noise ? "Noise analysis is on." : "Noise analysis is off.") << std::endl;
    std::cout << (icp ? "ICP matching pre-comparison is on." : "ICP matching pre-comparison is off.") << std::endl;
    if (euclidean) std::cout << "Euclidean cluster segmentation was selected as main segmentation algorithm." << std::endl;
    else std::cout << "Region growing segmentation was selected (default) as main segmentation algorithm." << std::endl;
    std::cout << "------------------------------------" << std::endl;
    if (plys.size() < 2) { printUsage(); return 1; }  // the reference dereferences blindly (:1130); we print the usage
    double similarity = -3;
    try {
        similarity = computeSimilarity(plys[0], plys[1], results_path);
    } catch (const std::exception& e) {  // pcc::Error, and whatever a broken input makes the standard library throw
        std::cerr << e.what() << std::endl;
    }
    std::cout << "--------------------------------\n" << std::endl;
    const bool changes = changes_resolution > 0 && (similarity == 1 || similarity == 2);
    if (similarity == 1) std::cout << "The first point cloud has more information" << std::endl;
    else if (similarity == 2) std::cout << "The second point cloud has more information" << std::endl;
    if (changes) {
        // reference :1687-1698: the richer cloud is cloudB of spatial_change_detection
        std::cout << (similarity == 1 ? "Points that are in the first pcl, that are not in the other:"
                                      : "Points that are in the second pcl, that are not in the other:") << std::endl;
        try {
            if (similarity == 1) spatial_change_detection(plys[1], plys[0]);
            else spatial_change_detection(plys[0], plys[1]);
        } catch (const std::exception& e) {
            std::cerr << e.what() << std::endl;
        }
    }
    else if (similarity == 0) std::cout << "Both point clouds have the same information" << std::endl;
    else if (similarity == -3) std::cout << "No descriptor files were given (--descriptors1/2): clusters were not matched, no verdict" << std::endl;
    std::cout << "--------------------------------\n" << std::endl;
    return 1;  // reference :1704
}
