# Build of libpcc_nn (gfx950 HIP kernels + C-ABI), the CPU oracle and helper tools.
# hipcc cross-compiles gfx950 without a GPU.  -ffp-contract=off everywhere: the
# distance arithmetic must round like FLANN's L2_Simple (no FMA).
HIPCC      ?= /opt/rocm/bin/hipcc
CC         ?= gcc
CXX        ?= g++
ARCH       ?= gfx950
HIPFLAGS   ?= --offload-arch=$(ARCH) -O3 -ffp-contract=off -fno-slp-vectorize -std=c++17 -fPIC -Iinclude -Ipointcloudcomparator_amd/csrc
CSRC       := pointcloudcomparator_amd/csrc
LIBDIR     := pointcloudcomparator_amd/lib
HIP_SRCS   := $(CSRC)/api.hip $(CSRC)/pack.hip $(CSRC)/nn1_brute.hip $(CSRC)/grid.hip $(CSRC)/cellsort.hip $(wildcard $(CSRC)/knn.hip $(CSRC)/cluster.hip $(CSRC)/icp.hip $(CSRC)/voxel.hip $(CSRC)/normals.hip $(CSRC)/region.hip $(CSRC)/region_rgb.hip $(CSRC)/region_rgb_batch.hip $(CSRC)/sac.hip $(CSRC)/flann_order.hip $(CSRC)/cellsort_mp.hip $(CSRC)/comm.hip $(CSRC)/small.hip $(CSRC)/match_batch.hip $(CSRC)/match_dims.hip $(CSRC)/match_fpfh.hip $(CSRC)/rift.hip $(CSRC)/fpfh.hip $(CSRC)/range_batch.hip $(CSRC)/fpfh_batch.hip $(CSRC)/vfh.hip $(CSRC)/vfh_batch.hip $(CSRC)/shot.hip $(CSRC)/sift.hip $(CSRC)/rift_batch.hip $(CSRC)/sift_batch.hip $(CSRC)/cluster_desc.hip $(CSRC)/cluster_match.hip $(CSRC)/match_colour.hip $(CSRC)/sor.hip $(CSRC)/segment.hip $(CSRC)/ground.hip $(CSRC)/change.hip)
HDRS       := $(wildcard $(CSRC)/*.hpp) include/pcc_nn.h
HIP_OBJS   := $(patsubst $(CSRC)/%.hip,build/%.o,$(HIP_SRCS))

all: lib oracle hosttest cli prof

lib: $(LIBDIR)/libpcc_nn.so
# the profiling build: same sources with the pair counter compiled in (pcc_index_stats[4]); never the timed library
prof: $(LIBDIR)/libpcc_nn_prof.so
PROF_OBJS  := $(patsubst $(CSRC)/%.hip,build/prof/%.o,$(HIP_SRCS))
build/prof/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p build/prof
	$(HIPCC) $(HIPFLAGS) -DPCC_COUNT_PAIRS $(EXTRA_HIPFLAGS) -c $< -o $@
$(LIBDIR)/libpcc_nn_prof.so: $(PROF_OBJS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(PROF_OBJS) -ldl
oracle: oracle/_build/libpcc_oracle.so
ubench: build/ubench_valu build/ubench_gather build/ubench_scatter
hosttest: build/test_host_mirror build/test_lane_ops build/test_report build/test_libm build/test_match_batch build/test_acosf build/rift_host build/rift_driver build/test_expf build/sift_host build/sift_driver build/test_rift_batch_plan build/rift_batch_driver build/test_match_dims_plan build/match_dims_driver build/test_rgb_merge build/test_sift_batch_plan build/sift_batch_driver build/test_device_math build/test_rgb_batch_split build/test_cloud_batch build/plane_removal_driver build/segment_driver build/euclid_segment_driver build/test_cluster_desc_plan build/cluster_desc_driver build/test_cluster_match_plan build/test_match_colour_plan build/test_ground_plan build/test_match_plan build/test_voxel_plan build/test_change_plan build/change_driver build/fpfh_host build/fpfh_driver build/test_match_fpfh_plan build/fpfh_match_driver build/test_range_batch_plan build/test_fpfh_batch_plan build/fpfh_batch_driver build/vfh_host build/vfh_driver build/test_vfh_batch_plan build/vfh_batch_driver build/shot_host build/shot_driver
cli: build/comparator build/ply_dump build/rgb_segments build/rgb_segments_device build/rgb_segments_batch build/ground_segments build/spatial_change

build/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) $(EXTRA_HIPFLAGS) -c $< -o $@

$(LIBDIR)/libpcc_nn.so: $(HIP_OBJS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(HIP_OBJS) -ldl

oracle/_build/libpcc_oracle.so: oracle/pcc_oracle.c oracle/pcc_oracle.h
	@mkdir -p oracle/_build
	$(CC) -O2 -ffp-contract=off -fno-fast-math -fPIC -shared -pthread -o $@ oracle/pcc_oracle.c -lm

build/ubench_gather: tools/ubench/ubench_gather.hip
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 $< -o $@

build/ubench_scatter: tools/ubench/ubench_scatter.hip
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 $< -o $@

build/ubench_valu: tools/ubench/ubench_valu.hip
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 $< -o $@

build/test_lane_ops: tests/cpp/test_lane_ops.hip $(CSRC)/lane_ops.hpp
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -I$(CSRC) $< -o $@

# the shared host/device arithmetic headers, device compile against host compile (the library's own flags: its code generation)
build/test_device_math: tests/cpp/test_device_math.hip $(CSRC)/libm_f32.hpp $(CSRC)/plane_fit.hpp $(CSRC)/rift_math.hpp $(CSRC)/sift_math.hpp $(CSRC)/rigid_solve.hpp
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) $< -o $@ -pthread

build/test_host_mirror: tests/cpp/test_host_mirror.cpp include/pcc/point_types.hpp include/pcc/search.hpp include/pcc/comparator_nn.hpp include/pcc/multi_device.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include $< -o $@ -L$(LIBDIR) -lpcc_nn -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

build/comparator: examples/comparator_main.cpp pointcloudcomparator_amd/host/ply_io.hpp pointcloudcomparator_amd/host/report.hpp include/pcc/octree.hpp include/pcc/multi_device.hpp include/pcc/rift.hpp include/pcc/sift.hpp include/pcc/descriptors.hpp include/pcc/point_types.hpp include/pcc/search.hpp include/pcc/comparator_nn.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude -Ipointcloudcomparator_amd/host $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

build/test_report: tests/cpp/test_report.cpp pointcloudcomparator_amd/host/report.hpp include/pcc/comparator_nn.hpp include/pcc/descriptors.hpp include/pcc/rift.hpp include/pcc/sift.hpp include/pcc/search.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude -Ipointcloudcomparator_amd/host $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

build/test_match_batch: tests/cpp/test_match_batch.cpp pointcloudcomparator_amd/host/report.hpp include/pcc/comparator_nn.hpp include/pcc/descriptors.hpp include/pcc/rift.hpp include/pcc/sift.hpp include/pcc/region_growing_rgb.hpp include/pcc/search.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude -Ipointcloudcomparator_amd/host $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

build/rgb_segments: tests/cpp/rgb_segments.cpp include/pcc/region_growing_rgb.hpp include/pcc/search.hpp include/pcc/point_types.hpp pointcloudcomparator_amd/host/ply_io.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude -Ipointcloudcomparator_amd/host $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

build/rgb_segments_device: tests/cpp/rgb_segments_device.cpp include/pcc/region_growing_rgb.hpp include/pcc/search.hpp include/pcc/point_types.hpp pointcloudcomparator_amd/host/ply_io.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude -Ipointcloudcomparator_amd/host $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

build/rgb_segments_batch: tests/cpp/rgb_segments_batch.cpp include/pcc/region_growing_rgb.hpp include/pcc/search.hpp include/pcc/point_types.hpp pointcloudcomparator_amd/host/ply_io.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude -Ipointcloudcomparator_amd/host $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# dev helper of tools/exp_rgb.py (not part of `all`)
build/rgb_time: tools/rgb_time.cpp include/pcc/region_growing_rgb.hpp include/pcc/search.hpp include/pcc/point_types.hpp pointcloudcomparator_amd/host/ply_io.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude -Ipointcloudcomparator_amd/host $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# the host half of pcc_region_growing_rgb against the oracle on the CPU (no library, no GPU), plain and under ASan + UBSan
build/pcc_oracle_host.o: oracle/pcc_oracle.c oracle/pcc_oracle.h
	@mkdir -p build
	$(CC) -O2 -ffp-contract=off -fno-fast-math -pthread -c $< -o $@

build/test_rgb_merge: tests/cpp/test_rgb_merge.cpp $(CSRC)/rgb_merge.hpp build/pcc_oracle_host.o
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -pthread -I$(CSRC) -Ioracle $< build/pcc_oracle_host.o -o $@ -lm

build/asan/test_rgb_merge: tests/cpp/test_rgb_merge.cpp $(CSRC)/rgb_merge.hpp build/asan/pcc_oracle.o
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -pthread -I$(CSRC) -Ioracle $< build/asan/pcc_oracle.o -o $@ -lm

test-rgb-merge: build/test_rgb_merge build/asan/test_rgb_merge
	build/test_rgb_merge
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_rgb_merge

# the host half of pcc_region_growing_rgb_batch (the per-cloud cut of a concatenation's segments and pairs) the same way
build/test_rgb_batch_split: tests/cpp/test_rgb_batch_split.cpp $(CSRC)/rgb_batch_split.hpp $(CSRC)/rgb_merge.hpp build/pcc_oracle_host.o
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -pthread -I$(CSRC) -Ioracle $< build/pcc_oracle_host.o -o $@ -lm

build/asan/test_rgb_batch_split: tests/cpp/test_rgb_batch_split.cpp $(CSRC)/rgb_batch_split.hpp $(CSRC)/rgb_merge.hpp build/asan/pcc_oracle.o
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -pthread -I$(CSRC) -Ioracle $< build/asan/pcc_oracle.o -o $@ -lm

test-rgb-batch-split: build/test_rgb_batch_split build/asan/test_rgb_batch_split
	build/test_rgb_batch_split
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_rgb_batch_split

build/test_libm: tests/cpp/test_libm.cpp $(CSRC)/libm_f32.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@ -lm

build/test_acosf: tests/cpp/test_acosf.cpp $(CSRC)/libm_f32.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@ -lm

# the RIFT pipeline on the CPU from the headers the kernels use (test infrastructure: no library, no GPU)
build/rift_host: tests/cpp/rift_host.cpp $(CSRC)/rift_math.hpp $(CSRC)/plane_fit.hpp $(CSRC)/libm_f32.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@ -lm

build/rift_driver: tests/cpp/rift_driver.cpp include/pcc/rift.hpp include/pcc/search.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# the FPFH pipeline on the CPU from the headers the kernels use (test infrastructure: no library, no GPU)
build/fpfh_host: tests/cpp/fpfh_host.cpp $(CSRC)/fpfh_math.hpp $(CSRC)/plane_fit.hpp $(CSRC)/libm_f32.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@ -lm

build/fpfh_driver: tests/cpp/fpfh_driver.cpp include/pcc/fpfh.hpp include/pcc/search.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# the VFH descriptor and matchVHF on the CPU from the headers the kernels use (test infrastructure: no library, no GPU)
build/vfh_host: tests/cpp/vfh_host.cpp $(CSRC)/vfh_math.hpp $(CSRC)/fpfh_math.hpp $(CSRC)/plane_fit.hpp $(CSRC)/libm_f32.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@ -lm

# pcc::processVHF on one or two clouds, then pcc::matchVHF on their descriptors
build/vfh_driver: tests/cpp/vfh_driver.cpp include/pcc/vfh.hpp include/pcc/search.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# the SHOT352 pipeline on the CPU from the headers the kernels use (test infrastructure: no library, no GPU)
build/shot_host: tests/cpp/shot_host.cpp $(CSRC)/shot_math.hpp $(CSRC)/libm_f64.hpp $(CSRC)/plane_fit.hpp $(CSRC)/libm_f32.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@ -lm

# pcc::processSHOT through the library
build/shot_driver: tests/cpp/shot_driver.cpp include/pcc/shot.hpp include/pcc/search.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# the host scaffold the range-batch calls share (offsets, routes, upload layout, host pack) on the CPU (no library, no GPU)
build/test_range_batch_plan: tests/cpp/test_range_batch_plan.cpp $(CSRC)/vfh_batch_plan.hpp $(CSRC)/fpfh_batch_plan.hpp $(CSRC)/range_batch_plan.hpp $(CSRC)/cloud_batch.hpp $(CSRC)/rift_batch_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -I$(CSRC) $< -o $@

# the routes, bases, work items and output splice of pcc_fpfh_descriptors_batch on the CPU (no library, no GPU)
build/test_fpfh_batch_plan: tests/cpp/test_fpfh_batch_plan.cpp $(CSRC)/fpfh_batch_plan.hpp $(CSRC)/range_batch_plan.hpp $(CSRC)/cloud_batch.hpp $(CSRC)/rift_batch_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -I$(CSRC) $< -o $@

# pcc::processFPFHBatch against the loop of pcc::processFPFH
build/fpfh_batch_driver: tests/cpp/fpfh_batch_driver.cpp include/pcc/fpfh.hpp include/pcc/search.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# the routes, bases, vote items, bounds and copy runs of pcc_vfh_descriptors_batch on the CPU (no library, no GPU)
build/test_vfh_batch_plan: tests/cpp/test_vfh_batch_plan.cpp $(CSRC)/vfh_batch_plan.hpp $(CSRC)/range_batch_plan.hpp $(CSRC)/cloud_batch.hpp $(CSRC)/rift_batch_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -I$(CSRC) $< -o $@

# pcc::processVHFBatch against the loop of pcc::processVHF, and the matchVHF matrix overload
build/vfh_batch_driver: tests/cpp/vfh_batch_driver.cpp include/pcc/vfh.hpp include/pcc/search.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# the record packing of pcc_match_fpfh_batch on the CPU (no library, no GPU)
build/test_match_fpfh_plan: tests/cpp/test_match_fpfh_plan.cpp $(CSRC)/match_fpfh_plan.hpp $(CSRC)/match_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -I$(CSRC) $< -o $@

# pcc::processFPFH on two clouds, then pcc::matchFPFH on their descriptors
build/fpfh_match_driver: tests/cpp/fpfh_match_driver.cpp include/pcc/fpfh.hpp include/pcc/search.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

build/test_expf: tests/cpp/test_expf.cpp $(CSRC)/libm_f32.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@ -lm

# the SIFT detector on the CPU from the header the kernels use (test infrastructure: no library, no GPU)
build/sift_host: tests/cpp/sift_host.cpp $(CSRC)/sift_math.hpp $(CSRC)/libm_f32.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@ -lm

build/sift_driver: tests/cpp/sift_driver.cpp include/pcc/sift.hpp include/pcc/rift.hpp include/pcc/search.hpp include/pcc/comparator_nn.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# the work-item table of pcc_rift_descriptors_batch on the CPU (no library, no GPU)
build/test_rift_batch_plan: tests/cpp/test_rift_batch_plan.cpp $(CSRC)/rift_batch_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -I$(CSRC) $< -o $@

build/rift_batch_driver: tests/cpp/rift_batch_driver.cpp include/pcc/rift.hpp include/pcc/search.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# the per-round tables and the keypoint splice of pcc_sift_keypoints_batch on the CPU (no library, no GPU)
build/test_sift_batch_plan: tests/cpp/test_sift_batch_plan.cpp $(CSRC)/sift_batch_plan.hpp $(CSRC)/rift_batch_plan.hpp $(CSRC)/cloud_batch.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -I$(CSRC) $< -o $@

build/sift_batch_driver: tests/cpp/sift_batch_driver.cpp include/pcc/sift.hpp include/pcc/rift.hpp include/pcc/search.hpp include/pcc/comparator_nn.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# the routing, keypoint order, cloud places and output splice of pcc_cluster_descriptors on the CPU (no library, no GPU)
build/test_cluster_desc_plan: tests/cpp/test_cluster_desc_plan.cpp $(CSRC)/cluster_desc_plan.hpp $(CSRC)/sift_batch_plan.hpp $(CSRC)/rift_batch_plan.hpp $(CSRC)/cloud_batch.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -I$(CSRC) $< -o $@

# pcc::clusterDescriptors, the descriptor loop of a comparison in one call
build/cluster_desc_driver: tests/cpp/cluster_desc_driver.cpp include/pcc/descriptors.hpp include/pcc/sift.hpp include/pcc/rift.hpp include/pcc/search.hpp include/pcc/comparator_nn.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# the candidates, gates, acceptance and work-item table of pcc_cluster_matching on the CPU (no library, no GPU)
build/test_cluster_match_plan: tests/cpp/test_cluster_match_plan.cpp $(CSRC)/cluster_match_plan.hpp $(CSRC)/match_dims_plan.hpp $(CSRC)/match_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@

# the plan the three descriptor searches share (slice rule, table of work items, shared reference clouds) against the tables its
# users built before they shared it (tests/golden/match_plan_tables.txt), on the CPU (no library, no GPU)
build/test_match_plan: tests/cpp/test_match_plan.cpp $(CSRC)/match_plan.hpp $(CSRC)/match_dims_plan.hpp $(CSRC)/cluster_match_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -I$(CSRC) $< -o $@

# the distinct clusters, routes, bases and the map back of pcc_match_colour_elements on the CPU (no library, no GPU)
build/test_match_colour_plan: tests/cpp/test_match_colour_plan.cpp $(CSRC)/match_colour_plan.hpp $(CSRC)/rift_batch_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -I$(CSRC) $< -o $@

# the window table, refusals and lattice sizing of the morphological ground filter on the CPU (no library, no GPU)
build/test_ground_plan: tests/cpp/test_ground_plan.cpp $(CSRC)/ground_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@

# the leaf lattice of the voxel grid (origin, dimensions, the int32 and 2^26 refusals) on the CPU (no library, no GPU)
build/test_voxel_plan: tests/cpp/test_voxel_plan.cpp $(CSRC)/voxel_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@

# the lattice of pcc_change_detection (anchor, voxel coordinates, the 2^31 and 2^21 refusals, keys, table size) on the CPU (no library, no GPU)
build/test_change_plan: tests/cpp/test_change_plan.cpp $(CSRC)/change_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@

# the reference's call sequence against pcc::octree::OctreePointCloudChangeDetector, and pcc::spatialChangeDetection
build/change_driver: tests/cpp/change_driver.cpp include/pcc/octree.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# pcc::spatialChangeDetection: two PLYs and a resolution in, the points of the second in voxels the first leaves empty out
build/spatial_change: tests/cpp/spatial_change.cpp include/pcc/octree.hpp include/pcc/point_types.hpp pointcloudcomparator_amd/host/ply_io.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude -Ipointcloudcomparator_amd/host $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# dev helper of tools/exp_changes.py (not part of `all`): the same lattice with std::unordered_set on one host core
build/changes_host: tools/changes_host.cpp $(CSRC)/change_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@

# pcc::groundSegmentation: a PLY in, <prefix>_ground.ply and <prefix>_object.ply out, as the reference's ground_segmentation writes them
build/ground_segments: tests/cpp/ground_segments.cpp include/pcc/ground.hpp include/pcc/point_types.hpp pointcloudcomparator_amd/host/ply_io.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude -Ipointcloudcomparator_amd/host $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# dev helper of tools/exp_ground.py (not part of `all`): the ground filter on one host core, lattice-accelerated
build/ground_host: tools/ground_host.cpp $(CSRC)/ground_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@

# the host scaffold the batch calls share (route split, pack, upload layouts) on the CPU (no library, no GPU)
build/test_cloud_batch: tests/cpp/test_cloud_batch.cpp $(CSRC)/cloud_batch.hpp $(CSRC)/rift_batch_plan.hpp $(CSRC)/sift_batch_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -I$(CSRC) $< -o $@

# the record packing and work-item table of pcc_match_knn_batch_dims on the CPU (no library, no GPU)
build/test_match_dims_plan: tests/cpp/test_match_dims_plan.cpp $(CSRC)/match_dims_plan.hpp $(CSRC)/match_plan.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -I$(CSRC) $< -o $@

build/match_dims_driver: tests/cpp/match_dims_driver.cpp include/pcc/comparator_nn.hpp include/pcc/search.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# pcc::removePlanes against the SACSegmentation + ExtractIndices loop it replaces
build/plane_removal_driver: tests/cpp/plane_removal_driver.cpp include/pcc/comparator_nn.hpp include/pcc/search.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# pcc::regionGrowingSegmentation against the VoxelGrid + NormalEstimation + RegionGrowing objects it replaces
build/segment_driver: tests/cpp/segment_driver.cpp include/pcc/comparator_nn.hpp include/pcc/search.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

# pcc::euclideanClusterSegmentation against the VoxelGrid + SACSegmentation + ExtractIndices + EuclideanClusterExtraction objects it replaces
build/euclid_segment_driver: tests/cpp/euclid_segment_driver.cpp include/pcc/comparator_nn.hpp include/pcc/search.hpp include/pcc/point_types.hpp include/pcc_nn.h $(LIBDIR)/libpcc_nn.so
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude $< -o $@ -L$(LIBDIR) -lpcc_nn -Wl,-rpath,'$$ORIGIN/../$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

build/ply_dump: tests/cpp/ply_dump.cpp pointcloudcomparator_amd/host/ply_io.hpp include/pcc/point_types.hpp
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -Wall -Iinclude -Ipointcloudcomparator_amd/host $< -o $@

# ---- sanitizers on the host-side code (CPU build only; sanitizers never run on the GPU box) --------------------
# oracle/pcc_oracle.c, csrc/flann_tree.hpp (the PCC_TIES_FLANN tree: build + walk), csrc/rigid_solve.hpp,
# csrc/plane_fit.hpp and host/ply_io.hpp under ASan + UBSan with a CPU-only driver, and the report writer's self-test.
SANFLAGS := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1 -ffp-contract=off
asan: build/asan/asan_driver build/asan/test_flann_tree build/asan/rift_host build/asan/fpfh_host build/asan/vfh_host build/asan/shot_host build/asan/sift_host build/asan/test_match_dims_plan build/asan/test_match_fpfh_plan build/asan/test_sift_batch_plan build/asan/test_rgb_batch_split build/asan/test_cloud_batch build/asan/test_cluster_desc_plan build/asan/test_cluster_match_plan build/asan/test_match_colour_plan build/asan/test_ground_plan build/asan/test_match_plan build/asan/test_voxel_plan build/asan/test_change_plan build/asan/test_range_batch_plan build/asan/test_fpfh_batch_plan build/asan/test_vfh_batch_plan
	ASAN_OPTIONS=detect_leaks=1 build/asan/asan_driver build/asan
	ASAN_OPTIONS=detect_leaks=1 build/asan/rift_host --self build/asan/rift_self.bin
	ASAN_OPTIONS=detect_leaks=1 build/asan/fpfh_host --self build/asan/fpfh_self.bin
	ASAN_OPTIONS=detect_leaks=1 build/asan/shot_host --self build/asan/shot_self.bin
	ASAN_OPTIONS=detect_leaks=1 build/asan/vfh_host --self build/asan/vfh_self.bin
	ASAN_OPTIONS=detect_leaks=1 build/asan/sift_host --self build/asan/sift_self.bin
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_match_dims_plan
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_match_fpfh_plan
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_sift_batch_plan
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_rgb_batch_split
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_cloud_batch
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_cluster_desc_plan
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_cluster_match_plan
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_match_colour_plan
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_ground_plan
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_match_plan
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_voxel_plan
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_change_plan
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_range_batch_plan
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_fpfh_batch_plan
	ASAN_OPTIONS=detect_leaks=1 build/asan/test_vfh_batch_plan
	@echo "asan: clean"

build/asan/pcc_oracle.o: oracle/pcc_oracle.c oracle/pcc_oracle.h
	@mkdir -p build/asan
	$(CC) $(SANFLAGS) -fno-fast-math -pthread -c $< -o $@

build/asan/asan_driver: tests/cpp/asan_driver.cpp build/asan/pcc_oracle.o $(CSRC)/flann_tree.hpp $(CSRC)/rigid_solve.hpp $(CSRC)/plane_fit.hpp pointcloudcomparator_amd/host/ply_io.hpp include/pcc/point_types.hpp
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -pthread -Iinclude -I$(CSRC) -Ipointcloudcomparator_amd/host -Ioracle $< build/asan/pcc_oracle.o -o $@ -lm

build/asan/test_flann_tree: tests/cpp/test_flann_tree.cpp $(CSRC)/flann_tree.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -pthread -I$(CSRC) $< -o $@

build/asan/rift_host: tests/cpp/rift_host.cpp $(CSRC)/rift_math.hpp $(CSRC)/plane_fit.hpp $(CSRC)/libm_f32.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@ -lm

build/asan/fpfh_host: tests/cpp/fpfh_host.cpp $(CSRC)/fpfh_math.hpp $(CSRC)/plane_fit.hpp $(CSRC)/libm_f32.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@ -lm

build/asan/shot_host: tests/cpp/shot_host.cpp $(CSRC)/shot_math.hpp $(CSRC)/libm_f64.hpp $(CSRC)/plane_fit.hpp $(CSRC)/libm_f32.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@ -lm

build/asan/vfh_host: tests/cpp/vfh_host.cpp $(CSRC)/vfh_math.hpp $(CSRC)/fpfh_math.hpp $(CSRC)/plane_fit.hpp $(CSRC)/libm_f32.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@ -lm

build/asan/sift_host: tests/cpp/sift_host.cpp $(CSRC)/sift_math.hpp $(CSRC)/libm_f32.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@ -lm

build/asan/test_match_dims_plan: tests/cpp/test_match_dims_plan.cpp $(CSRC)/match_dims_plan.hpp $(CSRC)/match_plan.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@

build/asan/test_match_fpfh_plan: tests/cpp/test_match_fpfh_plan.cpp $(CSRC)/match_fpfh_plan.hpp $(CSRC)/match_plan.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@

build/asan/test_range_batch_plan: tests/cpp/test_range_batch_plan.cpp $(CSRC)/vfh_batch_plan.hpp $(CSRC)/fpfh_batch_plan.hpp $(CSRC)/range_batch_plan.hpp $(CSRC)/cloud_batch.hpp $(CSRC)/rift_batch_plan.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@

build/asan/test_fpfh_batch_plan: tests/cpp/test_fpfh_batch_plan.cpp $(CSRC)/fpfh_batch_plan.hpp $(CSRC)/range_batch_plan.hpp $(CSRC)/cloud_batch.hpp $(CSRC)/rift_batch_plan.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@

build/asan/test_vfh_batch_plan: tests/cpp/test_vfh_batch_plan.cpp $(CSRC)/vfh_batch_plan.hpp $(CSRC)/range_batch_plan.hpp $(CSRC)/cloud_batch.hpp $(CSRC)/rift_batch_plan.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@

build/asan/test_match_plan: tests/cpp/test_match_plan.cpp $(CSRC)/match_plan.hpp $(CSRC)/match_dims_plan.hpp $(CSRC)/cluster_match_plan.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@

build/asan/test_sift_batch_plan: tests/cpp/test_sift_batch_plan.cpp $(CSRC)/sift_batch_plan.hpp $(CSRC)/rift_batch_plan.hpp $(CSRC)/cloud_batch.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@

build/asan/test_cloud_batch: tests/cpp/test_cloud_batch.cpp $(CSRC)/cloud_batch.hpp $(CSRC)/rift_batch_plan.hpp $(CSRC)/sift_batch_plan.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@

build/asan/test_cluster_desc_plan: tests/cpp/test_cluster_desc_plan.cpp $(CSRC)/cluster_desc_plan.hpp $(CSRC)/sift_batch_plan.hpp $(CSRC)/rift_batch_plan.hpp $(CSRC)/cloud_batch.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@

build/asan/test_cluster_match_plan: tests/cpp/test_cluster_match_plan.cpp $(CSRC)/cluster_match_plan.hpp $(CSRC)/match_dims_plan.hpp $(CSRC)/match_plan.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@

build/asan/test_match_colour_plan: tests/cpp/test_match_colour_plan.cpp $(CSRC)/match_colour_plan.hpp $(CSRC)/rift_batch_plan.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@

build/asan/test_ground_plan: tests/cpp/test_ground_plan.cpp $(CSRC)/ground_plan.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -Wall -I$(CSRC) $< -o $@

# (float-cast-overflow is not part of `undefined`: a conversion of a bound an int cannot hold must stop this one)
build/asan/test_voxel_plan: tests/cpp/test_voxel_plan.cpp $(CSRC)/voxel_plan.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -fsanitize=float-cast-overflow -fno-sanitize-recover=float-cast-overflow -Wall -I$(CSRC) $< -o $@

build/asan/test_change_plan: tests/cpp/test_change_plan.cpp $(CSRC)/change_plan.hpp
	@mkdir -p build/asan
	$(CXX) -std=c++17 $(SANFLAGS) -fsanitize=float-cast-overflow -fno-sanitize-recover=float-cast-overflow -Wall -I$(CSRC) $< -o $@

clean:
	rm -rf build $(LIBDIR)/*.so oracle/_build

.PHONY: all lib prof oracle ubench hosttest cli clean asan test-rgb-merge test-rgb-batch-split
