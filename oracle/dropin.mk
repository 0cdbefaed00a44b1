# oracle/dropin.mk -- the drop-in proof: the REFERENCE's own callers of dvo::DenseTracker, compiled UNMODIFIED from where they lie
# under $(REFERENCE), against THIS engine's facade headers (include/dvo/) instead of the reference's dvo_core, and linked with
# libdvo_hip.so.  Test infrastructure: the project's side of it (bridge, drivers, stubs, shims) lives in tests/dropin/, everything
# built from reference sources goes to oracle/_ref/dropin/ with the rest of oracle/_ref.  Needs the reference tree at build time
# only (the built objects travel with oracle/_ref).  `make -C oracle -f dropin.mk`
#
#   reference sources compiled (zero edits): dvo_slam/src/{local_tracker,keyframe_tracker,tracking_result_evaluation,local_map,
#       config}.cpp, dvo_slam/src/constraints/{constraint_proposal,constraint_proposal_validator,constraint_proposal_voter}.cpp
#       -- the tracking front end and the loop-closure proposal validation; in libdvo_dropin.so and benchmark_slam the pose-graph
#       back end is the counting sink oracle/ref_graph_stub.cpp, in benchmark_slam_graph it is the reference's own
#       dvo_slam/src/keyframe_graph.cpp + keyframe_constraint_search.cpp (below)
#   headers they see:  include/dvo/**          this engine's facade (DenseTracker, RgbdImagePyramid, PointSelection, util/...)
#                      $(REFERENCE)/dvo_slam/include   the reference's own dvo_slam headers
#                      tests/dropin/shim_threads/tbb   tbb::parallel_invoke on two real threads (the engine build only)
#                      oracle/shim/**          stand-ins for the third-party libraries that are not installed here (Eigen, OpenCV,
#                                              boost, TBB, g2o, ROS message / console headers)
#                      _ref/dropin/ft/dvo/visualization -> the reference's visualizer INTERFACE headers (display only, SURVEY.md
#                                              section 2 #10: they read RgbdImage's public fields, which the facade keeps)
#   tests/dropin/dropin_bridge.cpp: C entry points = oracle/ref_public_api.inc, the same caller code that oracle/_ref runs on the
#                      reference's CPU tracker (tests/test_dropin.py compares the two runs)
CXX ?= g++
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))..)
# the reference tree: where oracle/Makefile (the recipe of the rest of oracle/_ref) looks for it, unless given on the command line
REFERENCE ?= $(shell sed -n 's/^REFERENCE ?= //p' $(ROOT)/oracle/Makefile)
REFERENCE := $(REFERENCE)
D := $(ROOT)/tests/dropin
B := $(ROOT)/oracle/_ref/dropin
SLAM_SRC := $(REFERENCE)/dvo_slam/src
UNITS := local_tracker keyframe_tracker tracking_result_evaluation local_map config constraints/constraint_proposal \
         constraints/constraint_proposal_validator constraints/constraint_proposal_voter
FLAGS := -std=c++14 -O2 -fPIC -pthread -I$(D)/shim_threads -I$(ROOT)/oracle/shim -I$(REFERENCE)/dvo_slam/include -I$(ROOT)/include -I$(B)/ft
OBJS := $(foreach u,$(UNITS),$(B)/$(notdir $(u)).o)
FACADE := $(wildcard $(ROOT)/include/dvo/*.h $(ROOT)/include/dvo/core/*.h $(ROOT)/include/dvo/util/*.h $(ROOT)/include/dvo_hip.h)

all: $(if $(wildcard $(SLAM_SRC)/local_tracker.cpp),$(B)/libdvo_dropin.so $(B)/benchmark_slam $(B)/benchmark_slam_ref $(B)/libdvo_camera_node.so \
        $(B)/benchmark_slam_graph $(B)/benchmark_slam_graph_ref $(B)/libdvo_slam_node.so)

$(B)/libdvo_dropin.so: $(D)/dropin_bridge.cpp $(ROOT)/oracle/ref_public_api.inc $(ROOT)/oracle/ref_graph_stub.cpp $(FACADE) \
                         $(foreach u,$(UNITS),$(SLAM_SRC)/$(u).cpp) $(ROOT)/dvo_slam_amd/lib/libdvo_hip.so
	@mkdir -p $(B)/ft/dvo
	@ln -sfn $(REFERENCE)/dvo_core/include/dvo/visualization $(B)/ft/dvo/visualization
	@for u in $(UNITS); do $(CXX) $(FLAGS) -c $(SLAM_SRC)/$$u.cpp -o $(B)/$$(basename $$u).o || exit 1; done
	$(CXX) $(FLAGS) -c $(ROOT)/oracle/ref_graph_stub.cpp -o $(B)/ref_graph_stub.o
	$(CXX) $(FLAGS) -I$(ROOT)/oracle -c $(D)/dropin_bridge.cpp -o $(B)/dropin_bridge.o
	$(CXX) -shared -pthread -Wl,--no-undefined -o $@ $(OBJS) $(B)/ref_graph_stub.o $(B)/dropin_bridge.o \
	    -L$(ROOT)/dvo_slam_amd/lib -ldvo_hip '-Wl,-rpath,$$ORIGIN/../../../dvo_slam_amd/lib' -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib

# ---- the reference's BUILT TARGET dvo_benchmark/src/benchmark_slam.cpp (dvo_benchmark/CMakeLists.txt: rosbuild_add_executable
# benchmark), unmodified, twice:
#   _ref/dropin/benchmark_slam       against this engine's facade + libdvo_hip.so  (runs on the MI355X)
#   _ref/dropin/benchmark_slam_ref   against the reference's own dvo_core objects (oracle/_ref/*.o; runs on the CPU) -- the golden run
# Both link the same dvo_slam front-end sources, the counting pose-graph sink (oracle/ref_graph_stub.cpp) and tests/dropin/benchmark_stubs.cpp
# (PNG reading for cv::imread, constructible-only display classes).  tests/dropin/shim holds the extra third-party stand-ins this file needs.
BENCH_SRC := $(REFERENCE)/dvo_benchmark/src/benchmark_slam.cpp
BENCH_INC := -I$(D)/shim -I$(ROOT)/oracle/shim -I$(REFERENCE)/dvo_slam/include -I$(REFERENCE)/dvo_benchmark/include -I$(REFERENCE)/dvo_ros/include
BENCH_EXTRA := $(SLAM_SRC)/serialization/map_serializer_interface.cpp $(REFERENCE)/dvo_core/src/visualization/camera_trajectory_visualizer.cpp
SHIMS := $(shell find $(D)/shim $(ROOT)/oracle/shim -type f)
REF_OBJ_DIR := $(ROOT)/oracle/_ref
REF_CORE := dense_tracking dense_tracking_config dense_tracking_impl math_sse intrinsic_matrix surface_pyramid point_selection \
            least_squares weight_calculation rgbd_image rgbd_image_sse interpolation

$(B)/benchmark_slam: $(B)/libdvo_dropin.so $(D)/benchmark_stubs.cpp $(BENCH_SRC) $(SHIMS) $(ROOT)/include/dvo_benchmark/image_io.h
	@mkdir -p $(B)/bench
	$(CXX) -std=c++14 -O2 -fPIC -pthread $(BENCH_INC) -I$(ROOT)/include -I$(B)/ft -c $(BENCH_SRC) -o $(B)/bench/benchmark_slam.o
	@for f in $(BENCH_EXTRA) $(D)/benchmark_stubs.cpp; do $(CXX) -std=c++14 -O2 -fPIC -pthread $(BENCH_INC) -I$(ROOT)/include -I$(B)/ft -c $$f -o $(B)/bench/$$(basename $$f .cpp).o || exit 1; done
	$(CXX) -pthread -o $@ $(B)/bench/*.o $(OBJS) $(B)/ref_graph_stub.o \
	    -L$(ROOT)/dvo_slam_amd/lib -ldvo_hip '-Wl,-rpath,$$ORIGIN/../../../dvo_slam_amd/lib' -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib -lz

$(B)/benchmark_slam_ref: $(REF_OBJ_DIR)/libdvo_ref.so $(D)/benchmark_stubs.cpp $(BENCH_SRC) $(SHIMS) $(ROOT)/include/dvo_benchmark/image_io.h
	@mkdir -p $(B)/bench_ref
	$(CXX) -std=c++14 -O2 -march=native -ffp-contract=off -fPIC -pthread $(BENCH_INC) -I$(REFERENCE)/dvo_core/include -c $(BENCH_SRC) -o $(B)/bench_ref/benchmark_slam.o
	@for f in $(BENCH_EXTRA) $(D)/benchmark_stubs.cpp; do $(CXX) -std=c++14 -O2 -march=native -ffp-contract=off -fPIC -pthread $(BENCH_INC) -I$(REFERENCE)/dvo_core/include -idirafter $(ROOT)/include -c $$f -o $(B)/bench_ref/$$(basename $$f .cpp).o || exit 1; done
	$(CXX) -pthread -o $@ $(B)/bench_ref/*.o $(foreach u,$(REF_CORE) $(notdir $(UNITS)),$(REF_OBJ_DIR)/$(u).o) $(REF_OBJ_DIR)/ref_graph_stub.o -lz

# ---- the same executable with the reference's REAL pose-graph back end, dvo_slam/src/keyframe_graph.cpp (+ its neighbour search,
# keyframe_constraint_search.cpp), compiled unmodified in place of the counting sink: keyframe insertion, loop-closure proposals, the
# TBB parallel_reduce over thread-local ConstraintProposalValidators (-> concurrent DenseTracker::match calls on the engine), edge
# insertion and the robust-kernel bookkeeping all run; g2o is the container stand-in of oracle/shim/g2o, whose optimize() leaves the
# estimates where they are (graph optimisation is out of scope), PCL's radius search is tests/dropin/shim/pcl/kdtree.  The serialisers at the end of
# benchmark_slam.cpp (tests/dropin/benchmark_stubs.cpp) dump the graph's vertices and edges for comparison between the two builds:
#   _ref/dropin/benchmark_slam_graph       facade + libdvo_hip.so, parallel_reduce on four threads (-DDVO_SHIM_TBB_THREADS)
#   _ref/dropin/benchmark_slam_graph_ref   the reference's dvo_core objects (oracle/_ref), the same partition walked serially
GRAPH_UNITS := keyframe_graph keyframe_constraint_search
GRAPH_FLAGS := -std=c++14 -O2 -fPIC -pthread -I$(D)/shim_threads -I$(D)/shim -I$(ROOT)/oracle/shim -I$(REFERENCE)/dvo_slam/include -I$(ROOT)/include -I$(B)/ft
$(B)/benchmark_slam_graph: $(B)/benchmark_slam $(D)/graph_visualizer_stub.cpp $(foreach u,$(GRAPH_UNITS),$(SLAM_SRC)/$(u).cpp) $(SHIMS)
	@mkdir -p $(B)/graph
	@for u in $(GRAPH_UNITS); do $(CXX) $(GRAPH_FLAGS) -DDVO_SHIM_TBB_THREADS -c $(SLAM_SRC)/$$u.cpp -o $(B)/graph/$$u.o || exit 1; done
	$(CXX) $(GRAPH_FLAGS) -c $(D)/graph_visualizer_stub.cpp -o $(B)/graph/graph_visualizer_stub.o
	$(CXX) -pthread -o $@ $(B)/bench/*.o $(OBJS) $(B)/graph/*.o \
	    -L$(ROOT)/dvo_slam_amd/lib -ldvo_hip '-Wl,-rpath,$$ORIGIN/../../../dvo_slam_amd/lib' -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib -lz

$(B)/benchmark_slam_graph_ref: $(B)/benchmark_slam_ref $(D)/graph_visualizer_stub.cpp $(foreach u,$(GRAPH_UNITS),$(SLAM_SRC)/$(u).cpp) $(SHIMS)
	@mkdir -p $(B)/graph_ref
	@for u in $(GRAPH_UNITS); do $(CXX) -std=c++14 -O2 -march=native -ffp-contract=off -fPIC -pthread $(BENCH_INC) -I$(REFERENCE)/dvo_core/include \
	    -c $(SLAM_SRC)/$$u.cpp -o $(B)/graph_ref/$$u.o || exit 1; done
	$(CXX) -std=c++14 -O2 -fPIC -pthread $(BENCH_INC) -I$(REFERENCE)/dvo_core/include -c $(D)/graph_visualizer_stub.cpp -o $(B)/graph_ref/graph_visualizer_stub.o
	$(CXX) -pthread -o $@ $(B)/bench_ref/*.o $(foreach u,$(REF_CORE) $(notdir $(UNITS)),$(REF_OBJ_DIR)/$(u).o) $(B)/graph_ref/*.o -lz

# ---- the reference's live-camera front end dvo_ros/src/camera_dense_tracking.cpp + camera_base.cpp (the Affine3d&
# overload of match(), RgbdCameraPyramid::create per frame, convertRawDepthImageSse, configtools.h), unmodified, against the facade;
# ROS (node handles, message_filters, tf, cv_bridge, dynamic_reconfigure) are the stand-ins under tests/dropin/shim; tests/dropin/camera_node_driver.cpp feeds it
ROS_SRC := $(REFERENCE)/dvo_ros/src
$(B)/libdvo_camera_node.so: $(D)/camera_node_driver.cpp $(D)/camera_node_stubs.cpp $(ROS_SRC)/camera_dense_tracking.cpp $(ROS_SRC)/camera_base.cpp $(SHIMS) $(FACADE) \
                              $(ROOT)/dvo_slam_amd/lib/libdvo_hip.so
	@mkdir -p $(B)/ros $(B)/ft/dvo
	@ln -sfn $(REFERENCE)/dvo_core/include/dvo/visualization $(B)/ft/dvo/visualization
	@for f in $(ROS_SRC)/camera_dense_tracking.cpp $(ROS_SRC)/camera_base.cpp $(REFERENCE)/dvo_core/src/visualization/camera_trajectory_visualizer.cpp $(D)/camera_node_driver.cpp $(D)/camera_node_stubs.cpp; do \
	    $(CXX) -std=c++14 -O2 -fPIC -pthread $(BENCH_INC) -I$(ROOT)/include -I$(B)/ft -c $$f -o $(B)/ros/$$(basename $$f .cpp).o || exit 1; done
	$(CXX) -shared -pthread -Wl,--no-undefined -o $@ $(B)/ros/*.o \
	    -L$(ROOT)/dvo_slam_amd/lib -ldvo_hip '-Wl,-rpath,$$ORIGIN/../../../dvo_slam_amd/lib' -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib -lz

# ---- the reference's live SLAM node dvo_slam/src/camera_keyframe_tracking.cpp (+ dvo_ros/src/camera_base.cpp), unmodified, on the
# facade, with the front end, the real keyframe graph (above) and the reference's own no-op visualiser; tests/dropin/slam_node_driver.cpp feeds it
$(B)/libdvo_slam_node.so: $(B)/libdvo_camera_node.so $(B)/benchmark_slam_graph $(D)/slam_node_driver.cpp $(D)/slam_node_stubs.cpp $(SLAM_SRC)/camera_keyframe_tracking.cpp $(SHIMS)
	@mkdir -p $(B)/slam_node
	@for f in $(SLAM_SRC)/camera_keyframe_tracking.cpp $(D)/slam_node_driver.cpp $(D)/slam_node_stubs.cpp; do \
	    $(CXX) -std=c++14 -O2 -fPIC -pthread -I$(D)/shim_threads $(BENCH_INC) -I$(ROOT)/include -I$(B)/ft -c $$f -o $(B)/slam_node/$$(basename $$f .cpp).o || exit 1; done
	$(CXX) -shared -pthread -Wl,--no-undefined -o $@ $(B)/slam_node/*.o $(B)/ros/camera_base.o $(B)/ros/camera_trajectory_visualizer.o \
	    $(B)/bench/map_serializer_interface.o $(filter-out $(B)/ref_graph_stub.o,$(OBJS)) $(B)/graph/*.o \
	    -L$(ROOT)/dvo_slam_amd/lib -ldvo_hip '-Wl,-rpath,$$ORIGIN/../../../dvo_slam_amd/lib' -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib -lz

$(REF_OBJ_DIR)/libdvo_ref.so:
	$(MAKE) -C $(ROOT)/oracle

clean:
	rm -rf $(B)
