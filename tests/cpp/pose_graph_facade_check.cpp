// The C++ facade's pose graph (include/dvo_slam/pose_graph.h) and LocalMap::optimize (include/dvo_slam/local_map.h).
// usage: pose_graph_facade_check host | device
//  host: what needs no device -- ids are mapped to dense indices by rank, taken and unknown ids are refused, an edge leaves, a local
//        map loads as vertex 0 = the keyframe (fixed), vertex k = frame k, edge i = measurement i;
//  device: the same, then a local map two of whose frame poses are 0.1 m off is optimised for 50 iterations and comes back to what its
//        measurements say, and PoseGraph reports chi2 and weights and removes a planted false edge.
// Prints "ok" or the first mismatch.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dvo_slam/local_map.h"
#include "dvo_slam/pose_graph.h"

using dvo::core::AffineTransformd;
using dvo::core::Matrix6d;

namespace {

AffineTransformd shift(double x, double y, double z) {
  AffineTransformd T;
  T.setIdentity();
  T.matrix()(0, 3) = x;
  T.matrix()(1, 3) = y;
  T.matrix()(2, 3) = z;
  return T;
}

Matrix6d information(double v) {
  Matrix6d m;
  m.setZero();
  for (int i = 0; i < 6; ++i) m(i, i) = v;
  return m;
}

#define EXPECT(cond)                                      \
  if (!(cond)) {                                          \
    std::printf("line %d: %s\n", __LINE__, #cond);        \
    return 1;                                             \
  }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: pose_graph_facade_check host|device\n"); return 2; }
  const bool device = std::strcmp(argv[1], "device") == 0;

  // ids -> dense indices
  dvo_slam::PoseGraph g;
  EXPECT(g.addVertex(40, shift(0, 0, 0), true) && g.addVertex(7, shift(1, 0, 0)) && g.addVertex(1000, shift(2, 0, 0)));
  EXPECT(!g.addVertex(7, shift(9, 9, 9)) && g.numVertices() == 3);
  EXPECT(g.vertexIndex(7) == 0 && g.vertexIndex(40) == 1 && g.vertexIndex(1000) == 2 && g.vertexIndex(8) == -1);
  EXPECT(g.addEdge(5, 40, 7, shift(1, 0, 0), information(100.0)) && g.addEdge(2, 7, 1000, shift(1, 0, 0), information(100.0), 5.0));
  EXPECT(!g.addEdge(5, 7, 40, shift(0, 0, 0), information(1.0)) && !g.addEdge(6, 7, 7, shift(0, 0, 0), information(1.0)));
  EXPECT(!g.addEdge(6, 7, 8, shift(0, 0, 0), information(1.0)) && !g.addEdge(6, 7, 40, shift(0, 0, 0), information(1.0), -1.0));
  EXPECT(g.edgeIndex(2) == 0 && g.edgeIndex(5) == 1 && g.edgeIndex(6) == -1 && g.numEdges() == 2);
  EXPECT(g.estimate(1000).matrix()(0, 3) == 2.0 && g.chi2(5) == 0.0 && g.robustWeight(2) == 1.0);
  EXPECT(g.setFixed(7, true) && !g.setFixed(8, true) && g.setEstimate(7, shift(1.5, 0, 0)) && g.estimate(7).matrix()(0, 3) == 1.5);
  EXPECT(g.removeEdge(2) && !g.removeEdge(2) && g.numEdges() == 1 && g.edgeIndex(5) == 0 && !g.hasEdge(2) && g.hasEdge(5));

  // a local map as a graph
  dvo_slam::LocalMap::Ptr map = dvo_slam::LocalMap::create(dvo::core::RgbdImagePyramid::Ptr(), shift(1, 2, 3));
  // (frames 0 and 2 get no keyframe measurement: their estimates stay those of the frame before, 0.1 m short of what the odometry says)
  for (int k = 0; k < 4; ++k) {
    map->addFrame(dvo::core::RgbdImagePyramid::Ptr());
    map->addOdometryMeasurement(shift(0.1, 0, 0), information(400.0));
    if (k % 2 == 1) map->addKeyframeMeasurement(shift(0.1 * (k + 1), 0, 0), information(100.0));
  }
  dvo_slam::PoseGraph loaded;
  map->load(loaded);
  EXPECT(loaded.numVertices() == 5 && loaded.numEdges() == 6 && loaded.vertexIndex(0) == 0 && loaded.vertexIndex(4) == 4);
  EXPECT(loaded.estimate(0).matrix()(1, 3) == 2.0 && loaded.estimate(2).matrix()(0, 3) == 1.0 + 0.1 * 2);
  EXPECT(loaded.estimate(1).matrix()(0, 3) == 1.0 && loaded.estimate(3).matrix()(0, 3) == loaded.estimate(2).matrix()(0, 3));
  EXPECT(map->measurements().size() == 6 && map->measurements()[1].from == 1 && map->measurements()[1].to == 2 && map->measurements()[2].from == 0 &&
         map->measurements()[2].to == 2);

  if (device) {
    EXPECT(dvo_hip_device_count() > 0);
    const int trials = map->optimize();
    EXPECT(trials >= 1 && trials <= 50);
    // the measurements agree with each other: every frame lands 0.1 m behind the one before, the knocked-off ones included
    for (size_t k = 0; k < 4; ++k) {
      EXPECT(std::fabs(map->getFramePose(k).matrix()(0, 3) - (1.0 + 0.1 * double(k + 1))) < 1e-9);
      EXPECT(std::fabs(map->getFramePose(k).matrix()(1, 3) - 2.0) < 1e-9 && std::fabs(map->getFramePose(k).matrix()(2, 3) - 3.0) < 1e-9);
    }
    AffineTransformd keyframe;
    keyframe = map->getKeyframePose();
    EXPECT(keyframe.matrix()(0, 3) == 1.0 && keyframe.matrix()(1, 3) == 2.0 && keyframe.matrix()(2, 3) == 3.0);

    // a chain of five with one false edge under the kernel
    dvo_slam::PoseGraph chain;
    for (int v = 0; v < 5; ++v) chain.addVertex(10 * v, shift(0.2 * v + 0.01 * (v % 2), 0, 0), v == 0);
    int id = 0;
    for (int v = 0; v + 1 < 5; ++v) chain.addEdge(id++, 10 * v, 10 * (v + 1), shift(0.2, 0, 0), information(1e4), 5.0);
    for (int v = 0; v + 2 < 5; ++v) chain.addEdge(id++, 10 * v, 10 * (v + 2), shift(0.4, 0, 0), information(1e4), 5.0);
    const int planted = id;
    chain.addEdge(id++, 0, 40, shift(0.8, 1.0, 0), information(1e4), 5.0);
    EXPECT(chain.optimize(30) >= 1 && chain.report().final_cost < chain.report().initial_cost);
    for (int e = 0; e < planted; ++e) EXPECT(chain.robustWeight(e) > 0.5 && chain.chi2(e) < 25.0);
    EXPECT(chain.robustWeight(planted) < 0.01);
    const std::vector<int> gone = chain.removeOutlierConstraints(0.1);
    EXPECT(gone.size() == 1 && gone[0] == planted && chain.numEdges() == size_t(planted));
    EXPECT(chain.optimize(30) >= 0);
    for (int v = 0; v < 5; ++v) EXPECT(std::fabs(chain.estimate(10 * v).matrix()(0, 3) - 0.2 * v) < 1e-8 && std::fabs(chain.estimate(10 * v).matrix()(1, 3)) < 1e-8);
  }
  std::printf("ok\n");
  return 0;
}
