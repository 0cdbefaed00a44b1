// dvo_slam::PoseGraph::optimizeBatch (include/dvo_slam/pose_graph.h): many small graphs in one launch.
// usage: pose_graph_batch_facade_check host | device
//  host: what needs no device -- an empty list, a null entry, a graph without vertices, the same graph twice and a wrong number of
//        parameter sets are refused before anything is uploaded;
//  device: three chains of different lengths, one with a false edge under the kernel, optimised in one batch: every estimate, chi2 and
//        weight equals, bit for bit, what optimize() gives on a copy of the same graph; a graph beyond 1024 vertices is refused.
// Prints "ok" or the first mismatch.
#include <cstdio>
#include <cstring>
#include <vector>

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

// a chain of `n` vertices 0.2 apart, started up to 1 cm off, with edges to the next and the next but one; `planted`: a false edge too
int chain(dvo_slam::PoseGraph& g, int n, bool planted) {
  for (int v = 0; v < n; ++v) g.addVertex(10 * v, shift(0.2 * v + 0.01 * (v % 3), 0.005 * (v % 2), 0), v == 0);
  int id = 0;
  for (int v = 0; v + 1 < n; ++v) g.addEdge(id++, 10 * v, 10 * (v + 1), shift(0.2, 0, 0), information(1e4), 5.0);
  for (int v = 0; v + 2 < n; ++v) g.addEdge(id++, 10 * v, 10 * (v + 2), shift(0.4, 0, 0), information(1e4), 5.0);
  if (planted) g.addEdge(id++, 0, 10 * (n - 1), shift(0.8, 1.0, 0), information(1e4), 5.0);
  return id;
}

#define EXPECT(cond)                                      \
  if (!(cond)) {                                          \
    std::printf("line %d: %s\n", __LINE__, #cond);        \
    return 1;                                             \
  }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: pose_graph_batch_facade_check host|device\n"); return 2; }
  const bool device = std::strcmp(argv[1], "device") == 0;

  dvo_slam::PoseGraph a, b, empty;
  chain(a, 5, true);
  chain(b, 9, false);
  std::vector<dvo_slam::PoseGraph*> none, with_null, with_empty, twice, pair;
  with_null.push_back(&a); with_null.push_back(0);
  with_empty.push_back(&a); with_empty.push_back(&empty);
  twice.push_back(&a); twice.push_back(&b); twice.push_back(&a);
  pair.push_back(&a); pair.push_back(&b);
  EXPECT(dvo_slam::PoseGraph::optimizeBatch(none) == -1 && dvo_slam::PoseGraph::optimizeBatch(with_null, 30) == -1);
  EXPECT(dvo_slam::PoseGraph::optimizeBatch(with_empty) == -1 && dvo_slam::PoseGraph::optimizeBatch(twice, 30) == -1);
  EXPECT(dvo_slam::PoseGraph::optimizeBatch(pair, std::vector<dvo_hip_graph_params>(3, dvo_hip_graph_params_default())) == -1);
  EXPECT(a.estimate(10).matrix()(0, 3) == 0.2 + 0.01 && a.chi2(0) == 0.0);

  if (device) {
    EXPECT(dvo_hip_device_count() > 0);
    const int sizes[3] = {5, 9, 300};
    dvo_slam::PoseGraph batch[3], solo[3];
    int edges[3];
    std::vector<dvo_slam::PoseGraph*> all;
    for (int k = 0; k < 3; ++k) {
      edges[k] = chain(batch[k], sizes[k], k == 0);
      chain(solo[k], sizes[k], k == 0);
      all.push_back(&batch[k]);
    }
    EXPECT(dvo_slam::PoseGraph::optimizeBatch(all, 30) == 3);
    for (int k = 0; k < 3; ++k) {
      EXPECT(solo[k].optimize(30) == batch[k].report().iterations && batch[k].report().iterations >= 1);
      EXPECT(std::memcmp(&solo[k].report(), &batch[k].report(), sizeof(dvo_hip_graph_report)) == 0);
      EXPECT(batch[k].report().final_cost < batch[k].report().initial_cost);
      for (int v = 0; v < sizes[k]; ++v) {
        const AffineTransformd x = batch[k].estimate(10 * v), y = solo[k].estimate(10 * v);
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) {
            const double p = x.matrix()(r, c), q = y.matrix()(r, c);
            EXPECT(std::memcmp(&p, &q, sizeof(double)) == 0);
          }
      }
      for (int e = 0; e < edges[k]; ++e) EXPECT(batch[k].chi2(e) == solo[k].chi2(e) && batch[k].robustWeight(e) == solo[k].robustWeight(e));
    }
    EXPECT(batch[0].robustWeight(edges[0] - 1) < 0.01);
    // per-graph parameters: one trial for the first, the defaults for the others
    std::vector<dvo_hip_graph_params> each(3, dvo_hip_graph_params_default());
    each[0].max_iterations = 1;
    EXPECT(dvo_slam::PoseGraph::optimizeBatch(all, each) == 3 && batch[0].report().iterations == 1);
    // beyond the resident size: refused, and the graphs of the list stay as they are
    dvo_slam::PoseGraph large;
    chain(large, 1025, false);
    const double before = batch[1].estimate(10).matrix()(0, 3);
    all.push_back(&large);
    EXPECT(dvo_slam::PoseGraph::optimizeBatch(all, 30) == -1 && batch[1].estimate(10).matrix()(0, 3) == before);
    EXPECT(large.optimize(2) >= 1);
  }
  std::printf("ok\n");
  return 0;
}
