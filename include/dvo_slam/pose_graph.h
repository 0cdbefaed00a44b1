// dvo_slam/pose_graph.h -- the back end's pose graph, optimised on the device.
//
// What the reference does with a g2o::SparseOptimizer of VertexSE3 / EdgeSE3 (dvo_slam/src/keyframe_graph.cpp:256-285: the solver
// set-up; 620-636: addEdge with the Cauchy kernel of 840-845; 643-674: removeOutlierConstraints; 475-489: initializeOptimization + optimize), as
// far as the engine replaces it: vertices and edges are kept on the host under the caller's ids, mapped to dense indices (vertices
// in ascending id, edges in ascending id: the order of the device's sums), and optimize() hands them to dvo_hip_graph_* (include/dvo_hip.h;
// DESIGN.md section 12) and reads the poses back.  The information matrix is taken as given, translation rows first, exactly as the
// reference hands Result.Information to setInformation (keyframe_graph.cpp:628).  Not g2o: no other vertex or edge types, no
// marginals, Levenberg-Marquardt with a preconditioned conjugate-gradient solve only.
#pragma once

#include <algorithm>
#include <cstdint>
#include <iterator>
#include <map>
#include <utility>
#include <vector>

#include "dvo/core/rgbd_image.h"

namespace dvo_slam {

class PoseGraph {
 public:
  explicit PoseGraph(dvo_hip_context* ctx = 0) : ctx_(ctx), graph_(0), dirty_(true) {}
  ~PoseGraph() {
    if (graph_) dvo_hip_graph_destroy(ctx_, graph_);
  }
  PoseGraph(const PoseGraph&) = delete;
  PoseGraph& operator=(const PoseGraph&) = delete;

  // false: the id is taken (addVertex, addEdge) or unknown (the others)
  bool addVertex(int id, const dvo::core::AffineTransformd& pose, bool fixed = false) {
    if (vertices_.count(id)) return false;
    Vertex v;
    v.pose = pose;
    v.fixed = fixed;
    vertices_[id] = v;
    dirty_ = true;
    return true;
  }
  // delta: the width of the edge's Cauchy kernel, 0 = none (keyframe_graph.cpp:840-845)
  bool addEdge(int id, int from, int to, const dvo::core::AffineTransformd& measurement, const dvo::core::Matrix6d& information, double delta = 0.0) {
    if (edges_.count(id) || !vertices_.count(from) || !vertices_.count(to) || from == to || !(delta >= 0.0)) return false;
    Edge e;
    e.from = from;
    e.to = to;
    e.measurement = measurement;
    e.information = information;
    e.delta = delta;
    e.chi2 = 0.0;
    e.weight = 1.0;
    edges_[id] = e;
    dirty_ = true;
    return true;
  }
  bool removeEdge(int id) {
    dirty_ = true;
    return edges_.erase(id) == 1;
  }
  bool setFixed(int id, bool fixed) {
    std::map<int, Vertex>::iterator it = vertices_.find(id);
    if (it == vertices_.end()) return false;
    it->second.fixed = fixed;
    dirty_ = true;
    return true;
  }
  bool setEstimate(int id, const dvo::core::AffineTransformd& pose) {
    std::map<int, Vertex>::iterator it = vertices_.find(id);
    if (it == vertices_.end()) return false;
    it->second.pose = pose;
    dirty_ = true;
    return true;
  }
  size_t numVertices() const { return vertices_.size(); }
  size_t numEdges() const { return edges_.size(); }
  bool hasVertex(int id) const { return vertices_.count(id) == 1; }
  bool hasEdge(int id) const { return edges_.count(id) == 1; }
  // the dense index the device knows a vertex / an edge by: its rank among the ids; -1 for an unknown id
  int vertexIndex(int id) const { return rank(vertices_, id); }
  int edgeIndex(int id) const { return rank(edges_, id); }

  const dvo::core::AffineTransformd& estimate(int id) const { return vertices_.at(id).pose; }
  // e^T Omega e and the kernel's weight as the last optimize() or computeErrors() left them (g2o: chi2(), robustKernel()->robustify)
  double chi2(int edge) const { return edges_.at(edge).chi2; }
  double robustWeight(int edge) const { return edges_.at(edge).weight; }

  // optimize(iterations) of the reference: at most that many Levenberg-Marquardt trials; returns the trials run, -1 on an error
  // (message: dvo_hip_last_error).  report(): what the last call did.
  int optimize(int iterations) {
    dvo_hip_graph_params p = dvo_hip_graph_params_default();
    p.max_iterations = iterations;
    return optimize(p);
  }
  int optimize(const dvo_hip_graph_params& params) {
    if (vertices_.empty() || !upload()) return -1;
    if (dvo_hip_graph_optimize(ctx_, graph_, &params, &report_, 0, 0) != DVO_HIP_OK) return -1;
    return download() ? report_.iterations : -1;
  }
  // Many small graphs in ONE launch, one workgroup each (dvo_hip_graph_optimize_batch): the local maps of several trackers, or several
  // edge subsets of one graph held as graphs of their own.  Every graph is left as its own optimize() would have left it, bit for bit.
  // Each graph once, none null, all on one context, each within 1024 vertices and 4096 edges; params: one set for all, or one per
  // graph.  Returns the number of graphs optimised, -1 on an error (nothing has been optimised then).
  static int optimizeBatch(const std::vector<PoseGraph*>& graphs, int iterations) {
    dvo_hip_graph_params p = dvo_hip_graph_params_default();
    p.max_iterations = iterations;
    return optimizeBatch(graphs, std::vector<dvo_hip_graph_params>(1, p));
  }
  static int optimizeBatch(const std::vector<PoseGraph*>& graphs, const std::vector<dvo_hip_graph_params>& params = std::vector<dvo_hip_graph_params>()) {
    const size_t count = graphs.size();
    if (count == 0 || (params.size() > 1 && params.size() != count)) return -1;
    for (size_t i = 0; i < count; ++i) {
      if (!graphs[i] || graphs[i]->vertices_.empty()) return -1;
      for (size_t k = 0; k < i; ++k)
        if (graphs[k] == graphs[i]) return -1;
    }
    std::vector<dvo_hip_graph*> handles(count);
    for (size_t i = 0; i < count; ++i) {
      if (!graphs[i]->upload() || graphs[i]->ctx_ != graphs[0]->ctx_) return -1;
      handles[i] = graphs[i]->graph_;
    }
    std::vector<dvo_hip_graph_params> each(params);
    if (each.size() == 1) each.assign(count, params[0]);
    std::vector<dvo_hip_graph_report> reports(count);
    if (dvo_hip_graph_optimize_batch(graphs[0]->ctx_, int(count), handles.data(), each.empty() ? 0 : each.data(), reports.data(), 0, 0) != DVO_HIP_OK) return -1;
    for (size_t i = 0; i < count; ++i) {
      graphs[i]->report_ = reports[i];
      if (!graphs[i]->download()) return -1;
    }
    return int(count);
  }
  // chi2 and weights at the current estimates, without a step
  bool computeErrors() {
    if (vertices_.empty() || !upload()) return false;
    return download();
  }
  const dvo_hip_graph_report& report() const { return report_; }

  // removeOutlierConstraints (keyframe_graph.cpp:643-674): among the edges with a kernel, those whose weight is below the threshold
  // leave the graph, lowest weight first, at most n_max (-1: all).  Returns their ids.
  std::vector<int> removeOutlierConstraints(double weight_threshold, int n_max = -1) {
    std::vector<std::pair<double, int> > candidates;
    for (std::map<int, Edge>::const_iterator it = edges_.begin(); it != edges_.end(); ++it)
      if (it->second.delta > 0.0 && it->second.weight < weight_threshold) candidates.push_back(std::make_pair(it->second.weight, it->first));
    std::stable_sort(candidates.begin(), candidates.end());
    std::vector<int> gone;
    for (size_t i = 0; i < candidates.size() && (n_max < 0 || int(i) < n_max); ++i) {
      gone.push_back(candidates[i].second);
      removeEdge(candidates[i].second);
    }
    return gone;
  }

 private:
  struct Vertex {
    dvo::core::AffineTransformd pose;
    bool fixed;
  };
  struct Edge {
    int from, to;
    dvo::core::AffineTransformd measurement;
    dvo::core::Matrix6d information;
    double delta, chi2, weight;
  };

  template <typename M>
  static int rank(const M& m, int id) {
    typename M::const_iterator it = m.find(id);
    return it == m.end() ? -1 : int(std::distance(m.begin(), it));
  }

  bool upload() {
    if (!ctx_) ctx_ = dvo::core::DeviceContext::current();
    if (!ctx_) return false;
    if (!graph_ && dvo_hip_graph_create(ctx_, &graph_) != DVO_HIP_OK) return false;
    if (!dirty_) return true;
    const int n = int(vertices_.size()), m = int(edges_.size());
    std::vector<double> poses(size_t(n) * 16), Z(size_t(m) * 16), W(size_t(m) * 36), delta(size_t(m), 0.0);
    std::vector<unsigned char> fixed(static_cast<size_t>(n), 0);
    std::vector<int32_t> from(static_cast<size_t>(m), 0), to(static_cast<size_t>(m), 0);
    size_t at = 0;
    for (std::map<int, Vertex>::const_iterator it = vertices_.begin(); it != vertices_.end(); ++it, ++at) {
      dvo::compat::affine_to_rowmajor(it->second.pose, &poses[at * 16]);
      fixed[at] = it->second.fixed ? 1 : 0;
    }
    at = 0;
    for (std::map<int, Edge>::const_iterator it = edges_.begin(); it != edges_.end(); ++it, ++at) {
      from[at] = vertexIndex(it->second.from);
      to[at] = vertexIndex(it->second.to);
      dvo::compat::affine_to_rowmajor(it->second.measurement, &Z[at * 16]);
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) W[at * 36 + size_t(r * 6 + c)] = it->second.information(r, c);
      delta[at] = it->second.delta;
    }
    if (dvo_hip_graph_set_vertices(ctx_, graph_, n, poses.data(), fixed.data()) != DVO_HIP_OK) return false;
    if (dvo_hip_graph_set_edges(ctx_, graph_, m, from.data(), to.data(), Z.data(), W.data(), delta.data()) != DVO_HIP_OK) return false;
    dirty_ = false;
    return true;
  }

  bool download() {
    const int n = int(vertices_.size()), m = int(edges_.size());
    std::vector<double> poses(size_t(n) * 16), chi2(static_cast<size_t>(m)), weight(static_cast<size_t>(m));
    if (dvo_hip_graph_get_poses(ctx_, graph_, n, poses.data()) != DVO_HIP_OK) return false;
    if (dvo_hip_graph_edge_stats(ctx_, graph_, m, chi2.data(), weight.data()) != DVO_HIP_OK) return false;
    size_t at = 0;
    for (std::map<int, Vertex>::iterator it = vertices_.begin(); it != vertices_.end(); ++it, ++at)
      dvo::compat::affine_from_rowmajor(&poses[at * 16], it->second.pose);
    at = 0;
    for (std::map<int, Edge>::iterator it = edges_.begin(); it != edges_.end(); ++it, ++at) {
      it->second.chi2 = chi2[at];
      it->second.weight = weight[at];
    }
    return true;
  }

  dvo_hip_context* ctx_;
  dvo_hip_graph* graph_;
  bool dirty_;
  std::map<int, Vertex> vertices_;
  std::map<int, Edge> edges_;
  dvo_hip_graph_report report_ = dvo_hip_graph_report();
};

}  // namespace dvo_slam
