// Source-compatible stand-in for the reference's planner/learning_planner.hpp (class LearningPlanner, :16-307): loadModel,
// plan, callModel, getTraj, gethPolys, with the route search, the corridor, the network and the QP on the MI355X behind the
// C ABI.  No ROS, no Eigen, no libtorch: the constructor takes a LearningPlannerConfig instead of a node handle, the model is
// the flat weights file of time_net.hpp instead of a TorchScript archive, and matrix arguments are duck-typed ((r,c) / (i)
// access; polytopes also rows() and resize(r, 4); points a (x, y, z) constructor), so Eigen types work unchanged.
#pragma once
#include <cstdio>
#include <string>
#include <vector>

#include "qp_solver.hpp"
#include "sfc_gen_map.hpp"
#include "time_net.hpp"
#include "trajectory.hpp"

struct LearningPlannerConfig {
  int ModelMaxSeg = 5;
  int OptOrder = 4;  // 3: jerk (Trajectory<5>), otherwise snap (Trajectory<7>), as the reference branches (:203)
  QPConfig qp;
  double StopThreshold = 0.5;  // the exported model's stop-token threshold (fixed inside the TorchScript in the reference)

  LearningPlannerConfig() = default;
  LearningPlannerConfig(int modelMaxSeg, int optOrder, const QPConfig &qpConfig = QPConfig(), double stopThreshold = 0.5)
      : ModelMaxSeg(modelMaxSeg), OptOrder(optOrder), qp(qpConfig), StopThreshold(stopThreshold) {}
};

class LearningPlanner {
 public:
  // a polytope: rows [a b c d], raw form h . [x 1] <= 0 in vishPolys, planner form a . x <= d (unit normals) in hPolys
  struct HPoly {
    std::vector<double> a;
    long rows_ = 0;
    long rows() const { return rows_; }
    long cols() const { return 4; }
    void resize(long r, long) {
      rows_ = r;
      a.assign((size_t)r * 4, 0.0);
    }
    double &operator()(long r, long c) { return a[(size_t)r * 4 + c]; }
    double operator()(long r, long c) const { return a[(size_t)r * 4 + c]; }
  };

 private:
  LearningPlannerConfig config;
  QPSolver qp_solver;
  anet::TimeAllocNet net;
  size_t seg = 0;
  std::vector<HPoly> hPolys, vishPolys;
  Trajectory<5> jerk_traj;
  Trajectory<7> snap_traj;
  std::vector<float> times_;

  struct TimesView {  // times(i), as the reference's Eigen::Map<Eigen::VectorXf>
    const std::vector<float> &t;
    float operator()(long i) const { return t[(size_t)i]; }
  };
  struct Solution {  // qp_solution.resize(n), (i)
    std::vector<double> a;
    void resize(long n) { a.assign((size_t)n, 0.0); }
    double &operator()(long i) { return a[(size_t)i]; }
    double operator()(long i) const { return a[(size_t)i]; }
  };

 public:
  explicit LearningPlanner(const LearningPlannerConfig &conf) : config(conf), qp_solver(conf.qp) {
    qp_solver.setOrder(config.OptOrder);
  }

  template <class Poly>
  inline void gethPolys(std::vector<Poly> &plys) const {
    plys.clear();
    for (const HPoly &h : vishPolys) {
      Poly p;
      p.resize(h.rows(), 4);
      for (long r = 0; r < h.rows(); ++r)
        for (int c = 0; c < 4; ++c) p(r, c) = h(r, c);
      plys.emplace_back(p);
    }
  }
  inline void getTraj(Trajectory<5> &traj) const { traj = jerk_traj; }
  inline void getTraj(Trajectory<7> &traj) const { traj = snap_traj; }
  // the network's last output: seq_len times, zero after the count
  inline const std::vector<float> &getTimes() const { return times_; }

  // Extension: the corridor callModel works on, in planner form (plan() sets it from the map)
  template <class Poly>
  inline void setCorridor(const std::vector<Poly> &polys) {
    hPolys.clear();
    for (const Poly &p : polys) {
      HPoly h;
      h.resize((long)p.rows(), 4);
      for (long r = 0; r < h.rows(); ++r)
        for (int c = 0; c < 4; ++c) h(r, c) = p(r, c);
      hPolys.emplace_back(h);
    }
    seg = hPolys.size();
  }

  inline bool loadModel(const std::string &modelPath) {
    try {
      net.load(modelPath);
    } catch (const anet::Error &e) {
      std::fprintf(stderr, "error loading the model\nError: %s\n", e.what());
      return false;
    }
    if (net.seq_len() != config.ModelMaxSeg) {
      std::fprintf(stderr, "error loading the model\nError: the model takes %d polytopes, ModelMaxSeg is %d\n", net.seq_len(),
                   config.ModelMaxSeg);
      return false;
    }
    return true;
  }

  template <class MatA, class MatB>
  inline bool callModel(const MatA &iniPVA, const MatB &finPVA) {
    const int L = config.ModelMaxSeg;
    if (!net.loaded()) throw anet::Error(ANET_ERR_INVALID, "LearningPlanner::callModel before loadModel");
    if ((int)seg > L) return false;
    // stacked_state {1, 9, 2}: rows px, vx, ax, py, ..; column 0 start, column 1 end.  stacked_hpolys {1, 50, 4, L}
    float state[18];
    for (int a = 0; a < 3; ++a)
      for (int j = 0; j < 3; ++j) {
        state[(a * 3 + j) * 2] = (float)iniPVA(a, j);
        state[(a * 3 + j) * 2 + 1] = (float)finPVA(a, j);
      }
    std::vector<float> hp((size_t)ANET_MAX_POLY_ROWS * 4 * L, 0.0f);
    for (size_t i = 0; i < seg; ++i) {
      if (hPolys[i].rows() > ANET_MAX_POLY_ROWS) {
        std::fprintf(stderr, "polytope %zu has %ld rows, the model takes %d\n", i, hPolys[i].rows(), ANET_MAX_POLY_ROWS);
        return false;
      }
      for (long r = 0; r < hPolys[i].rows(); ++r)
        for (int c = 0; c < 4; ++c) hp[((size_t)r * 4 + c) * L + i] = (float)hPolys[i](r, c);
    }
    times_.assign((size_t)L, 0.0f);
    int32_t count = 0;
    net.forward(1, state, hp.data(), config.StopThreshold, times_.data(), &count);
    for (size_t i = 0; i < seg; i++)
      if (times_[i] < 1e-10) {
        std::printf("time and seg does not fit, the segment is%zu\n", seg);
        return false;
      }
    Solution flatten_coffmats;
    const TimesView times{times_};
    if (!qp_solver.solve(iniPVA, finPVA, hPolys, times, flatten_coffmats)) return false;
    // p(t) = c5*t^5 + c4*t^4 + ... + c1*t + c0
    if (config.OptOrder == 3) {
      jerk_traj.clear();
      jerk_traj.reserve((int)seg);
      fill(jerk_traj, flatten_coffmats);
    } else {
      snap_traj.clear();
      snap_traj.reserve((int)seg);
      fill(snap_traj, flatten_coffmats);
    }
    return true;
  }

  template <typename Map, class MatA, class MatB, class V3>
  inline bool plan(MatA &iniState, MatB &finState, std::vector<V3> &route, Map &mapPtr) {
    const anet::Vec3 o = mapPtr.getOrigin(), c = mapPtr.getCorner();
    const V3 lo(o(0), o(1), o(2)), hi(c(0), c(1), c(2));
    if (route.size() <= 0) {
      const V3 s(iniState(0, 0), iniState(1, 0), iniState(2, 0)), g(finState(0, 0), finState(1, 0), finState(2, 0));
      sfc_gen::planPath(s, g, lo, hi, &mapPtr, 0.01, route);
      if (route.size() <= 0) return false;
    }
    for (int a = 0; a < 3; ++a) finState(a, 0) = route.back()(a);

    /* corridor generation */
    hPolys.clear();
    vishPolys.clear();
    sfc_gen::convexCover(route, mapPtr, lo, hi, 7.0, 3.0, vishPolys);
    sfc_gen::shortCut(vishPolys);
    hPolys = vishPolys;
    seg = hPolys.size();
    if ((int)seg > config.ModelMaxSeg) {
      std::printf("give up this try, long corridor \n");
      return false;
    }
    for (size_t i = 0; i < seg; i++)
      for (long r = 0; r < hPolys[i].rows(); ++r) {
        HPoly &h = hPolys[i];
        const double norm = std::sqrt(h(r, 0) * h(r, 0) + h(r, 1) * h(r, 1) + h(r, 2) * h(r, 2));
        for (int k = 0; k < 4; ++k) h(r, k) /= norm;
        h(r, 3) = -h(r, 3);  // to make it work
      }
    return callModel(iniState, finState);
  }

 private:
  template <int D>
  inline void fill(Trajectory<D> &traj, const Solution &sol) {
    anet::Matrix<3, D + 1> coffMat;
    for (size_t i = 0; i < seg; i++) {
      for (int j = 0; j < 3; j++)
        for (int k = 0; k <= D; ++k) coffMat(j, k) = sol((long)(i * 3 * (D + 1) + j * (D + 1) + k));
      traj.emplace_back((double)times_[i], coffMat);
    }
  }
};
