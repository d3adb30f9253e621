// flatness::FlatnessMap facade: the reference's gcopter/flatness.hpp surface -- reset / forward / backward with the same argument
// order -- in front of the HIP kernels (anet_flat_forward / anet_flat_backward with a batch of one).  Vector arguments are
// duck-typed ((i) access): Eigen::Vector3d / Eigen::Vector4d work unchanged, anet::Vec3 and plain structs with operator() too;
// <Eigen/Eigen> is not needed to build against this header.
//
// One object = one state, like the reference; backward applies to the inputs of the last forward (the reference caches its
// intermediates in members; the kernel recomputes them from the cached inputs).  For batches, trajectories and the penalty of
// the MINCO objective call the C ABI (anet_flat_*_dev, anet_traj_flat_*, anet_minco_flat_partial_grads_dev) directly.
#pragma once
#include "core.hpp"

namespace flatness {

class FlatnessMap {
 public:
  inline void reset(const double &vehicle_mass, const double &gravitational_acceleration, const double &horizontal_drag_coeff,
                    const double &vertical_drag_coeff, const double &parasitic_drag_coeff, const double &speed_smooth_factor) {
    par.mass = vehicle_mass;
    par.grav = gravitational_acceleration;
    par.horiz_drag = horizontal_drag_coeff;
    par.vert_drag = vertical_drag_coeff;
    par.paras_drag = parasitic_drag_coeff;
    par.speed_eps = speed_smooth_factor;
  }

  // quat: (w, x, y, z)
  template <class V1, class V2, class V3, class Q, class O>
  inline void forward(const V1 &vel, const V2 &acc, const V3 &jer, const double &psi, const double &dpsi, double &thr, Q &quat,
                      O &omg) {
    for (int k = 0; k < 3; ++k) {
      in[k] = vel(k);
      in[3 + k] = acc(k);
      in[6 + k] = jer(k);
    }
    in[9] = psi;
    in[10] = dpsi;
    double q[4], o[3];
    anet::Context &ctx = anet::Context::thread_default();
    ctx.check(anet_flat_forward(ctx.get(), &par, 1, in, in + 3, in + 6, in + 9, in + 10, &thr, q, o));
    for (int k = 0; k < 4; ++k) quat(k) = q[k];
    for (int k = 0; k < 3; ++k) omg(k) = o[k];
  }

  template <class PG, class VG, class QG, class OG, class P, class V, class A, class J>
  inline void backward(const PG &pos_grad, const VG &vel_grad, const double &thr_grad, const QG &quat_grad, const OG &omg_grad,
                       P &pos_total_grad, V &vel_total_grad, A &acc_total_grad, J &jer_total_grad, double &psi_total_grad,
                       double &dpsi_total_grad) const {
    double pg[3], vg[3], qg[4], og[3], pt[3], vt[3], at[3], jt[3];
    for (int k = 0; k < 3; ++k) {
      pg[k] = pos_grad(k);
      vg[k] = vel_grad(k);
      og[k] = omg_grad(k);
    }
    for (int k = 0; k < 4; ++k) qg[k] = quat_grad(k);
    anet::Context &ctx = anet::Context::thread_default();
    ctx.check(anet_flat_backward(ctx.get(), &par, 1, in, in + 3, in + 6, in + 9, in + 10, pg, vg, &thr_grad, qg, og, pt, vt, at, jt,
                                 &psi_total_grad, &dpsi_total_grad));
    for (int k = 0; k < 3; ++k) {
      pos_total_grad(k) = pt[k];
      vel_total_grad(k) = vt[k];
      acc_total_grad(k) = at[k];
      jer_total_grad(k) = jt[k];
    }
  }

  // the six parameters as the C ABI takes them (the trajectory-level entry points: getBodyMargin, trajectory_map.hpp)
  inline const anet_flat_params &params() const { return par; }

 private:
  anet_flat_params par = {1.0, 9.8, 0.0, 0.0, 0.0, 1e-4};
  double in[11] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // vel, acc, jer, psi, dpsi of the last forward
};

}  // namespace flatness
