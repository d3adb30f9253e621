"""allocnet_amd -- MI355X-native batched MINCO / min-jerk / min-snap trajectory solver.

Host-side mirror (Python) of the reference's operator surface for the hot path; all arithmetic
runs in hand-written HIP kernels behind the C ABI in include/allocnet_amd.h.
"""
from ._lib import AnetError, load, LIB_PATH  # noqa: F401
from .context import Context, default_context  # noqa: F401
from .minco import MINCO, MINCO_S2NU, MINCO_S3NU, MINCO_S4NU, minco_solve, minco_solve_dev, bind_minco_solve, BoundMincoSolve, recommended_ld, minco_cost_grad, minco_cost_grad_dev, minco_cost_grad_launches, minco_piece_grad_shape, make_penalty, minco_sample_costs, minco_sample_costs_dev  # noqa: F401

from .trajectory import Piece, Trajectory, traj_eval, traj_cost, traj_cost_grad_T, traj_max_rate  # noqa: F401
from .trajectory import traj_row_margin, traj_qp_margins  # noqa: F401
from .trajectory import traj_voxel_hit, traj_voxel_hit_dev, traj_first_collision, HIT_FREE, HIT_OUTSIDE, HIT_INVALID  # noqa: F401
from .trajectory import traj_clearance, traj_clearance_dev  # noqa: F401
from .trajectory import traj_separation, traj_separation_dev  # noqa: F401
from . import lbfgs  # noqa: F401
from .lbfgs import (lbfgs_parameter_t, lbfgs_strerror, lbfgs_mvie, lbfgs_minco, lbfgs_minco_dev,  # noqa: F401
                    launch_order_from_counts, lbfgs_optimize_dev, lbfgs_optimize)
from . import qp  # noqa: F401
from .qp import (qp_assemble, qp_dims, qp_solve, qp_solve_vjp, qp_solve_dev, qp_solve_vjp_dev, qp_settings,  # noqa: F401
                 qp_ipm_launch_form, QPSolver, QPConfig)
from .min_traj_opt import MinTrajOpt, OsqpLayer  # noqa: F401
from . import firi as _firi_mod  # noqa: F401
from .firi import (firi, firi_dev, firi_params, convex_cover, polytope_depth, find_interior, overlap,  # noqa: F401
                   overlap_pt, short_cut, pack_model_inputs, to_planner_form)
from . import polytope  # noqa: F401
from .polytope import (polytope_vertices, polytope_vertices_dev, enumerate_vs, polytope_faces, polytope_volume,  # noqa: F401
                       corridor_vertices)
from . import sfc_opt  # noqa: F401
from .sfc_opt import (sfc_overlap_vertices, sfc_overlap_vertices_dev, sfc_forward_p, sfc_forward_p_dev,  # noqa: F401
                      sfc_backward_grad_p_dev, sfc_backward_p, sfc_backward_p_dev, lbfgs_minco_sfc, lbfgs_minco_sfc_dev,
                      sfc_default_max_verts, SFC_NO_OVERLAP, sfc_shortest_path, sfc_shortest_path_dev, sfc_path_cost_grad_dev, sfc_allot_pieces,
                      sfc_expand_corridor, sfc_route_waypoints, sfc_first_durations, sfc_setup)

from . import voxel_map  # noqa: F401
from .voxel_map import VoxelMap, gather_boxes_dev, distance_transform_dev, distance_query_dev, DIST_NONE  # noqa: F401
from .voxel_map import voxel_raycast_dev  # noqa: F401
from . import occupancy  # noqa: F401
from .occupancy import OccupancyMap, occupancy_params, depth_to_points_dev  # noqa: F401
from . import frontier  # noqa: F401
from .frontier import occupancy_frontier_dev, label_components_dev, component_stats_dev, view_gain_dev  # noqa: F401
from .frontier import frustum_points, frontier_clusters, candidate_views, next_view  # noqa: F401
from . import path_search  # noqa: F401
from .path_search import plan_path, plan_paths, PATH_EXACT, PATH_APPROXIMATE, PATH_INVALID_START  # noqa: F401
from . import flatness  # noqa: F401
from .flatness import (FlatnessMap, flat_forward, flat_forward_dev, flat_backward, flat_backward_dev,  # noqa: F401
                       traj_flat_states, traj_flat_extrema, make_flat_params, make_flat_penalty, minco_flat_cost_grad,
                       minco_flat_cost_grad_dev, minco_flat_partial_grads_dev)
from . import avoid  # noqa: F401
from .avoid import (AvoidOthers, make_avoid_penalty, minco_avoid_partial_grads_dev, minco_avoid_cost_grad_dev,  # noqa: F401
                    minco_avoid_cost_grad, neighbours_all, neighbours_from_pairs, upload_others, avoid_objective_dev)
from . import obstacle  # noqa: F401
from .obstacle import (make_obstacle_penalty, minco_obstacle_partial_grads_dev, minco_obstacle_cost_grad_dev,  # noqa: F401
                       minco_obstacle_cost_grad, obstacle_objective_dev)
from . import stop  # noqa: F401
from .stop import (make_stop_penalty, minco_stop_partial_grads_dev, minco_stop_cost_grad_dev, minco_stop_cost_grad,  # noqa: F401
                   stop_objective_dev, traj_stop_margin, traj_stop_margin_dev, traj_stop_check)
from . import yaw  # noqa: F401
from .yaw import (make_yaw_penalty, minco_solve_scalar, minco_solve_scalar_dev, minco_propagate_grad_scalar_dev,  # noqa: F401
                  minco_yaw_partial_grads_dev, minco_yaw_cost_grad, minco_yaw_cost_grad_dev, yaw_objective_dev, traj_yaw_margin,
                  traj_yaw_margin_dev, traj_flat_states_yaw, heading_waypoints, YawTrajectory)
from . import body  # noqa: F401
from .body import (make_body_penalty, box_body, minco_body_partial_grads_dev, minco_body_cost_grad_dev,  # noqa: F401
                   minco_body_cost_grad, body_objective_dev, traj_body_margin, traj_body_margin_dev)
from . import time_net  # noqa: F401
from .time_net import TimeAllocNet  # noqa: F401
from . import learning_planner  # noqa: F401
from .learning_planner import LearningPlanner, LearningPlannerConfig  # noqa: F401

__version__ = "0.1.0"
