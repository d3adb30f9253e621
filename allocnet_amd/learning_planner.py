"""Host mirror of class LearningPlanner (planner/learning_planner.hpp): loadModel, plan, callModel, getTraj, gethPolys, and the
batched form of callModel the reference lacks.  Route, corridor, network and QP all run on the device through the package's
own entry points; this file only strings them together the way learning_planner.hpp:140-306 does."""
import os

import numpy as np

from .firi import convex_cover, pack_model_inputs, short_cut, to_planner_form
from .path_search import plan_path
from .qp import QP_METHOD_INTERIOR_POINT, QPConfig, QPSolver, qp_settings, qp_solve
from .time_net import MAGIC, TimeAllocNet
from .trajectory import Trajectory

MIN_TIME = 1e-10            # learning_planner.hpp:183: a time below this among the first `seg` means "time and seg does not fit"


class LearningPlannerConfig:
    """The parameters the reference's constructor reads from the node handle (ModelMaxSeg, OptOrder, the QPConfig), and the stop
    threshold of the network, which the reference fixes inside the exported model (0.5)."""

    def __init__(self, ModelMaxSeg=5, OptOrder=4, qp=None, StopThreshold=0.5):
        self.ModelMaxSeg, self.OptOrder, self.StopThreshold = int(ModelMaxSeg), int(OptOrder), float(StopThreshold)
        self.QPConfig = qp if qp is not None else QPConfig()


def _accepted(out, b):
    """QPSolver::solve's rule (qp_solver.hpp:334-352): status Solved and the objective, read into a float, in [-0.01, 5000]."""
    result = float(np.float32(out["obj"][b]))
    return not (result > 5000 or result < -0.01 or out["status"][b] != 1)


def group_by_seg(segs, keep):
    """{seg: indices of the kept problems with that many polytopes, ascending}, by ascending seg: the groups `qp_solve` needs."""
    groups = {}
    for b in range(len(segs)):
        if keep[b]:
            groups.setdefault(int(segs[b]), []).append(b)
    return {s: groups[s] for s in sorted(groups)}


def stack_group(polys, idx, seg):
    """(len(idx), seg, M, 4) with zero rows as padding, M the most rows of any polytope of the group."""
    M = max(1, max(np.asarray(p).shape[0] for b in idx for p in polys[b]))
    hp = np.zeros((len(idx), seg, M, 4))
    for r, b in enumerate(idx):
        for i, p in enumerate(polys[b]):
            p = np.asarray(p, dtype=np.float64)
            hp[r, i, :p.shape[0]] = p
    return hp


class LearningPlanner:
    def __init__(self, config=None, ctx=None):
        self.config = config if config is not None else LearningPlannerConfig()
        if self.config.OptOrder not in (3, 4):
            raise ValueError("OptOrder must be 3 (jerk) or 4 (snap)")
        self._ctx = ctx
        self.net = None
        self.qp_solver = QPSolver(self.config.QPConfig, ctx=ctx)
        self.qp_solver.setOrder(self.config.OptOrder)
        self.hPolys, self.vishPolys = [], []
        self.traj = Trajectory(ctx=ctx)
        self.times = None

    # ---- the reference's interface ----------------------------------------------------------------
    def loadModel(self, modelPath):
        """The package's weights file (`TimeAllocNet.save`), or an exported TorchScript model, whose weights are read.  False
        when the file is missing or unreadable, or made for another ModelMaxSeg (learning_planner.hpp:58-80)."""
        if not os.path.isfile(modelPath):
            print("Model file not found")
            return False
        try:
            with open(modelPath, "rb") as f:
                own = f.read(len(MAGIC)) == MAGIC
            net = TimeAllocNet.load(modelPath, self._ctx) if own else TimeAllocNet.from_torchscript(modelPath, self._ctx)
        except Exception as e:  # noqa: BLE001 -- the reference reports and returns false
            print(f"error loading the model\nError: {e}")
            return False
        if net.seq_len != self.config.ModelMaxSeg:
            print(f"error loading the model\nError: the model takes {net.seq_len} polytopes, ModelMaxSeg is {self.config.ModelMaxSeg}")
            return False
        self.net = net
        return True

    def gethPolys(self):
        return [p.copy() for p in self.vishPolys]

    def getTraj(self):
        return self.traj

    def callModel(self, iniPVA, finPVA):
        """learning_planner.hpp:140-240 on self.hPolys (planner form): network, the check of the first `seg` times, QP, trajectory."""
        if self.net is None:
            raise RuntimeError("callModel before loadModel")
        seg = len(self.hPolys)
        try:
            state, corridor = pack_model_inputs(iniPVA, finPVA, self.hPolys, max_seg=self.config.ModelMaxSeg)
        except ValueError as e:      # more polytopes or rows than the model's tensor holds (the reference writes past its matrix)
            print(e)
            return False
        times, _ = self.net.forward(state, corridor, threshold=self.config.StopThreshold)
        self.times = times
        if (times[:seg] < MIN_TIME).any():
            print(f"time and seg does not fit, the segment is {seg}")
            return False
        ok, flat = self.qp_solver.solve(iniPVA, finPVA, self.hPolys, times)     # times(i), i < seg: the corridor's length
        if not ok:
            return False
        self.traj = self._fill(times, np.asarray(flat), seg)
        return True

    def plan(self, iniState, finState, route, voxel_map):
        """learning_planner.hpp:243-306.  iniState, finState: (3, 3) arrays, columns p, v, a; finState[:, 0] becomes route[-1].
        route: a list of points, filled by `plan_path` when empty (as the reference fills its argument)."""
        vm = voxel_map
        if len(route) <= 0:
            _, path = plan_path(np.asarray(iniState)[:, 0], np.asarray(finState)[:, 0], vm.getOrigin(), vm.getCorner(), vm, 0.01)
            route.extend(np.asarray(p, dtype=np.float64) for p in path)
            if len(route) <= 0:
                return False
        finState[:, 0] = route[-1]
        self.hPolys, self.vishPolys = [], []
        polys = convex_cover(route, vm, vm.getOrigin(), vm.getCorner(), 7.0, 3.0)
        self.vishPolys = short_cut(polys)
        seg = len(self.vishPolys)
        if seg > self.config.ModelMaxSeg:
            print("give up this try, long corridor ")
            return False
        rows = [len(p) for p in self.vishPolys]
        raw = np.zeros((seg, max(rows), 4))
        for i, p in enumerate(self.vishPolys):
            raw[i, :rows[i]] = p
        hp = to_planner_form(raw, rows)
        self.hPolys = [hp[i, :rows[i]] for i in range(seg)]
        return self.callModel(iniState, finState)

    # ---- the batched form ---------------------------------------------------------------------------
    def call_model_batch(self, iniPVA, finPVA, corridors):
        """callModel for B problems: iniPVA, finPVA (B, 3, 3); corridors: B lists of (m_i, 4) polytopes in planner form.  One
        network call, then one `qp_solve` per corridor length over the problems whose first `seg` times passed the check.
        Returns (ok (B,) bool, trajectories [Trajectory or None], times (B, L))."""
        if self.net is None:
            raise RuntimeError("call_model_batch before loadModel")
        ini = np.asarray(iniPVA, dtype=np.float64); fin = np.asarray(finPVA, dtype=np.float64)
        B = len(corridors)
        if ini.shape != (B, 3, 3) or fin.shape != (B, 3, 3):
            raise ValueError("iniPVA, finPVA (B, 3, 3) and B corridors expected")
        ok = np.zeros(B, dtype=bool)
        trajs = [None] * B
        if B == 0:
            return ok, trajs, np.zeros((0, self.net.seq_len), dtype=np.float32)
        packed = [pack_model_inputs(ini[b], fin[b], corridors[b], max_seg=self.config.ModelMaxSeg) for b in range(B)]
        times, _ = self.net.forward(np.stack([p[0] for p in packed]), np.stack([p[1] for p in packed]),
                                    threshold=self.config.StopThreshold)
        segs = [len(c) for c in corridors]
        keep = [segs[b] >= 1 and not (times[b, :segs[b]] < MIN_TIME).any() for b in range(B)]
        conf = self.config.QPConfig
        for seg, idx in group_by_seg(segs, keep).items():
            out = qp_solve(self.config.OptOrder, ini[idx], fin[idx], stack_group(corridors, idx, seg),
                           times[idx, :seg].astype(np.float64), res=conf.ConstRes, max_vel=conf.MaxVelBox, max_acc=conf.MaxAccBox,
                           settings=qp_settings(method=QP_METHOD_INTERIOR_POINT), ctx=self._ctx)
            for r, b in enumerate(idx):
                if _accepted(out, r):
                    ok[b] = True
                    trajs[b] = self._fill(times[b], out["coeffs"][r].reshape(-1), seg)
        return ok, trajs, times

    def _fill(self, times, flat, seg):
        """learning_planner.hpp:201-233: piece i gets times(i) and rows j of its coefficient block, highest power first."""
        D = 2 * self.config.OptOrder
        co = flat.reshape(seg, 3, D)
        traj = Trajectory(ctx=self._ctx)
        traj.reserve(seg)
        for i in range(seg):
            traj.emplace_back(float(times[i]), co[i])
        return traj
