"""What every anet_*_workspace function returns over a fixed list of shapes: tests/golden/workspace_sizes.json.

    python tools/record_workspace_sizes.py            print {function: [[arguments..., size], ...]} as JSON
    python tools/record_workspace_sizes.py --write    the same into tests/golden/workspace_sizes.json

The fixture was recorded before the layouts moved to csrc/workspace.h and is recorded again only when a workspace is meant to
change size.  The functions need no device.  Run it with the ANET_* switches unset: tuning() reads them once per process and
ANET_LBFGS_SPLIT_EVALS / ANET_LBFGS_SPLIT_MIN_VARS enter anet_lbfgs_minco_workspace (tests/test_workspace_layout_cpu.py starts
it in a child process with a cleaned environment).  cases() is the one list of shapes: the test feeds the same list, with the
recorded sizes, to tests/cpp/test_workspace_layout.cpp.
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")

BATCHES = [1, 3, 63, 64, 65, 577]      # batch or row stride; odd values: int32 rows padded to whole doubles
PIECES = [1, 2, 8, 10, 16]
MEM, PAST = [1, 8, 18], [0, 1, 3]
GRIDS = [(1, 1, 1), (7, 6, 4), (33, 17, 9), (64, 64, 16)]


def cases():
    """{function: [argument tuple, ...]}; L-BFGS parameters as (mem_size, past), a voxel grid as its three sizes"""
    p = itertools.product
    return {
        "anet_minco_cost_grad_workspace": list(p([2, 3, 4], PIECES, BATCHES)),
        "anet_qp_solve_workspace": list(p([3, 4], PIECES, BATCHES, [1, 8], [0, 5, 12])),
        "anet_lbfgs_workspace": list(p([1, 9, 29, 64], BATCHES, MEM, PAST)),
        "anet_lbfgs_minco_workspace": list(p([2, 3, 4], PIECES, BATCHES, MEM, PAST)),
        "anet_firi_workspace": list(p(BATCHES, [0, 1, 7], [4, 30])),
        "anet_voxel_workspace": list(GRIDS),
        "anet_voxel_gather_workspace": list(p([1, 3, 64, 577], [0, 1, 1000])),
        "anet_voxel_path_workspace": list(p(GRIDS, [1, 3, 65])),
    }


def query():
    sys.path.insert(0, ROOT)
    from allocnet_amd import _lib
    lib = _lib.load()

    def params(mem, past):
        q = _lib.LbfgsParams()
        lib.anet_lbfgs_default_params(ctypes.byref(q))
        q.mem_size, q.past = mem, past
        return ctypes.byref(q)

    def grid(size):
        g = _lib.VoxelGrid()
        g.size[:] = size
        g.origin[:] = (0.0, 0.0, 0.0)
        g.scale = 0.25
        return ctypes.byref(g)

    out = {}
    for fn, rows in cases().items():
        f = getattr(lib, fn)
        out[fn] = []
        for a in rows:
            if fn in ("anet_lbfgs_workspace", "anet_lbfgs_minco_workspace"):
                v = f(*a[:-2], params(a[-2], a[-1]))
            elif fn == "anet_voxel_workspace":
                v = f(grid(a))
            elif fn == "anet_voxel_path_workspace":
                v = f(grid(a[0]), a[1])
            else:
                v = f(*a)
            flat = [x for e in a for x in (e if isinstance(e, tuple) else (e,))]
            out[fn].append(flat + [int(v)])
    return out


if __name__ == "__main__":
    text = "{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in query().items()) + "\n}\n"
    if "--write" in sys.argv:
        with open(FIXTURE, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
