// The plain numbers the workspace layouts (workspace.h) share with the kernels that fill those workspaces.  No device code, no HIP
// include: the kernel headers and the host-only workspace.h both read them here.
#pragma once

namespace anet {

// rows of the L-BFGS state (lbfgs_step.h): doubles and int32 per problem
enum { DS_FX = 0, DS_STEP, DS_FINIT, DS_DGTEST, DS_DSTEST, DS_MU, DS_NU, DS_SMAX, DS_COUNT_ };  // DS_SMAX: stpmax of the running line search
enum { IS_DONE = 0, IS_RET, IS_K, IS_END, IS_BOUND, IS_COUNT, IS_BRACKT, IS_TOUCHED, IS_EVALS, IS_PHASE, IS_COUNT_ };
// a parked optimiser of the one-launch MINCO L-BFGS (lbfgs_resident.h): per-lane fields x 64 lanes, then 64 wave-uniform values
constexpr int kPersistContLaneFields = 22, kPersistContDoubles = (kPersistContLaneFields + 1) * 64;
constexpr int kIpmContScalars = 16;  // scalars parked behind the node states of a stopped problem (IpmArgs::cont)
constexpr int kFiriEll = 18;         // doubles of ellipsoid state per corridor (firi_kernels.h)
// Launch order for anet_lbfgs_minco_ordered_dev from the evaluation counts of a previous solve: a counting sort into 4096
// buckets of 16 evaluations, longest first (the order inside a bucket is whatever the atomics make it: irrelevant here).
constexpr int kOrderBuckets = 4096;
// connected components (frontier_kernels.h): voxels per block of the root count / rank pass; view gain: the alignment of a view's
// slot of mark bytes (the count pass reads and clears it in 16-byte pieces, 256 threads wide)
constexpr int kCompScanBlock = 256;
constexpr int kViewSlotAlign = 4096;

}  // namespace anet
