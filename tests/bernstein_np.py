"""TEST INFRASTRUCTURE ONLY -- the shared pieces of csrc/bernstein_walk.h in numpy float64 without fused operations, for the
float64 restatements of the four exact trajectory queries (corridor_margin_mp.margin_float64, traj_voxel_hit_mp.hit_float64,
traj_clearance_mp.clearance_float64, traj_separation_mp.separation_float64).  Same operations in the same order as the header."""
from math import comb

import numpy as np


def bernstein(ua):
    """control values on [0, 1] of ascending coefficients"""
    n = len(ua) - 1
    return np.array([sum(comb(i, k) / comb(n, k) * ua[k] for k in range(i + 1)) for i in range(n + 1)])


def halve(w, right):
    """control values on an interval -> those on its left or right half (de Casteljau at 1/2); w is left unchanged"""
    w = np.array(w, dtype=np.float64)
    M = len(w)
    le = np.empty(M)
    le[0] = w[0]
    for r in range(1, M):
        w[:M - r] = 0.5 * (w[:M - r] + w[1:M - r + 1])
        le[r] = w[0]
    return w if right else le      # in place, w has ended as the right half


def descend(root, lev, idx):
    """the control values of [idx, idx + 1] / 2^lev from those of [0, 1]: `lev` halvings chosen by the bits of idx"""
    w = np.array(root, dtype=np.float64)
    for l in range(lev):
        w = halve(w, (idx >> (lev - 1 - l)) & 1)
    return w


def sign_scan(w):
    """(var, first, mx): sign changes with zeros skipped, the first sign that is not zero (0: none), the largest modulus"""
    w = np.asarray(w, dtype=np.float64)
    sg = (w > 0.0).astype(int) - (w < 0.0).astype(int)
    nz = sg[sg != 0]
    var = int((nz[1:] != nz[:-1]).sum()) if len(nz) else 0
    first = int(nz[0]) if len(nz) else 0
    return var, first, float(np.abs(w).max())


def advance(lev, idx, split):
    """(lev, idx, more): to the left half (split), or to the next interval on the right; more = False: the walk is over"""
    if split:
        return lev + 1, idx << 1, True
    while lev > 0 and (idx & 1):
        idx >>= 1
        lev -= 1
    if lev == 0:
        return lev, idx, False
    return lev, idx + 1, True


def product_cv(x, y):
    """control values (degree 2n - 1) of x . y' / n from the control values x, y (3, n + 1)"""
    n = x.shape[1] - 1
    dots = np.einsum("ai,aj->ij", x, np.diff(y, axis=1))
    dv = np.zeros(2 * n)
    for i in range(n + 1):
        for j in range(n):
            dv[i + j] += comb(n, i) * comb(n - 1, j) / comb(2 * n - 1, i + j) * dots[i, j]
    return dv
