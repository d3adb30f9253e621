"""Pins the restatement the GPU suite compares against (tests/frontier_np.py): component labels against scipy.ndimage.label, view
gain against the scan of tests/occupancy_np.py through the identity the definition buys, and the frontier rule at its edges."""
import numpy as np
import pytest

from tests import frontier_np as fnp
from tests import occupancy_np as onp


@pytest.mark.parametrize("density", [0.1, 0.3, 0.6])
@pytest.mark.parametrize("connectivity", [6, 26])
def test_labels_partition_like_scipy_and_are_minimum_indices(connectivity, density):
    from scipy import ndimage
    size = (19, 13, 11)
    rng = np.random.default_rng(int(100 * density) + connectivity)
    mask = (rng.uniform(size=int(np.prod(size))) < density).astype(np.uint8)
    labels = fnp.label_components(mask, size, connectivity)
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    ref, k = ndimage.label(mask.reshape(size[2], size[1], size[0]), structure=structure)
    ref = ref.reshape(-1)
    assert ((labels >= 0) == (mask != 0)).all() and ((ref > 0) == (mask != 0)).all()
    on = np.flatnonzero(mask)
    assert len(np.unique(labels[on])) == k
    # the same partition: each of scipy's components carries one label of ours, and that label is its least index
    for c in range(1, k + 1):
        members = np.flatnonzero(ref == c)
        assert (labels[members] == members.min()).all()


def test_view_gain_is_the_unknown_count_a_scan_removes():
    """On a grid with no occupied voxel, gain == count(UNKNOWN before) - count(UNKNOWN after onp.integrate) for the same world points
    from the same origin: points beyond max_range, inside it, and inside min_range."""
    size, origin, scale = (24, 20, 12), (-1.0, 0.5, -0.25), 0.25
    rng = np.random.default_rng(5)
    n = int(np.prod(size))
    L = np.full(n, onp.UNKNOWN, dtype=np.int16)
    L[rng.uniform(size=n) < 0.3] = -405                                   # known free, nothing occupied
    prm = onp.Params(min_range=0.4, max_range=2.0)
    for k in range(3):
        t = np.asarray(origin) + rng.uniform(0.1, 0.9, 3) * np.asarray(size) * scale
        A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        d = rng.normal(size=(300, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        pts = d * rng.choice([0.1, 0.3, 0.9, 1.7, 2.5, 6.0], size=(300, 1))
        pts[:3] = np.nan
        world = fnp.world_points(A, t, pts)
        ln = np.linalg.norm(world[3:] - t, axis=1)
        assert (ln < prm.min_range).any() and (ln > prm.max_range).any() and ((ln > prm.min_range) & (ln < prm.max_range)).any()
        after = onp.integrate(L.copy(), size, origin, scale, prm, t, world)
        want = int((L == onp.UNKNOWN).sum() - (after == onp.UNKNOWN).sum())
        got = fnp.view_gain(L, size, origin, scale, prm, 0, A, t, pts)
        assert want > 50 and got.tolist() == [want], (k, want, got)


def test_view_gain_stops_at_occupied_and_flags_bad_views():
    size, origin, scale = (10, 3, 3), (0.0, 0.0, 0.0), 1.0
    L = np.full(90, onp.UNKNOWN, dtype=np.int16)
    L[10 + 10 * 3 + 5] = 900                                                # cell (5, 1, 1) occupied
    prm = onp.Params(min_range=0.0, max_range=20.0)
    t = np.array([0.5, 1.5, 1.5])
    pts = np.array([[9.0, 0.0, 0.0]])
    eye = np.eye(3)
    bad = eye.copy(); bad[1, 2] = np.inf
    g = fnp.view_gain(L, size, origin, scale, prm, 900, [eye, eye, bad], [t, [5.5, 1.5, 1.5], t], pts)
    assert g.tolist() == [5, 0, -1]                                        # cells 0..4, then blocked; inside the occupied cell; bad
    assert fnp.view_gain(L, size, origin, scale, prm, 901, [eye], [t], pts).tolist() == [9]   # below the threshold it is free


def test_frontier_rule_at_the_threshold_and_the_map_edge():
    size = (4, 3, 1)
    occ = 7
    L = np.full(12, -100, dtype=np.int16)
    L[5] = onp.UNKNOWN                                                      # (1, 1, 0): its face neighbours are 1, 9, 4, 6
    L[4], L[6] = occ - 1, occ                                               # L = occ - 1 is free, L = occ is not
    mask, count = fnp.frontier(L, size, occ)
    assert np.flatnonzero(mask).tolist() == [1, 4, 9] and count == 3
    # a free voxel on the boundary with no unknown neighbour INSIDE the map is not a frontier: nothing unknown, nothing marked
    mask, count = fnp.frontier(np.full(12, -100, dtype=np.int16), size, occ)
    assert count == 0 and not mask.any()
    # unknown itself is never a frontier, and a box cuts the mask
    mask, count = fnp.frontier(L, size, occ, box=((0, 0, 0), (4, 1, 1)))
    assert np.flatnonzero(mask).tolist() == [1] and count == 1
