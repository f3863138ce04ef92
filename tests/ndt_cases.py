"""Generators and host references shared by tests/test_ndt_host.py and tests/test_gpu_ndt.py (TEST INFRASTRUCTURE ONLY).

The refine cases are the surface clouds of tests/test_icp_plane.py (``surface_case``) at the shapes of tests/test_gpu_icp_plane.py.
The seeds were chosen on the CPU (``clear_of_thresholds`` below is the criterion, asserted again by the tests that rely on it)."""
import numpy as np

from deepsir_amd.ndt import ndt_map_host, ndt_refine_host
from test_icp_plane import surface_case

RES = 0.2                    # cell edge on the 1.5 x 1.5 surface: 10 .. 100 valid cells at the shapes below
STEP_TOL = 1e-4
CAP_ITERS = 6                # the capped runs stop here, far from convergence (the step norms are then > 10 x their thresholds)
ULP_SEEDS = (1, 2, 3, 4)

# (J, K, noise on ref, seeds of the three pairs of a call)
REFINE_CASES = [(37, 300, 0.0, (13, 23, 33)), (300, 300, 0.0, (4, 14, 24)), (1357, 1024, 0.0, (9, 19, 29)), (2500, 2500, 0.004, (8, 18, 28))]
NEIGHBORS = (7, 1)


def clear_of_thresholds(trace, factor, tol=STEP_TOL, res=RES):
    """True if at EVERY iteration of a host trace the convergence decision has a margin of `factor`: both step norms below their
    thresholds / factor (a clear stop), or at least one above its threshold x factor (a clear go-on).  An identity update (None)
    is a decision without arithmetic."""
    for t in trace:
        if t is None:
            continue
        nr, nt = t
        stop = nr * factor < tol and nt * factor < tol * res
        go = nr > tol * factor or nt > tol * res * factor
        if not (stop or go):
            return False
    return True


_MAPS, _HOST = {}, {}


def ref_map(J, K, seed, noise, res=RES):
    key = (J, K, seed, noise, res)
    if key not in _MAPS:
        _MAPS[key] = ndt_map_host(surface_case(J, K, seed, noise)["ref"], res)
    return _MAPS[key]


def host_refine(J, K, seed, noise, neighbors, max_iter, perturb_ulps=None):
    """ndt_refine_host on a surface case from its T0, computed once per (case, arguments) and left unchanged"""
    key = (J, K, seed, noise, neighbors, max_iter, perturb_ulps)
    if key not in _HOST:
        c = surface_case(J, K, seed, noise)
        _HOST[key] = ndt_refine_host(c["src"], c["ref"], c["T0"], RES, neighbors=neighbors, max_iter=max_iter, step_tol=STEP_TOL,
                                     perturb_ulps=perturb_ulps, m=ref_map(J, K, seed, noise))
    return _HOST[key]


def map_cloud(K, seed, res=0.25):
    """A reference cloud for the map tests: clusters of 1 .. 40 points, each inside one cell of edge `res`, anisotropic (a tilted
    slab: spreads 1 : 0.5 : 0.02 of a quarter cell) so that the 0.01 floor acts and the regularised condition number is 100 at the
    most; cluster sizes straddle the validity threshold of 6.  -> [K,3] float32, shuffled."""
    rng = np.random.default_rng(seed)
    pts = []
    left = K
    while left > 0:
        n = int(min(left, rng.choice([1, 3, 5, 6, 7, 12, 25, 40])))
        cell = rng.integers(0, 12, 3)
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        local = rng.uniform(-1, 1, (n, 3)) * np.array([0.2, 0.1, 0.004]) * res
        pts.append((cell + 0.5) * res + local @ Q.T)
        left -= n
    p = np.concatenate(pts)[:K]
    return p[rng.permutation(K)].astype(np.float32)
