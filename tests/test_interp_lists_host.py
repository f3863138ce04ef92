"""interp_idx without a search (csrc/knn.hip, interp_lists_kernel), stated in numpy over the oracle's lists.

Level l + 1 is the first m = n_{l+1} points of level l.  The 16-NN list of a query holds the 16 smallest candidates of level l under
(fp32 d2, then lower index), in that order; the interpolation search returns the minimum of the same order over the indices < m.  A
candidate that precedes a member of the 16 smallest is one of them, so if any list entry is < m, the first such entry in list order
is the answer; only a query whose 16 neighbours all lie outside the prefix needs a search (the "fallback").  Checked here against
oracle.knn's own interp_idx, with the share of fallback queries: small on shuffled clouds (15 other neighbours, each in the prefix with
probability 1/4: 0.75^15 = 1.3 %; measured 0 - 1.95 % per level on the synthetic pairs, hence the 5 % cap), most of a cloud sorted
along x, whose prefix is a slab."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import interp_lists_dump as cases  # noqa: E402
from oracle.knn import knn_pyramid  # noqa: E402

K, RATIOS = 16, (4, 4, 4, 4)


def levels(n):
    nl = [n]
    for r in RATIOS:
        nl.append(nl[-1] // r)
    return nl


def interp_from_lists(cloud):
    """-> (mismatches among the queries the rule answers, fallback share per level) against the oracle's interp_idx"""
    pyr = knn_pyramid(cloud, K, RATIOS)
    nl = levels(len(cloud))
    off, bad, share = 0, 0, []
    for l in range(len(RATIOS)):
        lists = pyr["neigh_idx"][off:off + nl[l]]
        want = pyr["interp_idx"][off:off + nl[l], 0]
        inside = lists < nl[l + 1]
        has = inside.any(1)
        first = lists[np.arange(nl[l]), inside.argmax(1)]
        bad += int((first[has] != want[has]).sum())
        share.append(1.0 - has.mean())
        off += nl[l]
    return bad, share


@pytest.mark.parametrize("n,kw", [(1027, {}), (1027, {"partial_overlap": True}), (5000, {}), (5000, {"partial_overlap": True})])
def test_random_clouds(n, kw):
    for cloud in cases.random_clouds(n, [3], **kw):
        bad, share = interp_from_lists(cloud)
        print("fallback share per level", n, kw, np.round(share, 4))
        assert bad == 0
        assert max(share) <= 0.05


def test_sorted_cloud_falls_back():
    for cloud in cases.sorted_clouds():
        bad, share = interp_from_lists(cloud)
        print("sorted: fallback share per level", np.round(share, 4))
        assert bad == 0
        assert share[0] >= 0.5


def test_duplicates_across_the_prefix_boundary():
    cloud = cases.duplicate_cloud()[0]
    nl = levels(len(cloud))
    # the case is what it says: some point of every prefix has a copy outside it (d2 = 0 on both sides of the boundary)
    for m in nl[1:4]:
        assert (cloud[m:nl[0], None, :] == cloud[None, :m, :]).all(2).any()
    bad, share = interp_from_lists(cloud)
    print("duplicates: fallback share per level", np.round(share, 4))
    assert bad == 0


def test_level_of_exactly_16_points():
    cloud = cases.random_clouds(1024, [5])[0]
    assert levels(1024)[3] == K
    bad, share = interp_from_lists(cloud)
    assert bad == 0
    assert share[3] == 0.0      # the list of a 16-point level is the whole level
