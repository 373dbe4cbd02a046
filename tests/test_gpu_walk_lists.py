"""GPU parity of the culled group walk's lists (knn32_group_kernel) on stores built to reach every
list path: 20 exact copies each of 100 states sit in one tile of the sorted store, so one ballot
offers more than 16 candidates at one distance (the bulk sort-merge, with ties at the k-th place),
the other states arrive through the single insertions; the SE(3) store spans more than one
mega-tile (131,072 states), the odd query counts leave a padding query in the last wave, and the
k values sit on both sides of the K2 = 16 / 32 / 64 list selection (k2 = k + 3).
Checked against the oracle's brute force: distances bit-identical, ids equal outside groups of
exactly equal distances (tests/parity.py)."""
import numpy as np
import pytest

import pyoracle as O
from ompl_amd import NearestNeighborsGPU
from ompl_amd import workloads as W
from ompl_amd.spaces import RealVectorStateSpace, SE3StateSpace
from parity import assert_knn_parity, oracle_knn_mt

pytestmark = pytest.mark.gpu

COPIES, DUP = 20, 100  # 100 states stored 20 times each
K_SE3 = (1, 10, 13, 29, 57)


def tied_store(sample, rng, n):
    """n states: n - 2,000 distinct ones and 20 copies each of 100 more, shuffled; + the 100."""
    base = sample(rng, n - COPIES * DUP)
    dup = sample(rng, DUP)
    data = np.concatenate([base, np.repeat(dup, COPIES, axis=0)])
    return np.ascontiguousarray(data[rng.permutation(len(data))]), dup


@pytest.fixture(scope="module")
def se3_case(gpu):
    rng = np.random.default_rng(2024)
    sp = SE3StateSpace()
    data, dup = tied_store(W.uniform_se3, rng, 140_000)
    q = np.ascontiguousarray(np.concatenate([dup, W.uniform_se3(rng, 255 - DUP)]))  # 255: a padding query
    nn = NearestNeighborsGPU(sp, gpu)
    nn.add(data)
    # the oracle's lists reach past the largest k by more than one tie group: the boundary class is whole
    oi, od = oracle_knn_mt(O, sp, data, q, max(K_SE3) + COPIES + 3)
    return nn, q, oi, od


@pytest.mark.parametrize("k", K_SE3)
def test_se3_tied_lists(se3_case, k):
    nn, q, oi, od = se3_case
    ids, d, cnt = nn.nearestKBatch(q, k)
    assert (cnt == k).all()
    assert (d[:DUP, :min(k, COPIES)] == 0.0).all(), "a stored copy of the query is at distance 0"
    assert_knn_parity(ids, d, oi, od, k)


def test_r6_tied_lists(gpu):
    rng = np.random.default_rng(2025)
    sp = RealVectorStateSpace(6)
    sample = lambda r, n: W.uniform_rv(r, n, 6)  # noqa: E731
    data, dup = tied_store(sample, rng, 20_000)
    q = np.ascontiguousarray(np.concatenate([dup, sample(rng, 129 - DUP)]))
    nn = NearestNeighborsGPU(sp, gpu)
    nn.add(data)
    ids, d, cnt = nn.nearestKBatch(q, 10)
    assert (cnt == 10).all()
    assert (d[:DUP] == 0.0).all()
    oi, od, _ = O.knn(sp, data, q, 10 + COPIES + 3)
    assert_knn_parity(ids, d, oi, od, 10)
