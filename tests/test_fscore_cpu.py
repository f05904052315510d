"""Metric_FScore (occ_metrics.py:322-410) without a GPU: the lattice offsets of ops.fscore_offsets against brute-force KDTree
distances, the numpy lattice restatement against every per-sample score and total of the reference in tests/golden/fscore.npz,
the refusal of thresholds that tie a lattice distance, and the argument checks of pw_occ_fscore / pw_occ_fscore_accumulate
(they fail before any HIP call)."""
import ctypes

import numpy as np
import pytest

from preworld_amd import _lib, metrics, ops
import _fscore_np as F

LATTICES = [(0.6, (0.4, 0.4, 0.4)), (1.0, (0.4, 0.4, 0.4)), (0.45, (0.4, 0.4, 0.4)), (0.6, (0.5, 0.5, 0.25)),
            (0.95, (0.3, 0.5, 0.2)), (1.3, (0.4, 0.6, 0.35)), (0.35, (0.4, 0.4, 0.4)), (2.1, (0.4, 0.4, 0.4))]


@pytest.mark.parametrize('t,vs', LATTICES)
def test_fscore_offsets_match_kdtree(t, vs):
    KDTree = pytest.importorskip('sklearn.neighbors').KDTree
    rs = np.random.RandomState(int(t * 1000) + int(sum(vs) * 100))
    m = ops.fscore_offsets(t, vs)
    assert m.dtype == np.int8 and m.shape[0] % 2 == 1 and m.shape[1] % 2 == 1
    for trial in range(4):
        shape = (rs.randint(3, 14), rs.randint(3, 14), rs.randint(2, 12))
        a = rs.rand(*shape) < rs.uniform(0.02, 0.3)
        b = rs.rand(*shape) < rs.uniform(0.02, 0.3)
        a[0, 0, 0] = b[-1, -1, -1] = True
        pts = [np.argwhere(g) * np.asarray(vs) + np.asarray(vs) / 2 + np.array([-40.0, -40.0, -1.0]) for g in (a, b)]
        d, _ = KDTree(pts[1], leaf_size=10).query(pts[0])
        want = d.ravel() < t                                   # occupied voxel of a: a voxel of b closer than t
        got = F.near(b, m)[a]
        assert np.array_equal(got, want), (t, vs, shape, trial)


def test_fscore_offsets_default_is_the_19_offsets():
    m = ops.fscore_offsets(0.6, (0.4, 0.4, 0.4))
    assert m.tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    assert int((2 * m.astype(np.int64) + 1)[m >= 0].sum()) == 19


def test_ambiguous_threshold_raises():
    with pytest.raises(ValueError, match='ties'):
        ops.fscore_offsets(0.8, (0.4, 0.4, 0.4))               # 2 voxels along x
    with pytest.raises(ValueError, match='ties'):
        ops.fscore_offsets(0.4 * np.sqrt(2.0), (0.4, 0.4, 0.4))
    with pytest.raises(ValueError, match='ties'):
        ops.fscore_offsets(1.0, (0.5, 0.5, 0.25))
    with pytest.raises(ValueError, match='ties'):
        metrics.Metric_FScore(threshold_complete=0.8, device='cpu')
    with pytest.raises(ValueError):
        ops.fscore_offsets(0.0, (0.4, 0.4, 0.4))
    ops.fscore_offsets(0.8 * (1 + 1e-6), (0.4, 0.4, 0.4))      # clear of the tie: fine


def test_restatement_reproduces_reference_fixture(golden):
    z = golden('fscore.npz')
    names = [str(c) for c in z['cases']]
    assert {'plain', 'camera', 'lidar', 'thr', 'voxel', 'gt255', 'allfree', 'small'} <= set(names)
    for name in names:
        kw, samples, per, totals = F.fixture_case(z, name)
        tot = [0.0, 0.0, 0.0]
        for i, s in enumerate(samples):
            sc = F.scores(F.case_counts(kw, s))
            assert sc == tuple(per[i]), (name, i, sc, per[i])
            tot = [a + b for a, b in zip(tot, sc)]
        assert tot == list(totals), (name, tot, totals)


def _ptrs(n):
    return (ctypes.c_void_p * max(n, 1))(*([16] * max(n, 1)))


@pytest.mark.parametrize('case', ['z65', 'rx8', 'ry8', 'h0', 'h9'])
def test_occ_fscore_rejects_limits_without_gpu(case):
    l = _lib.lib()
    n_h, Z, rx, ry = 1, 16, 1, 1
    if case == 'z65':
        Z = 65
    elif case == 'rx8':
        rx = 8
    elif case == 'ry8':
        ry = 8
    else:
        n_h = 0 if case == 'h0' else 9
    vb = (ctypes.c_uint32 * 8)()
    tab = (ctypes.c_int8 * ((2 * rx + 1) * (2 * ry + 1)))()
    rc = l.pw_occ_fscore(_ptrs(n_h), _ptrs(n_h), None, n_h, 4, 4, Z, vb, tab, tab, rx, ry, ctypes.c_void_p(16), None)
    assert rc == -1
    assert b'pw_occ_fscore' in l.pw_last_error()


@pytest.mark.parametrize('n_h', [0, 9])
def test_occ_fscore_accumulate_rejects_horizons_without_gpu(n_h):
    l = _lib.lib()
    rc = l.pw_occ_fscore_accumulate(ctypes.c_void_p(16), 1, n_h, ctypes.c_void_p(16), ctypes.c_void_p(16), None)
    assert rc == -1
    assert b'pw_occ_fscore_accumulate' in l.pw_last_error()
