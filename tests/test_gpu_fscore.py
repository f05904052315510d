"""Metric_FScore on the GPU (occ_metrics.py:322-410): pw_occ_fscore's count table against the numpy lattice restatement
(tests/_fscore_np.py) for 1 and 4 horizons, masked and not, Z in {8, 16, 33, 64} and partial tiles; accumulation, a captured
replay, the reference's float64 totals from tests/golden/fscore.npz, the empty-ground-truth convention, and the F-score inside
pipeline.SampleStream / harness.evaluate_stream (C1 mini-split, full-size C3, a range miss mid-stream).  All in this process."""
import numpy as np
import pytest
import torch

from preworld_amd import harness, metrics, ops, synth as S
from preworld_amd.pipeline import SampleStream
import _fscore_np as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GC = S.GRID_CONFIG_C1
HZ = (0, 2, 4, 6)
CONFIGS = [dict(), dict(thr_acc=1.0, thr_cmpl=0.45), dict(voxel_size=(0.5, 0.5, 0.25)), dict(void=(17,))]


def _grid(rs, shape):
    """mostly free, blobs of classes, a few unobserved voxels"""
    g = np.full(shape, 17, np.uint8)
    occ = rs.rand(*shape) < 0.25
    g[occ] = rs.randint(0, 17, int(occ.sum()))
    g[rs.rand(*shape) < 0.03] = 255
    return g


def _np_kw(kw):
    return dict(void=kw.get('void', (17, 255)), voxel_size=kw.get('voxel_size', (0.4, 0.4, 0.4)), thr_acc=kw.get('thr_acc', 0.6),
                thr_cmpl=kw.get('thr_cmpl', 0.6))


@pytest.mark.parametrize('H', [1, 4])
@pytest.mark.parametrize('shape', [(200, 200, 16), (101, 37, 16), (64, 50, 8), (33, 21, 33), (40, 30, 64)])
@pytest.mark.parametrize('masked', [False, True])
def test_counts_match_numpy(H, shape, masked):
    ci = (H + shape[0] + int(masked)) % len(CONFIGS)
    kw = CONFIGS[ci]
    rs = np.random.RandomState(H * 1000 + shape[0] * 7 + shape[2] + masked)
    preds, gts = [], []
    for _ in range(H):
        g = _grid(rs, shape)
        p = np.where(rs.rand(*shape) < 0.8, g, _grid(rs, shape)).astype(np.uint8)
        preds.append(p)
        gts.append(g)
    masks = [rs.rand(*shape) < 0.7 for _ in range(H)] if masked else None
    want = np.stack([F.counts(preds[h], gts[h], masks[h] if masked else None, **_np_kw(kw)) for h in range(H)])
    if shape == (101, 37, 16) and H == 4:
        # one horizon at an odd byte offset: the byte-load path at Z = 16
        buf = torch.zeros(preds[0].size + 1, dtype=torch.uint8, device=DEV)
        buf[1:] = torch.from_numpy(preds[0].ravel()).to(DEV)
        dp = [buf[1:].view(shape)] + [torch.from_numpy(p).to(DEV) for p in preds[1:]]
    else:
        dp = [torch.from_numpy(p).to(DEV) for p in preds]
    dg = [torch.from_numpy(g).to(DEV) for g in gts]
    dm = [torch.from_numpy(m).to(DEV) for m in masks] if masked else None
    table = torch.zeros(H, 4, dtype=torch.int64, device=DEV)
    ops.occ_fscore(dp, dg, dm, table, **kw)
    got = table.cpu().numpy()
    print('[fscore] H=%d %s masked=%s cfg %d: %s' % (H, shape, masked, ci, got[0].tolist()))
    assert np.array_equal(got, want), (got, want)
    ops.occ_fscore(dp, dg, dm, table, **kw)                    # accumulates
    assert np.array_equal(table.cpu().numpy(), 2 * want)
    # captured in a graph and replayed == an eager call
    gtab = torch.zeros_like(table)
    gr = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.occ_fscore(dp, dg, dm, gtab, **kw)                 # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(gr):
        gtab.zero_()
        ops.occ_fscore(dp, dg, dm, gtab, **kw)
    gtab.fill_(-5)
    gr.replay()
    torch.cuda.synchronize()
    assert np.array_equal(gtab.cpu().numpy(), want)


def test_metric_matches_reference_fixture(golden):
    z = golden('fscore.npz')
    for name in [str(c) for c in z['cases']]:
        kw, samples, per, totals = F.fixture_case(z, name)
        m = metrics.Metric_FScore(device=DEV, **kw)
        for pred, gt, lid, cam in samples:
            keep = [a.copy() if a is not None else None for a in (pred, gt, lid, cam)]
            m.add_batch(pred, gt, lid, cam)
            for a, b in zip((pred, gt, lid, cam), keep):   # the caller's arrays are untouched
                assert a is None or np.array_equal(a, b)
        got = np.array([m.tot_acc, m.tot_cmpl, m.tot_f1_mean])
        rel = np.abs(got - totals) / np.maximum(np.abs(totals), 1e-300)
        print('[fscore] %-14s device %s reference %s max rel diff %.3g' % (name, got.tolist(), totals.tolist(), rel.max()))
        assert m.cnt == len(samples) and m.n_empty_gt == 0
        assert np.all(rel <= 1e-12), (name, got, totals)
        # add_counts: the same from the per-sample count tables
        m2 = metrics.Metric_FScore(device=DEV, **kw)
        tab = torch.from_numpy(np.stack([F.case_counts(kw, s) for s in samples])).to(DEV)
        m2.add_counts(tab)
        assert m2.cnt == m.cnt and (m2.tot_acc, m2.tot_cmpl, m2.tot_f1_mean) == (m.tot_acc, m.tot_cmpl, m.tot_f1_mean)
    assert abs(m.count_fscore() - m.tot_f1_mean / m.cnt) == 0


def test_empty_ground_truth_convention():
    m = metrics.Metric_FScore(device=DEV)
    free = np.full((20, 30, 16), 17, np.uint8)
    some = free.copy()
    some[3:6, 4:9, 2:5] = 4
    m.add_batch(some, free, None, None)                        # the reference raises inside KDTree here
    assert (m.cnt, m.n_empty_gt) == (1, 1)
    assert (m.tot_acc, m.tot_cmpl, m.tot_f1_mean) == (0.0, 0.0, 0.0)
    m.add_batch(free, free, None, None)                        # empty prediction: (0, 0, 0) as in the reference
    m.add_batch(free, some, None, None)
    assert (m.cnt, m.n_empty_gt) == (3, 1)
    assert (m.tot_acc, m.tot_cmpl, m.tot_f1_mean) == (0.0, 0.0, 0.0)
    m.add_batch(some, some, None, None)
    assert (m.tot_acc, m.tot_cmpl) == (1.0, 1.0) and m.tot_f1_mean == 2.0 / (1 / (1.0 + 1e-8) + 1 / (1.0 + 1e-8))


# ---- the F-score inside the evaluation stream
FS = dict(threshold_acc=0.6, threshold_complete=0.6, voxel_size=[0.4, 0.4, 0.4], void=[17, 255])


def _samples(n, size, cams, rs, miss=None):
    out = []
    for i, seed in enumerate(range(1, n + 1)):
        frames = harness.lifted_frames(seed, cams, DEV)
        if i == miss:
            frames = [dict(fr, tran_feat=fr['tran_feat'] * 4096.0) for fr in frames]
        out.append(dict(frames=frames, ego=torch.from_numpy(S.ego_state(seed)).to(DEV), gt={h: _grid(rs, size) for h in HZ},
                        mask_camera=rs.rand(*size) < 0.7, mask_lidar=rs.rand(*size) < 0.8))
    return out


def _eager_fscore(stacks, samples, mask):
    want = {}
    for j, h in enumerate(HZ):
        m = metrics.Metric_FScore(device=DEV, use_image_mask=mask == 'camera', use_lidar_mask=mask == 'lidar', **FS)
        for st, s in zip(stacks, samples):
            m.add_batch(st[j], s['gt'][h], s['mask_lidar'], s['mask_camera'])
        want[h] = m
    return want


def _same_fscore(got, want, n):
    for h in HZ:
        g, w = got[h], want[h]
        assert g.cnt == w.cnt == n, (h, g.cnt, w.cnt)
        assert (g.tot_acc, g.tot_cmpl, g.tot_f1_mean) == (w.tot_acc, w.tot_cmpl, w.tot_f1_mean), h


def _same_miou(got, want):
    assert got.cnt == want.cnt
    for h in HZ:
        assert torch.equal(got.metrics[h]._hist, want.metrics[h]._hist), h
        assert torch.equal(got.metrics[h]._occ_hist, want.metrics[h]._occ_hist), h
    assert got.report() == want.report()


@pytest.mark.parametrize('fmask', [None, 'camera', 'lidar'])
def test_stream_fscore_c1(fmask):
    net = harness.build_model(harness.model_cfg(GC), S.synth_state_dict(0), DEV)
    samples = _samples(3, (100, 100, 8), 1, np.random.RandomState(31))
    rep0, stacks0, met0 = harness.evaluate_stream(net, samples, in_flight=2, keep_stacks=True)
    rep, stacks, met = harness.evaluate_stream(net, samples, in_flight=2, keep_stacks=True, fscore=dict(FS, mask=fmask))
    print('[fscore] C1 stream mask %s: %s' % (fmask, rep['fscore']))
    assert set(rep) == set(rep0) | {'fscore'} and all(rep[k] == rep0[k] for k in rep0)
    _same_miou(met, met0)                                      # mIoU unchanged, bit for bit
    assert all(np.array_equal(a, b) for a, b in zip(stacks, stacks0))
    _same_fscore(met.fscore, _eager_fscore(stacks, samples, fmask), 3)
    assert all(rep['fscore'][h] == met.fscore[h].tot_f1_mean / 3 for h in HZ)
    assert all(0.0 <= rep['fscore'][h] <= 1.0 for h in HZ)
    if fmask == 'camera':
        # the eager harness: the same metric over its own predictions
        rep_e, stacks_e, met_e = harness.evaluate(net, samples, DEV, fscore=dict(FS, mask=fmask))
        _same_fscore(met_e.fscore, _eager_fscore(stacks_e, samples, fmask), 3)
        assert set(rep_e['fscore']) == set(HZ)


def test_stream_fscore_full_size():
    net = harness.build_model(harness.model_cfg(S.GRID_CONFIG_FULL), S.synth_state_dict(0), DEV)
    samples = _samples(3, (200, 200, 16), 6, np.random.RandomState(32))
    rep, stacks, met = harness.evaluate_stream(net, samples, in_flight=2, keep_stacks=True, fscore=dict(FS, mask='camera'))
    torch.cuda.empty_cache()
    print('[fscore] full-size stream: %s' % rep['fscore'])
    _same_fscore(met.fscore, _eager_fscore(stacks, samples, 'camera'), 3)
    rep0, _, met0 = harness.evaluate_stream(net, samples, in_flight=2)
    _same_miou(met, met0)


def test_stream_fscore_range_miss_counted_once():
    net = harness.build_model(harness.model_cfg(GC), S.synth_state_dict(0), DEV)
    samples = _samples(6, (100, 100, 8), 1, np.random.RandomState(9), miss=3)
    st = SampleStream(net, samples[0]['frames'], samples[0]['ego'], in_flight=3, payload=True,
                      score=dict(horizons=HZ, n_cl=18, mask='camera', fscore=dict(FS, mask='lidar')))
    try:
        out = [{k: v[0].copy() for k, v in r.items()} for r in st.run(samples)]
        torch.cuda.synchronize()
        print('[fscore] range miss: replays %d, recalibrations %d' % (st.replays, st.recalibrations))
        assert len(out) == 6 and st.recalibrations >= 1
        assert all(st.fscore[h].cnt == 6 for h in HZ) and st.metric.cnt == 6
        stacks = [np.stack([o['semantic_occ_%ds' % h] for h in HZ]) for o in out]
        _same_fscore(st.fscore, _eager_fscore(stacks, samples, 'lidar'), 6)
    finally:
        st.close()
