"""Streaming evaluation on the GPU: the fused scoring kernel (pw_occ_score) against a numpy restatement of the reference metric,
pipeline.SampleStream / harness.evaluate_stream against harness.evaluate (C1 mini-split and full-size C3), a range miss in the
middle of a stream, a weight change between runs and the order of the yielded payloads.  All in this process; at most three
full-size slots exist at once."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from preworld_amd import harness, metrics, ops, synth as S
from preworld_amd.pipeline import SampleStream
from _parity import check_argmax

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GC = S.GRID_CONFIG_C1
LOGIT_TIE = 2e-4                        # as in test_gpu_e2e.py
HZ = (0, 2, 4, 6)


def _np_table(pred, gt, mask, n_cl):
    """hist_info (occ_metrics.py:82-105) over masked voxels + add_batch's binary histogram (:150-154; gt = 255 is occupied)"""
    m = np.ones(gt.shape, bool) if mask is None else mask.astype(bool)
    k = m & (gt < n_cl)
    hist = np.bincount(n_cl * gt[k].astype(np.int64) + pred[k], minlength=n_cl * n_cl)
    free = n_cl - 1
    b = np.bincount(2 * (gt[m] != free).astype(np.int64) + (pred[m] != free), minlength=4)
    return np.concatenate([hist, b]).astype(np.int64)


@pytest.mark.parametrize('H', [1, 4])
@pytest.mark.parametrize('N', [640000, 80000 + 13])
@pytest.mark.parametrize('masked', [False, True])
def test_occ_score_matches_numpy(H, N, masked):
    rs = np.random.RandomState(H * 1000 + N % 97 + masked)
    preds = [rs.randint(0, 18, N).astype(np.uint8) for _ in range(H)]
    gts = []
    for _ in range(H):
        g = rs.randint(0, 18, N).astype(np.uint8)
        g[rs.rand(N) < 0.05] = 255
        gts.append(g)
    masks = [(rs.rand(N) < 0.6).astype(np.uint8) for _ in range(H)] if masked else None
    want = np.stack([_np_table(preds[h], gts[h], masks[h] if masked else None, 18) for h in range(H)])
    dp = [torch.from_numpy(p).to(DEV) for p in preds]
    dg = [torch.from_numpy(g).to(DEV) for g in gts]
    dm = [torch.from_numpy(m).to(DEV).bool() for m in masks] if masked else None
    counts = torch.zeros(H, 18 * 18 + 4, dtype=torch.int64, device=DEV)
    ops.occ_score(dp, dg, dm, 18, counts)
    assert np.array_equal(counts.cpu().numpy(), want)
    ops.occ_score(dp, dg, dm, 18, counts)                      # accumulates
    assert np.array_equal(counts.cpu().numpy(), 2 * want)
    # captured in a graph and replayed twice == two eager calls
    gc = torch.zeros_like(counts)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.occ_score(dp, dg, dm, 18, gc)                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gc.zero_()
    with torch.cuda.graph(g):
        ops.occ_score(dp, dg, dm, 18, gc)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gc, counts)


def test_occ_score_rejects_bad_arguments():
    x = torch.zeros(16, dtype=torch.uint8, device=DEV)
    c = torch.zeros(1, 328, dtype=torch.int64, device=DEV)
    with pytest.raises(ops._lib.PreworldHipError):
        ops.occ_score([x] * 9, [x] * 9, None, 18, torch.zeros(9, 328, dtype=torch.int64, device=DEV))
    with pytest.raises(ops._lib.PreworldHipError):
        ops.occ_score([x], [x[:8]], None, 18, c)
    with pytest.raises(ops._lib.PreworldHipError):
        ops.occ_score([x], [x], None, 18, torch.zeros(1, 300, dtype=torch.int64, device=DEV))
    with pytest.raises(ops._lib.PreworldHipError):
        ops.occ_score([x], [x], None, 40, torch.zeros(1, 1604, dtype=torch.int64, device=DEV))


# ---- C1 mini-split of test_gpu_e2e.py
def _c1_split():
    rs = np.random.RandomState(77)
    samples = []
    for seed in (1, 2):
        gt = {h: rs.randint(0, 18, size=(100, 100, 8)).astype(np.uint8) for h in HZ}
        mask = rs.rand(100, 100, 8) < 0.7
        samples.append(dict(frames=harness.lifted_frames(seed, 1, DEV), ego=torch.from_numpy(S.ego_state(seed)).to(DEV),
                            gt=gt, mask_camera=mask))
    return samples


def _oracle_logits(seed, sd):
    bevs = []
    for f in range(2):
        depth, feat = S.lift_inputs(seed * 16 + f, N=1)
        r = S.synthetic_rig(1, dx=-2.5 * f)
        bev = O.lss_view_transform(depth, feat, r['sensor2ego'], r['intrin'], r['post_rot'], r['post_tran'],
                                   r['bda'], GC, S.INPUT_SIZE, S.DOWNSAMPLE)
        bevs.append(O.pre_process(bev, sd))
    vf = O.final_conv(O.encoder_forward(bevs[1], bevs[0], sd), sd)
    _, feats = O.preworld4d_decode(vf, S.ego_state(seed), sd, n_steps=6, post_finetune=True)
    return {h: O.occ_decode(feats[h], sd)[1] for h in HZ}


@pytest.fixture(scope='module')
def c1():
    sd = S.synth_state_dict(0)
    net = harness.build_model(harness.model_cfg(GC), sd, DEV)
    samples = _c1_split()
    rep, stacks, metric = harness.evaluate(net, samples, DEV)
    logits = [_oracle_logits(seed, sd) for seed in (1, 2)]
    return dict(net=net, samples=samples, report=rep, stacks=stacks, logits=logits)


def _hist_from_stacks(stacks, samples):
    m = metrics.Metric_mIoU_Temporal(num_classes=18, use_image_mask=True, device=DEV)
    for st, s in zip(stacks, samples):
        m.add_batch(st, s['gt'], None, {h: s['mask_camera'] for h in s['gt']})
    return m


def _same_metric(got, want):
    assert got.cnt == want.cnt
    for sec in range(4):
        assert np.array_equal(getattr(got, 'hist_%ds' % sec), getattr(want, 'hist_%ds' % sec)), sec
        assert np.array_equal(getattr(got, 'occ_hist_%ds' % sec), getattr(want, 'occ_hist_%ds' % sec)), sec
    assert got.report() == want.report()
    assert got.count_iou() == want.count_iou()
    gi, gl = got.count_miou()
    wi, wl = want.count_miou()
    assert gl == wl and np.array_equal(gi, wi, equal_nan=True)


@pytest.mark.parametrize('in_flight', [1, 2, 3])
def test_stream_matches_evaluate_on_the_c1_mini_split(c1, in_flight):
    rep, stacks, metric = harness.evaluate_stream(c1['net'], c1['samples'], in_flight=in_flight, keep_stacks=True)
    assert len(stacks) == 2 and metric.cnt == 2
    # the device-side scores are exactly what add_batch gives on the stream's own predictions
    _same_metric(metric, _hist_from_stacks(stacks, c1['samples']))
    for h in list(HZ) + ['avg_future']:
        assert abs(rep[h] - c1['report'][h]) <= 0.01, (h, rep[h], c1['report'][h])
    for i, (st, ev) in enumerate(zip(stacks, c1['stacks'])):
        for j, h in enumerate(HZ):
            check_argmax('stream M=%d C1 sample %d state %ds' % (in_flight, i, h), st[j], ev[j], c1['logits'][i][h], LOGIT_TIE)
    # scoring only: no stacks, the same totals
    rep2, none, metric2 = harness.evaluate_stream(c1['net'], c1['samples'], in_flight=in_flight)
    assert none is None and rep2 == rep
    _same_metric(metric2, metric)


def test_stream_matches_evaluate_full_size():
    gc = S.GRID_CONFIG_FULL
    net = harness.build_model(harness.model_cfg(gc), S.synth_state_dict(0), DEV)
    rs = np.random.RandomState(321)
    samples = []
    for seed in range(1, 5):
        gt = {}
        for h in HZ:
            g = rs.randint(0, 18, size=(200, 200, 16)).astype(np.uint8)
            g[rs.rand(200, 200, 16) < 0.02] = 255
            gt[h] = g
        samples.append(dict(frames=harness.lifted_frames(seed, 6, DEV), ego=torch.from_numpy(S.ego_state(seed)).to(DEV),
                            gt=gt, mask_camera=rs.rand(200, 200, 16) < 0.7))
    rep, stacks, metric = harness.evaluate_stream(net, samples, in_flight=2, keep_stacks=True)
    torch.cuda.empty_cache()
    _same_metric(metric, _hist_from_stacks(stacks, samples))
    want_rep, want_stacks, _ = harness.evaluate(net, samples, DEV)
    print('[stream] full size, 4 samples: stream %s, evaluate %s' % (rep, want_rep))
    for h in list(HZ) + ['avg_future']:
        assert abs(rep[h] - want_rep[h]) <= 0.01, (h, rep[h], want_rep[h])
    for i, s in enumerate(samples):
        with torch.no_grad():
            res = net.simple_test_from_lift(s['frames'], s['ego'], n_steps=6, want_logits=True)
        for j, h in enumerate(HZ):
            eager = res['semantic_occ_%ds' % h][0].cpu().numpy()
            assert np.array_equal(eager, want_stacks[i][j])
            lg = res['logits'][h][0].permute(2, 1, 0, 3).cpu().numpy()
            check_argmax('stream full-size sample %d state %ds' % (i, h), stacks[i][j], eager, lg, LOGIT_TIE)
        del res


def _payload_copy(res):
    return {k: v[0].copy() for k, v in res.items()}


def test_range_miss_mid_stream_is_repaired_and_counted_once():
    net = harness.build_model(harness.model_cfg(GC), S.synth_state_dict(0), DEV)
    rs = np.random.RandomState(9)
    samples = []
    for i, seed in enumerate(range(1, 7)):
        frames = harness.lifted_frames(seed, 1, DEV)
        if i == 3:
            frames = [dict(fr, tran_feat=fr['tran_feat'] * 4096.0) for fr in frames]
        gt = {}
        for h in HZ:
            g = rs.randint(0, 18, size=(100, 100, 8)).astype(np.uint8)
            g[rs.rand(100, 100, 8) < 0.05] = 255
            gt[h] = g
        samples.append(dict(frames=frames, ego=torch.from_numpy(S.ego_state(seed)).to(DEV), gt=gt,
                            mask_camera=rs.rand(100, 100, 8) < 0.7))
    # in_flight 3: sample 3 is the last one slot 0 runs, so its static buffers and range table still hold sample 3 afterwards
    st = SampleStream(net, samples[0]['frames'], samples[0]['ego'], in_flight=3, payload=True,
                      score=dict(horizons=HZ, n_cl=18, mask='camera'))
    try:
        out = [_payload_copy(r) for r in st.run(samples)]
        torch.cuda.synchronize()
        print('[stream] range miss: replays %d, recalibrations %d' % (st.replays, st.recalibrations))
        assert len(out) == 6 and st.recalibrations >= 1 and st.replays == 6 + st.recalibrations
        same = st.slots[0].cap.eager()
        torch.cuda.synchronize()
        for k in out[3]:
            assert np.array_equal(out[3][k], same[k][0].cpu().numpy()), k
        want_total = sum(int((s['mask_camera'] & (s['gt'][h] < 18)).sum()) for s in samples for h in HZ)
        got_total = sum(int(st.metric.metrics[h]._hist.sum()) for h in HZ)
        assert got_total == want_total, (got_total, want_total)
        assert all(int(st.metric.metrics[h]._occ_hist.sum()) == sum(int(s['mask_camera'].sum()) for s in samples) for h in HZ)
        assert st.metric.cnt == 6
        # and the totals are exactly add_batch's on the stream's own predictions
        stacks = [np.stack([o['semantic_occ_%ds' % h] for h in HZ]) for o in out]
        _same_metric(st.metric, _hist_from_stacks(stacks, samples))
    finally:
        st.close()


def _check_payload(name, got, res):
    """the 14 grids of one yielded sample against that sample's eager result (with logits): near-ties only; geo_occ follows
    the semantic grid (preworld_temporal_traj.py:313-319)"""
    for k in range(7):
        eager = res['semantic_occ_%ds' % k][0].cpu().numpy()
        lg = res['logits'][k][0].permute(2, 1, 0, 3).cpu().numpy()
        sem = got['semantic_occ_%ds' % k]
        check_argmax('%s state %ds' % (name, k), sem, eager, lg, LOGIT_TIE)
        assert np.array_equal(got['geo_occ_%ds' % k], np.where(sem != 17, 0, 17).astype(np.uint8)), k


def _perturbed_bn(net, seed):
    rs = np.random.RandomState(seed)
    sd = {}
    for k, v in net.state_dict().items():
        if k.endswith('running_var'):
            sd[k] = v * torch.from_numpy(np.exp2(rs.uniform(-1.5, 1.5, tuple(v.shape))).astype(np.float32)).to(v.device)
        elif k.endswith('running_mean'):
            sd[k] = v + 0.2 * torch.from_numpy(rs.standard_normal(tuple(v.shape)).astype(np.float32)).to(v.device)
    return sd


def test_weight_change_recaptures():
    net = harness.build_model(harness.model_cfg(GC), S.synth_state_dict(0), DEV)
    samples = [dict(frames=harness.lifted_frames(seed, 1, DEV), ego=torch.from_numpy(S.ego_state(seed)).to(DEV)) for seed in (1, 2, 3)]
    st = SampleStream(net, samples[0]['frames'], samples[0]['ego'], in_flight=2, payload=True)
    try:
        old = [_payload_copy(r) for r in st.run(samples)]
        net.load_state_dict(_perturbed_bn(net, 4), strict=False)
        new = [_payload_copy(r) for r in st.run(samples)]
        assert st.recaptures == 1
        changed = 0
        for i, s in enumerate(samples):
            with torch.no_grad():
                res = net.simple_test_from_lift(s['frames'], s['ego'], n_steps=6, want_logits=True)
            _check_payload('stream after load_state_dict sample %d' % i, new[i], res)
            changed += sum(int((new[i][k] != old[i][k]).sum()) for k in old[i] if k.startswith('semantic_occ'))
            del res
        print('[stream] weights changed: %d voxels differ from the results under the old weights' % changed)
        assert changed > 500, 'the stream still replays the old weights'
    finally:
        st.close()


def test_yielded_payloads_are_in_input_order():
    net = harness.build_model(harness.model_cfg(GC), S.synth_state_dict(0), DEV)
    samples = [dict(frames=harness.lifted_frames(seed, 1, DEV), ego=torch.from_numpy(S.ego_state(seed)).to(DEV)) for seed in range(1, 6)]
    st = SampleStream(net, samples[0]['frames'], samples[0]['ego'], in_flight=3, payload=True)
    try:
        out = [_payload_copy(r) for r in st.run(samples)]
        assert len(out) == 5 and all(len(o) == 14 for o in out) and st.replays >= 5
        for i, s in enumerate(samples):
            with torch.no_grad():
                res = net.simple_test_from_lift(s['frames'], s['ego'], n_steps=6, want_logits=True)
            _check_payload('stream M=3 sample %d' % i, out[i], res)
        assert any(not np.array_equal(out[0][k], out[1][k]) for k in out[0])
    finally:
        st.close()
