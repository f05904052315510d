"""harness.evaluate_stream(distributed=True) with the REAL captured hot path: two gloo ranks share cuda:0 (RCCL refuses two ranks
on one GPU; the tables then travel through host memory) and every rank must return exactly what ONE process returns over the
same samples -- integer tables equal, F-score float64 totals bit for bit -- with a rank that has no sample, with dump_dir, and
with a range miss on one rank.  C1 grid, two samples in flight, the F-score under the camera mask."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
HZ = (0, 2, 4, 6)
FSCORE = dict(mask='camera')


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Recording:
    """a sequence that records which items were read"""

    def __init__(self, items):
        self.items, self.read = items, set()

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        self.read.add(i)
        return self.items[i]


def _samples(n, dev, miss=None, empty_gt=None):
    import torch
    from preworld_amd import harness, synth as S
    rs = np.random.RandomState(11)
    out = []
    for i in range(n):
        frames = harness.lifted_frames(i + 1, 1, dev)
        if i == miss:                                  # the perturbation of test_range_miss_mid_stream_is_repaired_and_counted_once
            frames = [dict(fr, tran_feat=fr['tran_feat'] * 4096.0) for fr in frames]
        gt = {}
        for h in HZ:
            g = rs.randint(0, 18, size=(100, 100, 8)).astype(np.uint8)
            g[rs.rand(100, 100, 8) < 0.05] = 255
            gt[h] = np.full_like(g, 17) if i == empty_gt else g     # nothing occupied: the F-score's n_empty_gt case
        out.append(dict(frames=frames, ego=torch.from_numpy(S.ego_state(i + 1)).to(dev), gt=gt,
                        mask_camera=rs.rand(100, 100, 8) < 0.7, scene_name='scene-%04d' % (i // 2), sample_idx='tok%02d' % i))
    return out


def _compare(got, want, bad, what):
    """append to `bad` every way the metric `got` differs from `want`"""
    if got.cnt != want.cnt:
        bad.append('%s: cnt %d != %d' % (what, got.cnt, want.cnt))
    for sec in range(4):
        for name in ('hist_%ds' % sec, 'occ_hist_%ds' % sec):
            if not np.array_equal(getattr(got, name), getattr(want, name)):
                bad.append('%s: %s differs' % (what, name))
    if got.report() != want.report():
        bad.append('%s: report %s != %s' % (what, got.report(), want.report()))
    if got.count_iou() != want.count_iou():
        bad.append('%s: count_iou %s != %s' % (what, got.count_iou(), want.count_iou()))
    gi, gl = got.count_miou()
    wi, wl = want.count_miou()
    if gl != wl or not np.array_equal(gi, wi, equal_nan=True):
        bad.append('%s: count_miou %s != %s' % (what, gl, wl))
    for h in HZ:
        g, w = got.fscore[h], want.fscore[h]
        for name in ('cnt', 'tot_acc', 'tot_cmpl', 'tot_f1_mean', 'n_empty_gt'):
            if getattr(g, name) != getattr(w, name):          # float64 totals: bit for bit
                bad.append('%s: fscore[%d].%s %r != %r' % (what, h, name, getattr(g, name), getattr(w, name)))


def _worker(rank, world, port, case, tmp, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    import torch
    import torch.distributed as dist
    from preworld_amd import harness, synth as S
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        dev = 'cuda:0'
        torch.cuda.set_device(0)
        net = harness.build_model(harness.model_cfg(S.GRID_CONFIG_C1), S.synth_state_dict(0), dev)
        bad, info = [], {}
        if case == 'miss':
            samples = _samples(6, dev, miss=3)
            st = {}
            rep, none, metric = harness.evaluate_stream(net, iter(samples), in_flight=2, fscore=FSCORE, distributed=True, stats=st)
            want_rep, _, _ = harness.evaluate(net, samples, dev)
            info = dict(stats=st, report=rep, evaluate=want_rep)
            if st['all']['recalibrations'] < 1 or (rank == 1) != (st['recalibrations'] >= 1):
                bad.append('the range miss of sample 3 (rank 1) was not repaired there: %s' % st)
            if metric.cnt != 6 or any(metric.metrics[h].cnt != 6 or metric.fscore[h].cnt != 6 for h in HZ):
                bad.append('counts %d, not 6' % metric.cnt)
            for h in HZ:
                n_hist = int(metric.metrics[h]._hist.sum())
                n_occ = int(metric.metrics[h]._occ_hist.sum())
                if n_hist != sum(int((s['mask_camera'] & (s['gt'][h] < 18)).sum()) for s in samples):
                    bad.append('horizon %d: confusion total %d' % (h, n_hist))
                if n_occ != sum(int(s['mask_camera'].sum()) for s in samples):
                    bad.append('horizon %d: occ_hist total %d' % (h, n_occ))
            for h in list(HZ) + ['avg_future']:
                if abs(rep[h] - want_rep[h]) > 0.01:
                    bad.append('mIoU %s: %s vs evaluate %s' % (h, rep[h], want_rep[h]))
        else:
            n = 5 if case == 'five' else 1
            items = _samples(n, dev, empty_gt=2 if n == 5 else None)
            samples = _Recording(items)
            dump = os.path.join(tmp, 'dist')
            st = {}
            rep, none, metric = harness.evaluate_stream(net, samples, in_flight=2, fscore=FSCORE, distributed=True,
                                                        dump_dir=dump, stats=st)
            read = sorted(samples.read)
            # the same samples in ONE process (the group is initialised: distributed=False must not use it)
            st1 = {}
            want_rep, stacks, want = harness.evaluate_stream(net, items, in_flight=2, fscore=FSCORE, keep_stacks=True,
                                                             dump_dir=os.path.join(tmp, 'single%d' % rank), stats=st1)
            info = dict(stats=st, read=read, report=rep, n_empty_gt=[metric.fscore[h].n_empty_gt for h in HZ],
                        fscore={h: metric.fscore[h].tot_f1_mean for h in HZ})
            if none is not None or rep != want_rep:
                bad.append('report %s != single process %s' % (rep, want_rep))
            _compare(metric, want, bad, 'rank %d' % rank)
            if st['all']['recalibrations'] or st1['recalibrations']:
                bad.append('recalibrations: distributed %s, single %s' % (st['all'], st1['recalibrations']))
            if read != sorted({0} | set(range(rank, n, world))):
                bad.append('rank %d read items %s' % (rank, read))
            if st['samples'] != len(range(rank, n, world)) or st['n_samples'] != n:
                bad.append('stats %s' % st)
            if n == 5 and any(metric.fscore[h].n_empty_gt != 1 for h in HZ):
                bad.append('n_empty_gt %s, not 1' % info['n_empty_gt'])
            dist.barrier()
            if rank == 0:                              # the union of both ranks' files is the single-process dump
                def files(root):
                    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)
                got_files, want_files = files(dump), files(os.path.join(tmp, 'single0'))
                names = [os.path.join('scene-%04d' % (i // 2), 'tok%02d.npy' % i) for i in range(n)]
                if got_files != want_files or got_files != sorted(names):
                    bad.append('dumped %s, single process %s' % (got_files, want_files))
                for i, name in enumerate(names):
                    a = np.load(os.path.join(dump, name))
                    b = np.load(os.path.join(tmp, 'single0', name))
                    if a.shape != (1, 4, 100, 100, 8) or a.dtype != np.uint8 or not np.array_equal(a, b) \
                            or not np.array_equal(a[0], stacks[i]):
                        bad.append('dump %s: %s %s differs' % (name, a.shape, a.dtype))
        q.put((rank, bad, info))
    except Exception as e:
        q.put((rank, ['raised %r' % (e,)], {}))
        raise
    finally:
        dist.destroy_process_group()


def _run(case, tmp):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, case, str(tmp), q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=600) for _ in procs], key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.terminate()
    for rank, bad, info in res:
        print('[eval dist %s] rank %d: %s' % (case, rank, info))
    assert [r[0] for r in res] == [0, 1]
    assert all(p.exitcode == 0 for p in procs)
    assert not [b for r in res for b in r[1]], [r[1] for r in res]
    return res


def test_five_samples_split_3_2_equal_one_process(tmp_path):
    """rank 0 evaluates samples 0, 2, 4 and rank 1 samples 1, 3 (reading item 0 too); sample 2's GT is empty; both ranks return
    the single-process tables, report, count_iou / count_miou and F-score totals, and their dumps together are its dump"""
    res = _run('five', tmp_path)
    assert res[0][2]['read'] == [0, 2, 4] and res[1][2]['read'] == [0, 1, 3]


def test_one_sample_two_ranks_the_empty_rank_returns_the_result(tmp_path):
    res = _run('one', tmp_path)
    assert res[1][2]['stats']['samples'] == 0 and res[1][2]['report'] == res[0][2]['report']


def test_range_miss_on_one_rank_is_repaired_and_counted_once(tmp_path):
    """six samples from an iterable (every rank walks it), sample 3 far outside the calibrated window: rank 1 recalibrates"""
    _run('miss', tmp_path)
