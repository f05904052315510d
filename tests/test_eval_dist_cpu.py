"""Sharded evaluation (harness.evaluate_stream(distributed=True)) without a GPU: which rank evaluates which sample, the deferred
F-score rows a StreamScheduler writes at global indices (fake slots, a range miss included), the cross-rank reduction of
parallel.reduce_eval_counts under a 2-rank gloo group (a rank with no sample included) and the argument errors."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from preworld_amd import harness, metrics, parallel
from preworld_amd.pipeline import SampleStream, StreamScheduler

HZ = (0, 2, 4, 6)
NB = 18 * 18 + 4


@pytest.mark.parametrize('n,world', [(5, 2), (3, 8), (2, 2), (8, 8), (1, 2), (7, 3), (0, 2)])
def test_every_sample_is_evaluated_once_in_order(n, world):
    shards = [list(parallel.eval_shard(n, r, world)) for r in range(world)]
    assert sorted(i for s in shards for i in s) == list(range(n))          # each index exactly once: no padded duplicate
    for r, s in enumerate(shards):
        assert s == sorted(s) and all(i % world == r for i in s)
    if n < world:
        assert all(shards[r] == [] for r in range(n, world))
    assert [list(parallel.eval_shard(5, r, 2)) for r in range(2)] == [[0, 2, 4], [1, 3]]


def _counts(i):
    """stand-in per-sample tables of global sample i: (H, n_cl*n_cl + 4) mIoU counts and (H, 4) F-score counts"""
    rs = np.random.RandomState(100 + i)
    return (torch.from_numpy(rs.randint(0, 50, (len(HZ), NB)).astype(np.int64)),
            torch.from_numpy(rs.randint(0, 1000, (len(HZ), 4)).astype(np.int64)))


class _RowSlot:
    """a fake slot whose commit(index) writes the sample's F-score row through SampleStream's own deferred-row table"""

    def __init__(self, owner, log, bad):
        self.owner, self.log, self.bad = owner, log, bad
        self.current = None

    def stage(self, sample):
        pass

    def load(self, sample):
        self.current = sample['i']

    def launch(self, buf):
        self.log.append(('launch', self.current))

    def wait(self):
        pass

    def ranges_ok(self):
        if self.bad.get(self.current, 0) > 0:
            self.bad[self.current] -= 1
            return False
        return True

    def recalibrate(self):
        self.log.append(('recalibrate', self.current))

    def commit(self, index):
        self.log.append(('commit', self.current, index))
        self.owner._fs_row(index).copy_(_counts(self.current)[1])

    def result(self, buf):
        return self.current


def _row_owner():
    st = SampleStream.__new__(SampleStream)                  # only the deferred-row table of a stream: no capture, no GPU
    st.horizons, st.fs_rows, st.fs_totals = HZ, None, torch.zeros(len(HZ), 3, dtype=torch.float64)
    return st


@pytest.mark.parametrize('M', [1, 2, 3])
def test_deferred_fscore_rows_land_at_their_global_index(M):
    # rank 1 of 3 over a 40-sample split: global samples 1, 4, 7, ..., 37; sample 13 leaves its window once
    own = list(parallel.eval_shard(40, 1, 3))
    owner, log = _row_owner(), []
    sched = StreamScheduler([_RowSlot(owner, log, {13: 1}) for _ in range(M)])
    got = list(sched.run(((i, {'i': i}) for i in own), indexed=True))
    assert got == own
    assert sched.recalibrations == 1 and sched.replays == len(own) + 1
    commits = [e for e in log if e[0] == 'commit']
    assert [e[1] for e in commits] == own and all(e[1] == e[2] for e in commits)      # once each, with its own index
    i_rec = log.index(('recalibrate', 13))
    assert log[i_rec + 1] == ('launch', 13) and log.index(('commit', 13, 13)) > i_rec
    rows = owner.fs_rows
    assert rows.dtype == torch.int64 and rows.shape[0] >= 38 and rows.shape[1:] == (len(HZ), 4)   # grown on demand
    for i in range(rows.shape[0]):
        want = _counts(i)[1] if i in own else torch.zeros(len(HZ), 4, dtype=torch.int64)
        assert torch.equal(rows[i], want), i


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _reduce_worker(rank, world, port, n, capacity, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        m = metrics.Metric_mIoU_Temporal(num_classes=18, use_image_mask=True, device='cpu')
        own = list(parallel.eval_shard(n, rank, world))
        # capacity None: the shortest table that holds this rank's rows (shorter than the split on rank 1 of 5 samples)
        rows = torch.zeros((capacity or (own[-1] + 1 if own else 0), len(HZ), 4), dtype=torch.int64)
        for i in own:
            t, r = _counts(i)
            m.add_counts(t)
            rows[i] = r
        counters, total = parallel.reduce_eval_counts(m, rows, n, [len(own), 10 * rank + 1], via_host=True)
        want = metrics.Metric_mIoU_Temporal(num_classes=18, use_image_mask=True, device='cpu')
        for i in range(n):
            want.add_counts(_counts(i)[0])
        ok = m.cnt == n and all(m.metrics[h].cnt == n for h in HZ)
        for h in HZ:
            ok = ok and torch.equal(m.metrics[h]._hist, want.metrics[h]._hist)
            ok = ok and torch.equal(m.metrics[h]._occ_hist, want.metrics[h]._occ_hist)
        ok = ok and m.report() == want.report()
        ok = ok and tuple(total.shape) == (n, len(HZ), 4) and total.dtype == torch.int64
        ok = ok and torch.equal(total, torch.stack([_counts(i)[1] for i in range(n)]))
        ok = ok and counters == [n, sum(10 * r + 1 for r in range(world))]
        # without the F-score: no row table, no MAX all-reduce -- the histograms alone
        m2 = metrics.Metric_mIoU_Temporal(num_classes=18, use_image_mask=True, device='cpu')
        for i in own:
            m2.add_counts(_counts(i)[0])
        c2, none = parallel.reduce_eval_counts(m2, None, n, [], via_host=True)
        ok = ok and none is None and c2 == [] and m2.cnt == n and m2.report() == want.report()
        q.put((rank, bool(ok), len(own)))
    except Exception as e:
        q.put((rank, repr(e), -1))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('n,capacity', [(5, 16), (5, None), (1, 16)], ids=['5-samples', '5-samples-short-table', '1-sample-empty-rank'])
def test_reduction_over_two_gloo_ranks_is_exact(n, capacity):
    """rank 0 gets 3 of 5 samples, rank 1 gets 2 (or none of 1); local row tables longer or shorter than the split"""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, n, capacity, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=120) for _ in procs])
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.terminate()
    assert [r[0] for r in res] == [0, 1] and all(p.exitcode == 0 for p in procs)
    assert all(r[1] is True for r in res), res
    assert [r[2] for r in res] == [len(parallel.eval_shard(n, r, 2)) for r in range(2)]


def test_argument_errors():
    sample = dict(frames=[], ego=torch.zeros(1, 1, 21), gt={h: np.zeros((2, 2, 2), np.uint8) for h in HZ})
    assert not dist.is_initialized()
    with pytest.raises(ValueError, match='dump_dir'):
        harness.evaluate_stream(None, [sample], keep_stacks=True, distributed=True)
    with pytest.raises(ValueError, match='process group'):
        harness.evaluate_stream(None, [sample], distributed=True)
    with pytest.raises(ValueError, match='scene_name'):
        harness.evaluate_stream(None, [sample], dump_dir='unused')
    with pytest.raises(ValueError, match='scene_name'):
        harness.evaluate_stream(None, [dict(sample, scene_name='scene-0001')], dump_dir='unused')
