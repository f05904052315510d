"""pipeline.StreamScheduler / SampleStream bookkeeping without a GPU: fake slots record what the scheduler asks of them --
results in input order for M = 1, 2, 3, one repair and one counted table for a replay that left its window, a re-capture when
the module's fingerprint changes -- and the metrics' add_counts against add_batch's arithmetic on CPU tensors."""
import numpy as np
import pytest
import torch

from preworld_amd import _lib, metrics
from preworld_amd.pipeline import SampleStream, StreamScheduler


class FakeSlot:
    """replays are instantaneous; `bad` maps a sample index to how many of its replays leave the window"""

    def __init__(self, log, bad):
        self.log, self.bad = log, bad
        self.current = None
        self.launches = 0

    def stage(self, sample):
        self.log.append(('stage', sample['i']))

    def load(self, sample):
        self.current = sample['i']
        self.log.append(('load', sample['i']))

    def launch(self, buf):
        self.launches += 1
        self.log.append(('launch', self.current, buf))

    def wait(self):
        self.log.append(('wait', self.current))

    def ranges_ok(self):
        if self.bad.get(self.current, 0) > 0:
            self.bad[self.current] -= 1
            return False
        return True

    def recalibrate(self):
        self.log.append(('recalibrate', self.current))

    def commit(self):
        self.log.append(('commit', self.current))

    def result(self, buf):
        return self.current


def _run(M, n, bad=None):
    log = []
    slots = [FakeSlot(log, dict(bad or {})) for _ in range(M)]
    sched = StreamScheduler(slots)
    got = list(sched.run({'i': i} for i in range(n)))
    return got, log, sched


@pytest.mark.parametrize('M', [1, 2, 3])
def test_results_come_out_in_input_order(M):
    got, log, sched = _run(M, 7)
    assert got == list(range(7))
    assert sched.replays == 7 and sched.recalibrations == 0
    assert [e[1] for e in log if e[0] == 'commit'] == list(range(7))
    # a slot's previous sample is finished (waited on, committed) before the slot takes the next one; nothing else is waited on
    for i in range(M, 7):
        assert log.index(('commit', i - M)) < log.index(('load', i))
        assert log.index(('wait', i - M)) < log.index(('load', i))
    # M samples in flight: sample i is enqueued before sample i - M + 1 is waited on
    for i in range(M - 1, 7):
        if i - M + 1 >= 0:
            assert log.index(('load', i)) < log.index(('wait', i - M + 1))
    # two payload buffers per slot alternate
    bufs = [e[2] for e in log if e[0] == 'launch']
    assert bufs == [(i // M) % 2 for i in range(7)]


def test_lazy_generator_yields_oldest_after_enqueueing_the_next():
    log = []
    slots = [FakeSlot(log, {}) for _ in range(2)]
    it = StreamScheduler(slots).run({'i': i} for i in range(5))
    assert next(it) == 0
    assert ('load', 2) in log and ('wait', 1) not in log     # sample 2 was enqueued before sample 0 was handed out


def test_a_failed_range_check_is_repaired_once_and_counted_once():
    got, log, sched = _run(2, 6, bad={3: 1})
    assert got == list(range(6))
    assert sched.recalibrations == 1 and sched.replays == 7
    assert [e[1] for e in log if e[0] == 'commit'] == list(range(6))
    i_rec = log.index(('recalibrate', 3))
    assert log[i_rec + 1][:2] == ('launch', 3)                 # the same static inputs replayed, into the same payload buffer
    assert log[i_rec + 1][2] == [e for e in log if e[:2] == ('launch', 3)][0][2]
    assert log.index(('commit', 3)) > i_rec


def test_a_replay_that_stays_outside_raises_and_is_not_counted():
    with pytest.raises(_lib.PreworldHipError):
        _run(2, 6, bad={2: 2})
    log = []
    slots = [FakeSlot(log, {2: 2}) for _ in range(2)]
    it = StreamScheduler(slots).run({'i': i} for i in range(6))
    with pytest.raises(_lib.PreworldHipError):
        list(it)
    assert ('commit', 2) not in log


class _FakeNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(3))
        self.register_buffer('rm', torch.zeros(3))


def test_fingerprint_change_recaptures(monkeypatch):
    captures = []

    def fake_capture(self):
        captures.append(1)
        self.slots = [FakeSlot([], {}) for _ in range(self.in_flight)]
        self._fp = self._fingerprint()
    monkeypatch.setattr(SampleStream, '_capture', fake_capture)
    net = _FakeNet()
    frames = [{'bda': torch.zeros(1, 3, 3)}]
    st = SampleStream(net, frames, in_flight=2, payload=False)
    assert len(captures) == 1
    assert list(st.run({'i': i} for i in range(3))) == [0, 1, 2]
    assert len(captures) == 1 and st.recaptures == 0 and st.replays == 3
    net.load_state_dict({'w': torch.full((3,), 2.0), 'rm': torch.ones(3)})
    assert list(st.run({'i': i} for i in range(2))) == [0, 1]
    assert len(captures) == 2 and st.recaptures == 1 and st.replays == 5
    list(st.run({'i': i} for i in range(2)))
    assert len(captures) == 2
    with torch.no_grad():
        net.rm.add_(1.0)                                          # an in-place buffer update bumps its version
    list(st.run({'i': i} for i in range(1)))
    assert len(captures) == 3


def _np_table(pred, gt, mask, n_cl):
    """numpy restatement: hist_info (occ_metrics.py:82-105) + the binary histogram of add_batch (:150-154)"""
    m = np.ones(gt.shape, bool) if mask is None else mask.astype(bool)
    k = m & (gt < n_cl)
    hist = np.bincount(n_cl * gt[k].astype(np.int64) + pred[k], minlength=n_cl * n_cl)
    free = n_cl - 1
    b = np.bincount(2 * (gt[m] != free).astype(np.int64) + (pred[m] != free), minlength=4)
    return np.concatenate([hist, b]).astype(np.int64)


def test_add_counts_equals_add_batch_arithmetic():
    """the device-table path of the metrics against the reference arithmetic on CPU tensors (hist_info + the binary
    histogram), through the temporal metric's attributes and report()"""
    rs = np.random.RandomState(5)
    shape = (6, 5, 4)
    m = metrics.Metric_mIoU_Temporal(num_classes=18, use_image_mask=True, device='cpu')
    want = {h: np.zeros(18 * 18 + 4, np.int64) for h in (0, 2, 4, 6)}
    for _ in range(3):
        rows = []
        mask = rs.rand(*shape) < 0.7
        for h in (0, 2, 4, 6):
            pred = rs.randint(0, 18, shape).astype(np.uint8)
            gt = rs.randint(0, 18, shape).astype(np.uint8)
            gt[rs.rand(*shape) < 0.1] = 255
            t = _np_table(pred, gt, mask, 18)
            want[h] += t
            rows.append(t)
        m.add_counts(torch.from_numpy(np.stack(rows)))
    assert m.cnt == 3 and all(m.metrics[h].cnt == 3 for h in (0, 2, 4, 6))
    for h in (0, 2, 4, 6):
        assert np.array_equal(getattr(m, 'hist_%ds' % (h // 2)), want[h][:324].reshape(18, 18).astype(np.float64))
        assert np.array_equal(getattr(m, 'occ_hist_%ds' % (h // 2)), want[h][324:].reshape(2, 2).astype(np.float64))
    rep = m.report()
    assert set(rep) == {0, 2, 4, 6, 'avg_future'}
    with pytest.raises(ValueError):
        m.add_counts(torch.zeros(3, 328, dtype=torch.int64))
    one = metrics.Metric_mIoU(num_classes=18, device='cpu')
    one.add_counts(torch.from_numpy(want[0]), n=3)
    assert one.cnt == 3 and np.array_equal(one.hist, want[0][:324].reshape(18, 18))
    with pytest.raises(ValueError):
        one.add_counts(torch.zeros(10, dtype=torch.int64))
