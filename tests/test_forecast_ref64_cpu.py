"""tests/_forecast_ref64.py must be trusted before it judges a kernel: the float64 step, plan_head and attribute MLPs against the
float32 oracle and the reference model's stored outputs (tests/golden/forecast_small.npz), the accumulator-order permutation
against the hand-written loop of test_gpu_range.py, and every condition a regime of tests/test_gpu_forecast_ref64.py relies on,
proven in float64 so that a later change of seed cannot empty a regime.  No GPU."""
import numpy as np
import pytest

import _forecast_ref64 as R
from oracle import oracle as O
from preworld_amd import synth as S


def _sd_blocks(sd, names=('density_mlp', 'semantic_mlp', 'color_mlp')):
    return [(sd[n + '.0.weight'], sd[n + '.0.bias'], sd[n + '.2.weight'], sd[n + '.2.bias']) for n in names]


def _plan(sd):
    return [sd['plan_head.%d.%s' % (i, k)] for i in (0, 2, 4) for k in ('weight', 'bias')]


def test_step_and_plan_head_vs_oracle_and_golden(golden):
    """A sequential float32 sum of K terms is off by at most K 2^-24 sum|terms|, by about sqrt(K) of it when the roundings are
    independent: the oracle's two layers (K = 64 + 128) must sit within 16 units of the normaliser, and so must the stored reference
    states, which are float32 outputs of the reference model chained over six steps (each compared from the stored state before)."""
    g = golden('forecast_small.npz')
    sd = S.synth_state_dict(int(g['seed_sd']))
    v = np.random.RandomState(int(g['seed_v'])).standard_normal((1, 8, 8, 4, 32)).astype(np.float32).reshape(-1, 32)
    ego = S.ego_state(int(g['seed_ego'])).reshape(1, 21)
    e, bd_e = R.plan_head64(ego, *_plan(sd))
    eo = O.plan_head(ego, sd)
    qe_o, qe_g = R.q_of(eo, e, bd_e), R.q_of(g['ego_feat'], e, bd_e)
    W1, b1, W2, b2 = [sd['fusion_head.%s' % k] for k in ('0.weight', '0.bias', '2.weight', '2.bias')]
    c1 = R.c1_64(eo, W1, b1)[0][0]
    want = R.step64(v, W1[:, :32], c1, W2, b2)
    q_o = R.q_of(O.forecast_step(v, eo[0], sd), want, R.step_bound(v, W1[:, :32], c1, W2, b2))
    print('\n[ref64] plan_head: oracle %.2f, stored reference %.2f units; one step: oracle %.2f units' % (qe_o, qe_g, q_o))
    assert qe_o <= 16 and qe_g <= 16 and q_o <= 16
    np.testing.assert_allclose(e, g['ego_feat'], rtol=1e-4, atol=1e-5)
    c1g = R.c1_64(g['ego_feat'], W1, b1)[0][0]
    states = g['states'].reshape(7, -1, 32)
    for k in range(6):
        q = R.q_of(states[k + 1], R.step64(states[k], W1[:, :32], c1g, W2, b2), R.step_bound(states[k], W1[:, :32], c1g, W2, b2))
        assert q <= 16, (k, q)
    np.testing.assert_allclose(R.chain64(v, W1[:, :32], c1g, W2, b2, 6), states[1:], rtol=2e-4, atol=2e-4)
    # the float32 restatements are float32 all the way and agree with float64 to their own precision
    assert R.q_of(R.plan_head32(ego, *_plan(sd)), e, bd_e) <= 16 and R.step32(v, W1[:, :32], c1, W2, b2).dtype == np.float32


def test_attribute_mlps_vs_oracle_and_golden(golden):
    g = golden('forecast_small.npz')
    sd = S.synth_state_dict(int(g['seed_sd']))
    v = np.random.RandomState(int(g['seed_v'])).standard_normal((1, 8, 8, 4, 32)).astype(np.float32)
    out, bd = R.attr64(v.reshape(-1, 32), _sd_blocks(sd), True)
    pre, _ = R.attr64(v.reshape(-1, 32), _sd_blocks(sd), False)
    np.testing.assert_array_equal(out[:, 2:], pre[:, 2:])                       # the density softplus touches channels 0 and 1 only
    np.testing.assert_allclose(out[:, :2], R.softplus(pre[:, :2]), rtol=1e-15)
    assert not out[:, 22:].any() and not bd[:, 22:].any()
    _, dens, sem = O.attribute_decode(v, sd)
    qd = R.q_of(dens.reshape(-1), out[:, 0], bd[:, 0])
    qs = R.q_of(sem.reshape(-1, 17), out[:, 2:19], bd[:, 2:19])
    print('\n[ref64] attribute MLPs: oracle density %.2f, semantic %.2f units' % (qd, qs))
    assert qd <= 16 and qs <= 16                                                 # K = 32 + 64 sequential float32 terms, as above
    np.testing.assert_allclose(out[:, 0:2], g['density'].reshape(-1, 2), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(out[:, 2:19], g['semantic'].reshape(-1, 17), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(out[:, 19:22], g['color'].reshape(-1, 3), rtol=1e-4, atol=1e-4)
    # one block of 18 outputs (the BEVStereo4DOCC predicter's form): columns 18 .. 23 stay zero
    blk = R.attr_blocks(3, [18])
    o1, b1 = R.attr64(v.reshape(-1, 32)[:33], blk, False)
    assert o1.shape == (33, 24) and not o1[:, 18:].any() and not b1[:, 18:].any() and np.abs(o1[:, :18]).min() > 0
    assert R.q_of(R.attr32(v.reshape(-1, 32)[:33], blk, False), o1, np.maximum(b1, 1e-300)) <= 4


def test_c1_to_c1p_is_the_accumulator_permutation():
    c1 = np.random.RandomState(1).standard_normal((3, 128)).astype(np.float32)
    c1p = R.c1_to_c1p(c1)
    want = np.zeros_like(c1)
    for s in range(3):                              # the loop test_gpu_range.py states by hand
        for h in range(2):
            for tile in range(4):
                for r in range(16):
                    want[s, h * 64 + tile * 16 + r] = c1[s, tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h]
    np.testing.assert_array_equal(c1p, want)
    idx = R.c1_to_c1p(np.arange(128))
    assert sorted(idx.tolist()) == list(range(128)) and idx.shape == (128,)
    assert c1p.dtype == c1.dtype and c1p.flags['C_CONTIGUOUS']


@pytest.fixture(scope='module')
def stats():
    return {name: R.regime_stats(R.regime(name)) for name in R.REGIMES}


def test_regime_conditions(stats):
    """what each regime is FOR, on the committed seed, in float64"""
    for name, s in stats.items():
        print('\n[ref64] %-14s growth %5.2f  z > 20: %.3f  z < -20: %.3f  max|v0| %.4f  max|states| %.4f'
              % (name, s['growth'], s['hi'], s['lo'], s['v0_max'], s['st_max']))
        assert s['growth'] <= 32, name
        for m in (s['v0_max'], s['st_max']):        # the slot offsets of the GPU test land where they are stated
            frac = np.log2(m) % 1.0
            assert 2.0 ** frac >= 1.001 and 2.0 ** (frac - 1) <= 0.999, (name, m)
    assert stats['dead']['lo'] == 1.0
    assert stats['linear']['hi'] >= 0.9
    assert stats['w1x64']['hi'] >= 0.4 and stats['w1x64']['lo'] >= 0.4
    assert stats['ego_x64']['hi'] >= 0.2 and stats['ego_x64']['lo'] >= 0.2
    assert stats['base']['hi'] <= 0.01 and stats['base']['lo'] <= 0.01
    m = stats['mixed_samples']                      # per sample: base, ego_x64, dead
    assert m['hi_s'][0] <= 0.01 and m['lo_s'][0] <= 0.01 and m['hi_s'][1] >= 0.2 and m['lo_s'][1] >= 0.2 and m['lo_s'][2] == 1.0
    assert np.abs(R.regime('w1x64')['W1a']).sum(1).max() > 300


@pytest.mark.parametrize('name', list(R.REGIMES))
def test_float32_yardstick(name):
    """q32 of the float32 restatement, step by step on its own states.  Bd counts the rounding of every operand and intermediate
    once, in the worst direction; a float32 evaluation rounds each of them once and its sums in numpy's blocked order a few times
    more, so it has to land at a few units: above 4 the yardstick, and with it every GPU bound, would be slack."""
    d = R.regime(name)
    v, qs = d['v0'], []
    for _ in range(R.N_STEPS):
        nxt = R.step32(v, d['W1a'], d['c1'], d['W2'], d['b2'])
        q, q32 = R.step_q(nxt, v, d['W1a'], d['c1'], d['W2'], d['b2'])
        assert q == q32
        qs.append(q32)
        v = nxt
    print('\n[ref64] %-14s q32 per step: %s' % (name, ' '.join('%.2f' % q for q in qs)))
    assert 0 < min(qs) and max(qs) <= 4.0, (name, qs)
