"""pw_forecast_steps, pw_forecast_steps_h2, pw_forecast_prologue and pw_attr_mlp against float64, one recursion step at a time
(tests/_forecast_ref64.py; the reference and every regime condition are proven on the CPU in tests/test_forecast_ref64_cpu.py).

Every comparison prints  q = max |got - ref| / (2^-24 Bd)  beside q32, the same figure of a float32 restatement on the same inputs,
and asserts  q <= 2 q32 + 1  (_forecast_ref64.bound).  The reference of state k + 1 is the float64 step of the kernel's own fp32
state k, so the recursion's amplification is in no bound.  The split-fp16 kernel keeps its state in fp32 registers whatever the
output format; a run with h2 output is therefore judged from the fp32 states of the same launch repeated with fp32 output (the two
are byte-equal up to the storage split, test_formats_byte_for_byte), and its decoded output carries the storage format's own
rounding on top, which is reported as a separate figure `q_h2` and bounded with the format's floor (_judge).

MEASURED on an MI355X with the kernel as it is now (profiles/forecast_pin.md has every figure); the bound is met everywhere, the closest cases are
    pw_forecast_steps_h2, fp32 states     worst q 1.47 at q32 1.58 (ego_x64, states' slot at the bottom of the window), <= 0.37 of the bound
    pw_forecast_steps                     worst q 2.02 at q32 1.63 (w1/64);  1.84 at q32 0.74 (base sample of mixed_samples) = 0.74 of the bound
    pw_attr_mlp                           worst q 0.97 at q32 0.97
    pw_forecast_prologue                  worst q 3.87 at q32 3.45 (c1, B = 64, ego x 100)
    decoded h2 output                     2.95 of 3.00 with the slot at its ideal exponent or above (dead); 13.0 / 20.1 at the bottom of the
                                          window (dead / the dead sample of mixed_samples): the storage format's floor, _judge
"""
import numpy as np
import pytest
import torch

import _forecast_ref64 as R
from preworld_amd import _lib, ops
from preworld_amd import synth as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = np.float64

# voxels one launch covers before a wave takes a second trip of its grid-stride loop (blocks x 4 waves x tiles per trip x 32 voxels):
CAP_FP32 = 1280 * 4 * 32          # pw_forecast.hip:230  nb = min(want, 1280)              -> 163 840
CAP_H2 = 512 * 4 * 2 * 32         # pw_forecast.hip:510  nb = min(want, 512), two tiles    -> 131 072
CAP_ATTR = 768 * 4 * 32           # pw_forecast.hip:614  nb = min(want, 768)               ->  98 304


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _nans(shape):
    """output buffers start as NaN: an element a kernel does not write can then not pass for the result of an earlier launch that
    the allocator's reused block still holds"""
    return torch.full(shape, float('nan'), device=DEV, dtype=torch.float32)


def _dev(d):
    """device operands of a draw / regime, packed for both forecast kernels (once per dict)"""
    if 'dev' not in d:
        d.setdefault('W1a', np.ascontiguousarray(d['W1'][:, :32]))
        W1, W2 = T(d['W1']), T(d['W2'])
        d['dev'] = dict(pack32=ops.forecast_pack(W1, W2), pack_h2=ops.forecast_pack_h2(W1, W2), c1p=T(R.c1_to_c1p(d['c1'])), b2=T(d['b2']))
    return d['dev']


def _slot_ctx(exps):
    ctx = ops.RangeCtx(DEV, n_slots=len(exps))
    ctx.tab[:, 0] = torch.tensor(exps, dtype=torch.int32, device=DEV)
    return ctx


def _ideal_exps(d, n_steps):
    """the exponents calibration would settle on: the largest |v0| and the largest state magnitude (float64) in [2^12, 2^13)"""
    st = R.chain64(d['v0'], d['W1a'], d['c1'], d['W2'], d['b2'], n_steps)
    return ops.RangeCtx.ideal_exp(float(np.abs(d['v0']).max())), ops.RangeCtx.ideal_exp(float(np.abs(st).max()))


def _run_fp32(d, n_steps, v0=None):
    g = _dev(d)
    v0 = T(d['v0']) if v0 is None else v0
    return ops.forecast_steps(v0, d['v0'].shape[0], g['pack32'][0], g['pack32'][1], g['c1p'], g['b2'], n_steps, states=_nans((n_steps,) + tuple(v0.shape)))


def _run_h2(d, n_steps, e0, e1, in_h2, out_h2, v0=None):
    """pw_forecast_steps_h2 under two hand-set slots (0: v0, 1: states).  Returns (ctx, x = v0 as the kernel reads it in fp32, out)"""
    g = _dev(d)
    ctx = _slot_ctx([e0, e1])
    v0 = T(d['v0']) if v0 is None else v0
    xh = ops.f32_to_h2(v0, out=ops.H2(torch.empty_like(v0), ctx.tab[0]))
    x = ops.h2_to_f32(xh)
    buf = _nans((n_steps,) + tuple(v0.shape))
    out = ops.forecast_steps_h2(xh if in_h2 else x, d['v0'].shape[0], g['pack_h2'], g['c1p'], g['b2'], n_steps,
                                states=ops.H2(buf, ctx.tab[1]), out_h2=out_h2)
    return ctx, x, out


def _judge(tag, prevs, gots, d, fails, sample=None, floor=0.0):
    """step k: gots[k] against the float64 step of prevs[k]; prints every figure, collects what misses the bound.  Returns the worst
    (q, its q32).

    floor > 0 is for a DECODED h2 output only: |got - ref| <= (2 q32 + 1) 2^-24 Bd + floor with floor = 2^-25 2^e, the storage
    format's absolute resolution -- lo = fp16(u - hi) is subnormal for |u| < 2^-3 stored units and resolves 2^-25 of them (pw_h2.h
    "Range").  Measured: with the states' slot at its ideal exponent or above the decoded output meets the plain bound (the floor
    is then negligible); at the bottom of the accepted window (d = -6), where the floor is 2^-31.5 of the tensor's maximum instead of
    2^-37.5, `dead` reaches q = 13 and the dead sample of `mixed_samples` 20.  The term of the normaliser that carries it is
    |v| + |b2| (in `dead` there is no hidden term), and it is not the kernel's arithmetic: the fp32 states of the same launch sit at
    q = 1.00 at every offset.  So the bound of a decoded output is widened by exactly that floor and nothing else.
    In `dead` at the ideal exponent the decoded output sits at 2.95 of 3.00.  That IS the worst case by construction -- one fp32
    rounding of v + b2 (q32 = 1, one unit) plus the two-plane split's 2^-23 relative (two units) on a normaliser that is just
    |v| + |b2| -- so a reseed lands on the same edge, never beyond it."""
    W1a, c1, W2, b2 = d['W1a'], d['c1'] if sample is None else d['c1'][sample], d['W2'], d['b2']
    worst = (0.0, 0.0, -1.0)
    for k in range(len(gots)):
        ref = R.step64(prevs[k], W1a, c1, W2, b2)
        bd = R.step_bound(prevs[k], W1a, c1, W2, b2)
        q32 = R.q_of(R.step32(prevs[k], W1a, c1, W2, b2), ref, bd)
        err = np.abs(gots[k] - ref)
        q = float((err / (R.EPS * bd)).max())
        r = float((err / (R.bound(q32) * R.EPS * bd + floor)).max())
        ok = bool(np.isfinite(gots[k]).all()) and r <= 1.0
        print('[pin-step] %-58s step %d  q %6.2f  q32 %5.2f  bound %5.2f%s%s' % (
            tag, k + 1, q, q32, R.bound(q32), '  with the storage floor: %.2f of the bound' % r if floor else '', '' if ok else '   <-- MISS'))
        if not ok:
            fails.append((tag, k + 1, round(q, 3), round(q32, 3), round(r, 3)))
        if q / R.bound(q32) > worst[2]:
            worst = (q, q32, q / R.bound(q32))
    return worst[:2]


def _chain_prevs(x, got):
    return [x] + [got[k] for k in range(len(got) - 1)]


# ------------------------------------------------------------------------------------------ a. tiles, pairs, samples, steps
SHAPES = [(1, 1), (1, 31), (1, 32), (1, 33), (1, 64), (1, 65), (3, 37), (2, 105), (64, 5)]


@pytest.mark.parametrize('n_steps', [1, 7])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_tiles_pairs_samples_steps(shape, n_steps):
    """partial tiles, one pair, a pair plus a lone partial tile, sample boundaries inside a tile and a pair, 64 samples (the dynamic
    LDS of k_forecast_h2 is then exactly 64 KB); every sample has its own c1"""
    d = R.draw(*shape)
    _dev(d)
    fails = []
    got = N(_run_fp32(d, n_steps)).astype(F64)
    assert got.shape == (n_steps,) + d['v0'].shape
    q = _judge('a fp32 %dx%d' % shape, _chain_prevs(d['v0'], got), got, d, fails)
    print('[pin] a | fp32 | %dx%d steps %d | q %.2f | q32 %.2f' % (shape + (n_steps,) + q))
    e0, e1 = _ideal_exps(d, n_steps)
    ctx, x, out = _run_h2(d, n_steps, e0, e1, in_h2=False, out_h2=False)
    got = N(out).astype(F64)
    q = _judge('a h2 (fp32 i/o) %dx%d' % shape, _chain_prevs(N(x), got), got, d, fails)
    print('[pin] a | h2 | %dx%d steps %d | q %.2f | q32 %.2f' % (shape + (n_steps,) + q))
    ctx.fold()
    assert ctx.check() == []
    assert not fails, fails


@pytest.mark.parametrize('n_vox', sorted({s * n for s, n in SHAPES}))
def test_attr_mlp_tiles(n_vox):
    blocks = R.attr_blocks(7, [2, 17, 3])
    v = (np.random.RandomState(8).standard_normal((n_vox, 32)) * 2).astype(np.float32)
    _attr_case('a attr %d voxels' % n_vox, v, blocks, True)


def _modules(blocks):
    ms = []
    for W1, b1, W2, b2 in blocks:
        m = torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.Softplus(), torch.nn.Linear(64, W2.shape[0])).to(DEV)
        with torch.no_grad():
            for p, a in zip((m[0].weight, m[0].bias, m[2].weight, m[2].bias), (W1, b1, W2, b2)):
                p.copy_(T(a))
        ms.append(m)
    return ms


def _attr_case(tag, v, blocks, final_softplus, packed=None):
    packed = packed or ops.pack_mlp_blocks(_modules(blocks))
    got = N(ops.attr_mlp(T(v), packed, final_softplus=final_softplus, out=_nans((v.shape[0], 24))))
    n_used = sum(b[2].shape[0] for b in blocks)
    ref, bd = R.attr64(v, blocks, final_softplus)
    assert got.shape == (v.shape[0], 24) and np.isfinite(got).all()
    assert not got[:, n_used:].any(), 'unused columns must be exactly 0'
    q = R.q_of(got[:, :n_used], ref[:, :n_used], bd[:, :n_used])
    q32 = R.q_of(R.attr32(v, blocks, final_softplus)[:, :n_used], ref[:, :n_used], bd[:, :n_used])
    print('[pin] %s | q %.2f | q32 %.2f | bound %.2f' % (tag, q, q32, R.bound(q32)))
    assert q <= R.bound(q32), (tag, q, q32)
    return got


def test_more_than_64_samples_is_refused():
    """the argument check of pw_forecast_steps_h2 itself: operands are built first, nothing is launched"""
    d = R.draw(65, 1)
    g = _dev(d)
    v0, states = T(d['v0']), _nans((1, 65, 1, 32))
    with pytest.raises(_lib.PreworldHipError, match='<= 64 samples'):
        ops.forecast_steps_h2(v0, 65, g['pack_h2'], g['c1p'], g['b2'], 1, states=states)
    torch.cuda.synchronize()
    assert bool(torch.isnan(states).all())


# ------------------------------------------------------------------------------------------ b. several trips, placement invariance
def test_several_trips_and_placement_invariance():
    """2 x 82 019 voxels (5 127 tiles: the last pair has an empty second tile, the last tile 6 voxels, the sample boundary is mid
    tile), above the grid caps of all three kernels, filled by repeating 211 distinct voxels per sample (211 mod 64 = 19 is coprime to
    64: every voxel visits every lane and both tiles of a pair).  Every copy must be bit-identical to its first copy; the first
    copies are compared with float64."""
    NB, NV, n_steps = 211, 82019, 2
    assert 2 * NV > max(CAP_FP32, CAP_H2, CAP_ATTR) and (2 * NV + 31) // 32 == 5127 and 2 * NV % 32 == 6 and NV % 32
    d = R.draw(2, NB)
    idx = torch.arange(NV, device=DEV) % NB
    v0 = T(d['v0'])[:, idx].contiguous()                                  # (2, NV, 32)
    fails = []

    def copies_equal(name, st):                                            # st (steps, 2, NV, ch)
        first = st[:, :, :NB]
        same = bool(torch.equal(_bits(st), _bits(first[:, :, idx])))
        if not same:
            bad = (_bits(st) != _bits(first[:, :, idx])).any(-1).nonzero()
            fails.append((name, 'copies differ', bad[:4].tolist(), int(bad.shape[0])))
        return N(first)

    got = copies_equal('fp32', _run_fp32(d, n_steps, v0=v0)).astype(F64)
    q = _judge('b fp32 2x82019', _chain_prevs(d['v0'], got), got, d, fails)
    print('[pin] b | fp32 | 2x82019 steps 2 | q %.2f | q32 %.2f' % q)
    e0, e1 = _ideal_exps(d, n_steps)
    ctx, x, out = _run_h2(d, n_steps, e0, e1, in_h2=True, out_h2=False, v0=v0)
    got = copies_equal('h2 fp32 out', out).astype(F64)
    q = _judge('b h2 2x82019', _chain_prevs(N(x[:, :NB]), got), got, d, fails)
    print('[pin] b | h2 | 2x82019 steps 2 | q %.2f | q32 %.2f' % q)
    ctx2, _, out_h = _run_h2(d, n_steps, e0, e1, in_h2=True, out_h2=True, v0=v0)
    copies_equal('h2 h2 out', out_h.buf)                                   # a voxel's 32 channels are one 128-byte row in h2 storage too
    again = ops.f32_to_h2(out, out=ops.H2(torch.empty_like(out), _slot_ctx([e1]).tab[0]))
    assert torch.equal(_bits(out_h.buf), _bits(again.buf)), 'h2 store path differs from pw_f32_to_h2 of the fp32 output'
    for c in (ctx, ctx2):
        c.fold()
        assert c.check() == []
    del out, out_h, again
    blocks = R.attr_blocks(7, [2, 17, 3])
    packed = ops.pack_mlp_blocks(_modules(blocks))
    grid = ops.attr_mlp(v0, packed, final_softplus=True, out=_nans((2, NV, 24)))
    assert tuple(grid.shape) == (2, NV, 24)
    first = copies_equal('attr', grid[None])[0].reshape(-1, 24)
    ref, bd = R.attr64(d['v0'].reshape(-1, 32), blocks, True)
    qa = R.q_of(first[:, :22], ref[:, :22], bd[:, :22])
    q32 = R.q_of(R.attr32(d['v0'].reshape(-1, 32), blocks, True)[:, :22], ref[:, :22], bd[:, :22])
    print('[pin] b | attr | 2x82019 | q %.2f | q32 %.2f' % (qa, q32))
    assert qa <= R.bound(q32) and not first[:, 22:].any()
    assert not fails, fails


# ------------------------------------------------------------------------------------------ c. formats, byte for byte
def test_formats_byte_for_byte():
    """x = v0 after the h2 round trip: fp32-in and h2-in runs are identical in each output format (all four combinations), the h2
    output (v_permlane32_swap store path) is the bytes pw_f32_to_h2 makes of the fp32 output under the same exponent, and `states=`
    as an ops.H2 with its own slot or as a raw buffer under the active RangeCtx write the same bytes and record the same maximum"""
    d = R.regime('base')
    n_steps = 3
    e0, e1 = _ideal_exps(d, n_steps)
    runs = {}
    for in_h2 in (False, True):
        for out_h2 in (False, True):
            ctx, x, out = _run_h2(d, n_steps, e0, e1, in_h2, out_h2)
            ctx.fold()
            assert ctx.check() == []
            runs[in_h2, out_h2] = (out.buf if out_h2 else out, ctx.compact.clone())
    for out_h2 in (False, True):
        assert torch.equal(_bits(runs[False, out_h2][0]), _bits(runs[True, out_h2][0])), 'fp32-in and h2-in differ (h2 out: %s)' % out_h2
        assert torch.equal(runs[False, out_h2][1][1], runs[True, out_h2][1][1])
    again = ops.f32_to_h2(runs[True, False][0], out=ops.H2(torch.empty_like(runs[True, False][0]), _slot_ctx([e1]).tab[0]))
    differ = (_bits(again.buf) != _bits(runs[True, True][0]))
    print('[pin] c | h2 store path vs pw_f32_to_h2 of the fp32 output: %d of %d words differ' % (int(differ.sum()), differ.numel()))
    assert not bool(differ.any())
    # states as a raw buffer: the slot comes from the active context (its first), same exponent -> same bytes, same record
    g = _dev(d)
    ctx_r = _slot_ctx([e1])
    xh = ops.f32_to_h2(T(d['v0']), out=ops.H2(torch.empty(d['v0'].shape, device=DEV), _slot_ctx([e0]).tab[0]))
    raw = _nans((n_steps,) + d['v0'].shape)
    with ops.use_range(ctx_r):
        ctx_r.begin()
        out = ops.forecast_steps_h2(xh, 2, g['pack_h2'], g['c1p'], g['b2'], n_steps, states=raw, out_h2=True)
    ctx_r.fold()
    assert out.buf.data_ptr() == raw.data_ptr() and out.rng.data_ptr() == ctx_r.tab[0].data_ptr()
    assert torch.equal(_bits(raw), _bits(runs[True, True][0])) and torch.equal(ctx_r.compact[0], runs[True, True][1][1])


# ------------------------------------------------------------------------------------------ d. regimes x position in the window
OFFSETS = [(-6, -6), (0, 0), (2, 2), (-6, 2)]       # (v0 slot, states slot): stored maximum in [2^(12+d), 2^(13+d))


@pytest.mark.parametrize('name', list(R.REGIMES))
def test_regimes_across_the_accepted_window(name):
    """h2 in / h2 out, 2 x 105 voxels (mixed_samples: 3 x 105), 6 steps, slots set by hand from the bottom [2^6, 2^7) to the top
    [2^14, 2^15) of the window a replayed graph is accepted in (RangeCtx.HARD_LO / HARD_HI, k_rng_audit): the bound holds, check()
    is empty and the audit counts nothing.  One bit outside on either side (d = -7, d = +4) check() and the audit both flag both
    slots; what such a run computes is not asserted (an Inf there is the documented behaviour), only that above the window the
    states do hold non-finite values and the states' slot says so.  In w1x8, w1x64 and dead that slot is flagged by NaN alone: a
    voxel with an Inf in v0 turns NaN in the first step and the voxels that stay finite stay inside the window.  The fp32 kernel
    runs each regime once; mixed_samples is judged per sample in both kernels."""
    d = R.regime(name)
    _dev(d)
    n_s = d['v0'].shape[0]
    fails = []
    got = N(_run_fp32(d, R.N_STEPS)).astype(F64)
    if n_s == 3:
        for s in range(3):
            q = _judge('d fp32 %s sample %d (%s)' % (name, s, R.MIXED[s]), _chain_prevs(d['v0'][s], got[:, s]), got[:, s], d, fails, sample=s)
            print('[pin] d | fp32 | %s/%s | - | q %.2f | q32 %.2f' % ((name, R.MIXED[s]) + q))
    else:
        q = _judge('d fp32 %s' % name, _chain_prevs(d['v0'], got), got, d, fails)
        print('[pin] d | fp32 | %s | - | q %.2f | q32 %.2f' % ((name,) + q))
    i0, i1 = _ideal_exps(d, R.N_STEPS)
    for d0, d1 in OFFSETS:
        ctx, x, out = _run_h2(d, R.N_STEPS, i0 - d0, i1 - d1, in_h2=True, out_h2=True)
        ctx.fold()
        ctx.audit()
        _, x32, st32 = _run_h2(d, R.N_STEPS, i0 - d0, i1 - d1, in_h2=True, out_h2=False)
        assert torch.equal(x, x32)
        st32 = N(st32).astype(F64)
        prevs = _chain_prevs(N(x), st32)
        dec = N(ops.h2_to_f32(out)).astype(F64)
        tag = 'd h2 %s (%+d, %+d)' % (name, d0, d1)
        floor = 2.0 ** (i1 - d1 - 25)                                  # 2^-25 stored units of the states' slot (_judge)
        sticky = ctx.sticky.tolist()
        print('[pin-slots] %s: check %s, audit %s, slots %s' % (tag, ctx.check(), sticky, ctx.compact.tolist()))
        if n_s == 3:                                                   # per sample: a small-ego sample keeps its accuracy beside a large one
            for s in range(3):
                ps = [p[s] for p in prevs]
                q = _judge('%s sample %d (%s)' % (tag, s, R.MIXED[s]), ps, st32[:, s], d, fails, sample=s)
                qh = _judge('%s sample %d (%s) h2 out' % (tag, s, R.MIXED[s]), ps, dec[:, s], d, fails, sample=s, floor=floor)
                print('[pin] d | h2 | %s/%s | %+d,%+d | q %.2f | q32 %.2f | q_h2 %.2f' % ((name, R.MIXED[s], d0, d1) + q + qh[:1]))
        else:
            q = _judge(tag, prevs, st32, d, fails)
            qh = _judge(tag + ' h2 out', prevs, dec, d, fails, floor=floor)
            print('[pin] d | h2 | %s | %+d,%+d | q %.2f | q32 %.2f | q_h2 %.2f' % ((name, d0, d1) + q + qh[:1]))
        if ctx.check() != [] or sticky[:3] != [0, 0, 1]:
            fails.append((tag, 'window', ctx.check(), sticky))
    for dd in (-7, 4):
        ctx, _, out = _run_h2(d, R.N_STEPS, i0 - dd, i1 - dd, in_h2=True, out_h2=True)
        ctx.fold()
        ctx.audit()
        sticky = ctx.sticky.tolist()
        nonfinite = not bool(torch.isfinite(ops.h2_to_f32(out)).all())
        print('[pin-slots] d h2 %s (%+d): check %s, audit %s, non-finite states: %s' % (name, dd, ctx.check(), sticky, nonfinite))
        if ctx.check() != [0, 1] or sticky[:3] != [2, 1, 1] or nonfinite != (dd > 0):
            fails.append((name, dd, 'both slots must be flagged by check() and by the audit', ctx.check(), sticky, nonfinite))
    assert not fails, fails


def test_nan_states_are_recorded_in_the_slot():
    """fp32 input with a NaN in three voxels: the states of those voxels are NaN from the first step on and the states' slot must say
    so (pw_h2.h: a NaN pattern is above every number; check() and the audit flag the slot) although a v_max_f32 drops a NaN.  Every
    other voxel is bit-identical to the run without them.  And with NaN in EVERY voxel the slot must not look unwritten."""
    d = R.regime('base')
    e0, e1 = _ideal_exps(d, 3)
    _, x, clean = _run_h2(d, 3, e0, e1, in_h2=False, out_h2=True)
    g = _dev(d)
    bad = [(0, 0, 5), (0, 104, 31), (1, 63, 0)]                        # (sample, voxel, channel): first lane, last voxel of a sample, a pair's second tile
    for every in (False, True):
        v0 = x.clone()
        if every:
            v0[:, :, 7] = float('nan')
        for s, i, c in bad:
            v0[s, i, c] = float('nan')
        ctx = _slot_ctx([e1])
        out = ops.forecast_steps_h2(v0, 2, g['pack_h2'], g['c1p'], g['b2'], 3, states=ops.H2(_nans((3,) + tuple(v0.shape)), ctx.tab[0]), out_h2=True)
        ctx.fold()
        ctx.audit()
        dec = ops.h2_to_f32(out)
        if not every:
            keep = torch.ones(2, 105, dtype=torch.bool, device=DEV)
            for s, i, _ in bad:
                keep[s, i] = False
                assert bool(torch.isnan(dec[:, s, i]).all())
            assert torch.equal(_bits(out.buf[:, keep]), _bits(clean.buf[:, keep]))
        else:
            assert bool(torch.isnan(dec).all())
        assert ctx.check() == [0] and ctx.sticky.tolist()[:3] == [1, 1, 1], (every, ctx.check(), ctx.sticky.tolist(), ctx.compact.tolist())


# ------------------------------------------------------------------------------------------ e. prologue
@pytest.mark.parametrize('scale', [1.0, 100.0])
@pytest.mark.parametrize('B', [1, 3, 64])
def test_prologue(B, scale):
    """plan_head and the hoisted ego term: every dot product's error in units of 2^-24 sum|terms| of that product, against a float32
    multiply-add chain in the kernel's order; c1p is c1 in accumulator order, bit for bit"""
    sd = S.synth_state_dict(4)
    plan = [sd['plan_head.%d.%s' % (i, k)] for i in (0, 2, 4) for k in ('weight', 'bias')]
    W1, b1 = sd['fusion_head.0.weight'], sd['fusion_head.0.bias']
    ego = (np.random.RandomState(B).standard_normal((B, 21)) * scale).astype(np.float32)
    tp = [T(a) for a in plan]
    ef, c1, c1p = ops.forecast_prologue(T(ego), [(tp[0], tp[1]), (tp[2], tp[3]), (tp[4], tp[5])], T(W1), T(b1))
    ef, c1, c1p = N(ef), N(c1), N(c1p)
    e64, bd = R.plan_head64(ego, *plan)
    q, q32 = R.q_of(ef, e64, bd), R.q_of(R.plan_head32(ego, *plan), e64, bd)
    c64, bdc = R.c1_64(ef, W1, b1)                                       # from the kernel's own ego_feat: local again
    qc, qc32 = R.q_of(c1, c64, bdc), R.q_of(R.c1_32(ef, W1, b1), c64, bdc)
    print('[pin] e | prologue | B %d scale %g | ego_feat q %.2f q32 %.2f | c1 q %.2f q32 %.2f' % (B, scale, q, q32, qc, qc32))
    assert ef.shape == (B, 32) and c1.shape == (B, 128) and np.isfinite(ef).all() and np.isfinite(c1).all()
    assert q <= R.bound(q32) and qc <= R.bound(qc32), (q, q32, qc, qc32)
    assert np.array_equal(c1p.view(np.int32), R.c1_to_c1p(c1).view(np.int32))


# ------------------------------------------------------------------------------------------ f. attribute MLP forms
@pytest.mark.parametrize('n_vox', [33, 210])
def test_attr_mlp_forms(n_vox):
    """three blocks with and without the density softplus (which touches channels 0 and 1 only), two blocks, and the one block of
    18 outputs the BEVStereo4DOCC predicter runs (final_softplus=False, columns 18 .. 23 exactly 0)"""
    v = (np.random.RandomState(9).standard_normal((n_vox, 32)) * 2).astype(np.float32)
    b3 = R.attr_blocks(7, [2, 17, 3])
    p3 = ops.pack_mlp_blocks(_modules(b3))
    on = _attr_case('f attr 3 blocks softplus %d' % n_vox, v, b3, True, p3)
    off = _attr_case('f attr 3 blocks plain %d' % n_vox, v, b3, False, p3)
    assert np.array_equal(on[:, 2:].view(np.int32), off[:, 2:].view(np.int32)) and (on[:, :2] > 0).all() and not np.array_equal(on[:, :2], off[:, :2])
    _attr_case('f attr 2 blocks softplus %d' % n_vox, v, b3[:2], True)
    _attr_case('f attr 1 block of 18 %d' % n_vox, v, R.attr_blocks(3, [18]), False)
