"""tests/_infer_ref64.py must be trusted before it judges a kernel.  Here: the float64 restatements against the float32 oracle,
torch's own float64 ops and the reference model's stored logits; the h2 decoder on a hand-built chunk and on split -> decode
round trips; every input condition a GPU row relies on (ragged grids, ReLU clamp shares, entirely clamped OccHead voxels, the
near-tie cap) proven on the reference alone; the float32 floor table Q32 each GPU bound is built from; and the dispatch thresholds
restated as functions of the CU count, with each row's expected kernel derived from them.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref64 as C64
import _infer_ref64 as R
from oracle import oracle as O
from preworld_amd import ops
from preworld_amd import synth as S

CONV_ROWS = [n for n in R.ROWS if R.ROWS[n]['kind'] == 'conv']
OCC_ROWS = [n for n in R.ROWS if R.ROWS[n]['kind'] == 'occ']
FPN_ROWS = [n for n in R.ROWS if R.ROWS[n]['kind'] == 'fpn']


def _ncdhw(a):
    return np.ascontiguousarray(np.asarray(a).transpose(0, 4, 1, 2, 3))


# ------------------------------------------------------------------------------------------------ 1. the reference is pinned
@pytest.mark.parametrize('stride', [1, 2])
def test_conv_bn_act_vs_oracle_and_torch(stride):
    """conv_bn_act against torch's float64 conv to float64 rounding, and against the float32 oracle in units of u: the oracle adds
    its 27 x 32 products one after the other in float32, whose worst case is K u; sqrt(K) = 30 is asserted (measured: below 8)."""
    rs = np.random.RandomState(3)
    x = rs.standard_normal((2, 5, 7, 9, 32)).astype(np.float32)
    w = (rs.standard_normal((48, 32, 3, 3, 3)) * 0.05).astype(np.float32)
    scale = np.exp2(rs.randint(-10, 3, 48)).astype(np.float32)
    bias = (scale * rs.standard_normal(48)).astype(np.float32)
    grid = tuple(C64.out_extent(v, 3, stride) for v in (5, 7, 9))
    res = (scale * rs.standard_normal((2,) + grid + (48,))).astype(np.float32)
    y, n = R.conv_bn_act(x, w, scale, bias, res, relu=True, stride=stride)
    t = torch.from_numpy
    want = F.conv3d(t(_ncdhw(x)).double(), t(w).double(), stride=stride, padding=1).permute(0, 2, 3, 4, 1)
    want = torch.relu(want * t(scale).double() + t(bias).double() + t(res).double())
    assert float(((y - want).abs() / n).max()) < 1e-13
    o = O.conv3d(_ncdhw(x), w, None, stride, 1) * scale[None, :, None, None, None] + bias[None, :, None, None, None]
    o = np.maximum(o + _ncdhw(res), 0).transpose(0, 2, 3, 4, 1)
    q = float(R.q_of(o, y, n).max())
    print('[pin] conv_bn_act stride %d vs float32 oracle: max q %.2f' % (stride, q))
    assert q < 30.0
    assert 0.25 < float((y == 0).double().mean()) < 0.75 and float(n.min()) > 0


def _occ_oracle(P):
    mid = np.maximum(O.conv3d(_ncdhw(P.x), P.w0) * P.s0[None, :, None, None, None] + P.b0[None, :, None, None, None], 0)
    hid = np.maximum(np.einsum('oc,bcdhw->bodhw', P.w1, mid) * P.s1[None, :, None, None, None] + P.b1[None, :, None, None, None], 0)
    return np.einsum('oc,bcdhw->bdhwo', P.w2, hid)


def test_occ_head_vs_oracle_restatement():
    """the OccHead restatement against the float32 oracle composition test_occ_head_* use, in units of the propagated n"""
    P = R.occ_operands((3, 2, 9, 7), 'normal')
    ref, r32 = R.occ_ref((3, 2, 9, 7), 'normal')
    q = float(R.q_of(_occ_oracle(P), ref.logits, ref.n).max())
    print('[pin] occ_head vs float32 oracle: max q %.2f' % q)
    assert q < 30.0
    assert np.array_equal(ref.geo, np.where(ref.occ != 17, 0, 17)) and float(ref.margin.min()) >= 0.0
    assert np.array_equal(ref.occ, ref.logits.argmax(-1).numpy())              # torch documents the first maximum as well


def test_occ_head_vs_reference_fixture(golden):
    """tests/golden/conv_stack_small.npz: the reference OccHead's own float32 logits of its stored final_conv output (fed as
    (1, C, X, Y, Z)), to the tolerance test_conv_stack_golden holds the kernels to"""
    g = golden('conv_stack_small.npz')
    sd = S.synth_state_dict(int(g['seed_sd']))
    p = 'occupancy_head.'
    fold = lambda k: [a.numpy() for a in ops.fold_bn(*[torch.from_numpy(sd[p + k + s]) for s in ('.weight', '.bias', '.running_mean', '.running_var')])]
    (s0, b0), (s1, b1) = fold('occ_convs.0.1'), fold('occ_pred_conv.1')
    x = g['final_conv'].transpose(0, 4, 3, 2, 1)                                # (1, C, Z, Y, X) -> (1, X, Y, Z, C)
    ref = R.occ_head(x, sd[p + 'occ_convs.0.0.weight'], s0, b0, sd[p + 'occ_pred_conv.0.weight'].reshape(8, 16), s1, b1,
                     sd[p + 'occ_pred_conv.3.weight'].reshape(18, 8))
    np.testing.assert_allclose(ref.logits.numpy(), g['logits'].transpose(0, 2, 3, 4, 1), rtol=5e-4, atol=5e-4)
    assert (ref.occ[0] != g['occ']).mean() < 1e-3


@pytest.mark.parametrize('shape,lv16,lv32', [((2, 5, 19, 27), (3, 10, 14), (2, 5, 7)), ((1, 4, 8, 24), (2, 4, 12), (1, 2, 6)),
                                             ((1, 1, 3, 2), (1, 2, 1), (1, 1, 1))])
def test_neck_vs_torch_interpolate(shape, lv16, lv32):
    """the neck restatement (its own align_corners=True interpolation, float64 laterals) against F.interpolate in float64"""
    rs = np.random.RandomState(5)
    B, D, H, W = shape
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))
    x8, x16, x32 = t(B, D, H, W, 32), t(B, *lv16, 64), t(B, *lv32, 128)
    w8, w16, w32, sc, bi = t(32, 32), t(32, 64), t(32, 128), t(32), t(32)
    y, n = R.neck(x8, w8, x16, x32, sc, bi, w16=w16, w32=w32)
    up = lambda v: F.interpolate(v.permute(0, 4, 1, 2, 3), size=(D, H, W), mode='trilinear', align_corners=True).permute(0, 2, 3, 4, 1)
    want = torch.relu((x8 @ w8.t() + up(x16 @ w16.t()) + up(x32 @ w32.t())) * sc + bi)
    assert float(((y - want).abs() / n).max()) < 1e-13
    y2, n2 = R.neck(x8, w8, x16 @ w16.t(), x32 @ w32.t(), sc, bi)              # the form the fused kernel is given
    assert float(((y2 - want).abs() / n2).max()) < 1e-13 and bool((n2 <= n * (1 + 1e-12)).all())


# ------------------------------------------------------------------------------------------------ 2. the decoder is pinned
def test_h2_decode_hand_built_chunk():
    """one 128-byte chunk written slot by slot as pw_h2.h documents it: slot(half, ks, p) = 4 half + 2 ks + p holds plane p of
    channels 16 ks + 8 half + 0 .. 7; value = (hi + lo) * 2^e"""
    chunk = np.zeros(64, np.float16)
    want = np.zeros(32)
    for half in range(2):
        for ks in range(2):
            for j in range(8):
                c = 16 * ks + 8 * half + j
                hi, lo = np.float16(c + 1), np.float16(-(c + 1) * 2.0 ** -12)
                chunk[(4 * half + 2 * ks + 0) * 8 + j] = hi
                chunk[(4 * half + 2 * ks + 1) * 8 + j] = lo
                want[c] = (float(hi) + float(lo)) * 2.0 ** -3
    got = R.h2_decode(chunk.view(np.float32).reshape(1, 32), -3)
    assert np.array_equal(got[0], want)
    # the header's byte formula h2_group_off(c, p) = (4 ((c >> 3) & 1) + 2 (c >> 4) + p) * 16 + 2 (c & 7), in fp16 units
    for p, idx in ((0, R.HI_IDX), (1, R.LO_IDX)):
        assert [int(i) for i in idx] == [((4 * ((c >> 3) & 1) + 2 * (c >> 4) + p) * 16 + 2 * (c & 7)) // 2 for c in range(32)]
    assert sorted(list(R.HI_IDX) + list(R.LO_IDX)) == list(range(64))


def test_h2_split_decode_round_trip():
    """x -> split -> decode over 2^-20 .. 2^15: within the storage term 2^-21 |x| + 2^-37 amax; the quantised operands reproduce
    themselves exactly, and so do quantised weights through the library's own host-side packer"""
    rs = np.random.RandomState(7)
    x = (np.exp2(rs.uniform(-20, 15, (3, 5, 64))) * rs.choice([-1.0, 1.0], (3, 5, 64))).astype(np.float32)
    x[0, 0, :3] = [2.0 ** 15, 0.0, -2.0 ** -20]
    e = R.ideal_exp(float(np.abs(x).max()))
    assert e == 15 - 12 == ops.RangeCtx.ideal_exp(float(np.abs(x).max()))
    back = R.h2_decode(R.h2_encode(x, e), e)
    err = np.abs(back - x.astype(np.float64))
    assert (err <= np.abs(x) * 2.0 ** -21 + float(np.abs(x).max()) * 2.0 ** -37).all()
    xq, buf, e2 = R.quant_x(x)
    assert e2 == e and np.array_equal(R.quant_x(xq)[0], xq) and np.array_equal(R.h2_decode(buf, e), xq.astype(np.float64))
    w = R.quant_w(rs.standard_normal((32, 32, 3, 3, 3)) * 0.05)
    assert np.array_equal(R.quant_w(w), w)
    # ops.pack_conv_weight_h2 is plain torch: its planes of a quantised weight add up to the weight exactly
    wpk, inv = ops.pack_conv_weight_h2(torch.from_numpy(w))
    planes = wpk.view(torch.float16).view(1, 27, 1, 2, 2, 2, 32, 8).double()      # (ch, tap, nt, ks, p, h, j, e)
    back = (planes[:, :, :, :, 0] + planes[:, :, :, :, 1]).permute(0, 2, 5, 3, 4, 6, 1)[0, 0]   # (j, ks, h, e, tap)
    back = back.reshape(32, 32, 27) * inv.double()[:, None, None]
    assert torch.equal(back, torch.from_numpy(w).double().reshape(32, 32, 27))


# ------------------------------------------------------------------------------------------------ 3. each row is what it claims
def _expected_kernel(name, cus=R.CUS):
    """the dispatch rules of pw_conv3d_h2 / pw_conv3d_ndhwc / pw_conv3d_wino restated (case selection only: the GPU test asserts
    the kernel that actually ran)"""
    r = R.ROWS[name]
    o = R.OPSETS[r['ops']]
    c0, c1 = R.row_split(name)
    Do, Ho, Wo = R.out_grid(o)
    ntiles, n_out = o['cout'] // 32, o['B'] * Do * Ho * Wo
    nblk = R.n_tiles(o['B'], Do, Ho, Wo)
    fm0, fm1 = r['fmt']
    h2epi = fm0 == 1 and (c1 == 0 or fm1 == 1) and r['res'] is None
    if r['api'] == 'wino':
        return 'k_conv3d_wino_ws<%d>' % R.wino_ng(nblk, o['cout'], cus)
    if r['api'] == 'f32':
        nt = 2 if ntiles % 2 == 0 else 1
        if o['k'] == 3 and o['stride'] == 1 and r['algo'] != 2 and nt == 2:
            nt = R.f32_nt(nblk, ntiles)
        if o['k'] == 3 and o['stride'] == 1 and r['algo'] in (1, 4):
            return 'k_conv3d_k3s1_pipe<%d>' % nt if r['algo'] == 4 else 'k_conv3d_k3s1<%d, 1>' % nt
        assert o['k'] == 2, 'only the 2x2x2 stride-2 gather is a row of the fp32 gather kernel'
        return 'k_conv3d_gather<%d, %d, %d, 1, 1>' % (nt, o['k'], o['stride'])
    if o['k'] == 3 and o['stride'] == 1 and r['algo'] not in (2, 3):
        nt = R.h2_nt(nblk, ntiles, cus)
        epi = 1 if h2epi else 2 if (fm0 == 1 and c1 == 0 and r['res'] == 'h2') else 3 if (fm0 == 0 and (c1 == 0 or fm1 == 0) and r['res'] is None) else 0
        wr = nt == 1 and ntiles == 1 and o['cin'] == 32 and epi > 0
        return R.H2 % (1 if wr else nt, epi, 'true' if wr else 'false')
    if o['k'] == 3 and o['stride'] == 2 and r['algo'] == 0 and h2epi and ntiles in (4, 8):
        return 'k_conv3d_h2_s2<%d>' % (ntiles // 4)
    nt = 2 if ntiles % 2 == 0 else 1
    mt = R.gather_mt(n_out, ntiles // nt) if (o['k'], o['stride']) == (3, 2) else 1
    nch = o['cin'] // 32
    ks = (4 if nch % 4 == 0 else 2 if nch % 2 == 0 else 1) if r['algo'] == 3 and mt == 1 else 1
    return R.GA % (nt, o['k'], o['stride'], mt, ks, 'true' if h2epi else 'false')


def test_thresholds_at_256_cus():
    assert R.nt2_batch(256) == 2 and R.OPSETS['A']['B'] == 2 and R.n_tiles(1, *R.G_BIG) == 64
    assert R.h2_nt(128, 8, 256) == 2 and R.h2_nt(127, 8, 256) == 1 and R.h2_nt(60, 4, 256) == 1 and R.h2_nt(1 << 12, 3, 256) == 1
    assert R.h2_nt(128, 8, 304) == 1 and R.nt2_batch(304) == 3                  # a larger part needs a third sample
    assert R.gather_mt(22960, 3) == 1 and R.gather_mt(170 * 128, 3) == 2 and R.gather_mt(336, 1) == 2
    assert R.f32_nt(128, 8) == 2 and R.f32_nt(127, 8) == 1 and R.wino_ng(128, 256, 256) == 2 and R.wino_ng(64, 32, 256) == 1


@pytest.mark.parametrize('name', CONV_ROWS)
def test_conv_row_is_what_it_claims(name):
    r = R.ROWS[name]
    o = R.OPSETS[r['ops']]
    assert _expected_kernel(name) == r['kernel'], (name, _expected_kernel(name), r['kernel'])
    Do, Ho, Wo = R.out_grid(o)
    if 'gather' in r['kernel']:
        assert (o['B'] * Do * Ho * Wo) % 128, (name, 'the last block of 128 output voxels must be partial')
    else:
        tile = R.S2_TILE if '_s2' in r['kernel'] else (R.BD, R.BH, R.BW)
        assert Do % tile[0] and Ho % tile[1] and Wo % tile[2], (name, 'tiles must be cut in every axis', (Do, Ho, Wo), tile)
    if o['stride'] == 2:
        assert o['k'] == 2 or (o['D'] % 2 and o['H'] % 2 and o['W'] % 2), (name, 'odd input extents in every axis')
    ref = R.conv_ref(name)
    for i, y in enumerate(ref.y):
        assert float(ref.n[i].min()) > 0.0 and bool(torch.isfinite(y).all())
        if r['relu'][i]:
            share = float((y == 0).double().mean())
            assert 0.25 <= share <= 0.75, (name, i, 'ReLU clamps %.3f of the outputs' % share)
        if r['fmt'][i]:
            assert ref.e[i] == R.ideal_exp(float(y.abs().max()))
    if r['res'] == 'h2':                # the residual is stored under y0's exponent, inside fp16's range
        assert float(np.abs(ref.res).max()) * 2.0 ** -ref.e[0] < 65504.0
        assert np.array_equal(R.h2_decode(ref.resbuf, ref.e[0]), ref.res.astype(np.float64))
    if o['regime'] == 'wide':           # the regime the per-tensor metric is blind to: n spans orders of magnitude inside one tensor
        assert float(ref.n[0].max() / ref.n[0].min()) > 1e3


def test_conv_rows_cover_every_instantiation_and_regime():
    kernels = set(R.ROWS[n]['kernel'] for n in R.ROWS)
    for nt in (1, 2):
        for epi in range(4):
            assert R.H2 % (nt, epi, 'false') in kernels
    for epi in (1, 2, 3):
        assert R.H2 % (1, epi, 'true') in kernels
    for k in ('k_conv3d_h2_s2<1>', 'k_conv3d_h2_s2<2>', 'k_occ_head_h2<true>', 'k_occ_head_h2<false>', 'k_fpn3d_fuse<true>',
              'k_fpn3d_fuse<false>', 'k_conv3d_k3s1_pipe<1>', 'k_conv3d_k3s1_pipe<2>', 'k_conv3d_k3s1<1, 1>', 'k_conv3d_k3s1<2, 1>',
              'k_conv3d_wino_ws<1>', 'k_conv3d_wino_ws<2>', 'k_occ_head_wino', 'k_occ_head16<1>', 'k_conv3d_gather<2, 2, 2, 1, 1>'):
        assert k in kernels, k
    regimes = {}
    for n, r in R.ROWS.items():
        regimes.setdefault(r['family'], set()).add(R.OPSETS[r['ops']]['regime'] if r['kind'] == 'conv' else r['regime'])
    for fam, have in regimes.items():
        assert have == {'normal', 'relu', 'wide'}, (fam, have)
    # sample boundaries: a row of each NT with B >= 2, and the resident kernel's one- and two-trip loops
    assert R.OPSETS['A']['B'] >= 2 and R.OPSETS['B']['B'] >= 2
    items = lambda s: R.n_tiles(R.OPSETS[s]['B'], *R.out_grid(R.OPSETS[s]))
    assert items('C') < 256 < items('D') < 512 and items('D') % 256


@pytest.mark.parametrize('name', OCC_ROWS)
def test_occ_row_is_what_it_claims(name):
    r = R.ROWS[name]
    ref, _ = R.occ_ref(r['shape'], r['regime'])
    B, D, H, W = r['shape']
    if r['shape'] != (1, 4, 8, 8):                                      # (the one whole tile of the three shapes)
        assert D % R.BD and H % R.BH and W % R.BW
    dead = ref.dead.numpy()
    assert dead.any(), (name, 'no voxel whose hidden layer is entirely clamped')
    assert bool((ref.logits[ref.dead] == 0).all()) and (ref.occ[dead] == 0).all()
    share = float(R.near_tie(ref, R.bound(name)).double().mean())
    print('[pin] %-22s entirely clamped %d of %d voxels (%.2f %%); near-ties at the asserted bound %.2f: %.2f %%' % (
        name, int(dead.sum()), dead.size, 100.0 * dead.mean(), R.bound(name), 100.0 * share))
    assert share <= 0.02, (name, share)
    assert len(set(ref.occ.reshape(-1).tolist())) >= 5


@pytest.mark.parametrize('name', FPN_ROWS)
def test_fpn_row_is_what_it_claims(name):
    r = R.ROWS[name]
    ref = R.fpn_ref(name)
    B, D, H, W = r['shape']
    assert (W >= 32) == (r['kernel'] == 'k_fpn3d_fuse<true>') and (B * D * H * W) % 128
    if 'odd' in name:
        assert any(2 * a != b for a, b in zip(r['lv16'], (D, H, W))) and any(4 * a != b for a, b in zip(r['lv32'], (D, H, W)))
        assert r['lv16'] == tuple((v + 1) // 2 for v in (D, H, W)) and r['lv32'] == tuple((v + 1) // 2 for v in r['lv16'])
    assert 0.25 <= float((ref.y == 0).double().mean()) <= 0.75 and float(ref.n.min()) > 0.0


# ------------------------------------------------------------------------------------------------ 4. the float32 floor table
@pytest.mark.parametrize('name', list(R.ROWS))
def test_q32_floor(name):
    """Q32 holds max q of the float32 restatement, rounded up; the restatement must stay under it and not far under"""
    worst, mean = R.q32(name)
    print('[pin] %-22s %-46s q32 max %.3f  mean %.3f  (table %.2f, GPU bound %.2f)' % (
        name, R.ROWS[name]['kernel'], worst, mean, R.Q32[name], R.bound(name)))
    assert worst <= R.Q32[name], (name, worst, R.Q32[name])
    assert worst >= 0.5 * R.Q32[name], (name, 'the table entry is not this measurement', worst, R.Q32[name])
