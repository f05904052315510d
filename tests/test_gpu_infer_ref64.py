"""GPU: the inference convolutions on every kernel path -- k_conv3d_h2<NT, EPI, WR> (all eleven instantiations), the split-fp16
gather kernel, k_conv3d_h2_s2<1|2>, k_occ_head_h2<true|false>, k_fpn3d_fuse<true|false> and the fp32 kernels behind
PW_PRECISION=f32 -- against the float64 restatements of tests/_infer_ref64.py.

One parametrised test over _infer_ref64.ROWS.  Every row asserts the kernel that ran (pw_last_kernel), max q <= 2 * Q32[row] + 1
per element in units of u = 2^-24 n (plus the h2 storage term on h2 outputs), finite outputs, a bit-identical second call and, for
h2 outputs, the range slot's recorded maximum against this file's own decode.  Q32 comes from the float32 restatement on the CPU
(test_infer_ref64_cpu.py), never from a kernel.  h2 inputs are uploaded as bytes encoded by _infer_ref64.h2_encode and h2 outputs
are decoded by _infer_ref64.h2_decode, so the convolution is tested alone."""
import numpy as np
import pytest
import torch

import _infer_ref64 as R
from preworld_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def slot(e):
    s = torch.zeros(ops.RNG_ROW, dtype=torch.int32, device=DEV)
    s[0] = int(e)
    return s


def ran():
    return _lib.lib().pw_last_kernel().decode()


def bits(t):
    t = t.buf if isinstance(t, ops.H2) else t
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def value(y, e):
    """a kernel output as float64 numpy: h2 through this suite's own decoder, fp32 as it is"""
    if isinstance(y, ops.H2):
        return R.h2_decode(y.buf.contiguous().cpu().numpy(), e)
    return y.contiguous().cpu().numpy().astype(np.float64)


def score(name, tag, got, ref, n, h2_out):
    q = R.q_of(got, ref, n, R.storage_term(ref) if h2_out else None)
    worst, b = float(q.max()), R.bound(name)
    print('[pin] %-22s %-8s max q %8.3f  mean q %.3f  bound %.2f = 2 x %.2f + 1%s  (%.0f %% of it)' % (
        name, tag, worst, float(q.mean()), b, R.Q32[name], ' + %.1f' % R.FORMAT_TERM[name] if name in R.FORMAT_TERM else '',
        100.0 * worst / b))
    assert np.isfinite(np.asarray(got)).all(), (name, tag, 'not finite')
    return worst, b


def check_slot(name, y, e, dec):
    se, rec = ops.slot_state(y.rng)
    amax = float(np.abs(dec).max())
    assert se == e, (name, 'exponent', se, e)
    assert abs(rec - amax) <= amax * 2.0 ** -21 + amax * 2.0 ** -37, (name, 'recorded maximum', rec, amax)


# ------------------------------------------------------------------------------------------------ conv rows
def _conv_call(name, x_exp_shift=0, sliced=False):
    """run the row once on fresh destinations -> (outputs tuple, the wide NaN buffers when sliced, kernel name)"""
    r = R.ROWS[name]
    o, P, ref = R.OPSETS[r['ops']], R.operands(r['ops']), R.conv_ref(name)
    c0, c1 = R.row_split(name)
    B = o['B']
    grid = R.out_grid(o)
    wt = T(P.w)
    wides = []

    def dst(i, c):
        if sliced:
            wide = torch.full((B,) + grid + (3 * c,), float('nan'), device=DEV)
            wides.append((wide, c))
            buf = wide[..., c:2 * c]
        else:
            buf = torch.empty((B,) + grid + (c,), device=DEV)
        return ops.H2(buf, slot(ref.e[i])) if r['fmt'][i] else buf
    out0, out1 = dst(0, c0), (dst(1, c1) if c1 else None)
    res = None
    if r['res'] == 'h2':
        res = ops.H2(T(ref.resbuf), slot(ref.e[0]))
    elif r['res'] == 'f32':
        res = T(ref.res)
    kw = dict(residual=res, cout0=c0, cout1=c1, relu0=r['relu'][0], relu1=r['relu'][1], out0=out0, out1=out1)
    bias = T(ref.bias)
    if r['api'] == 'h2':
        x = ops.H2(T(P.xbuf), slot(P.ex + x_exp_shift))
        wpk, inv = ops.pack_conv_weight_h2(wt)
        y = ops.conv3d_h2(x, wpk, T(P.scale) * inv, bias, out_h2=tuple(bool(f) for f in r['fmt']), ksize=o['k'], stride=o['stride'],
                          algo=r['algo'], **kw)
    else:
        x = T(P.x)
        if x_exp_shift:
            x = x * 2.0 ** x_exp_shift
        if r['api'] == 'f32':
            y = ops.conv3d_ndhwc(x, ops.pack_conv_weight(wt), T(P.scale), bias, ksize=o['k'], stride=o['stride'], algo=r['algo'], **kw)
        else:
            y = ops.conv3d_wino(x, ops.pack_conv_weight_wino(wt), T(P.scale), bias, **kw)
    return (y if c1 else (y,)), wides, ran()


def run_conv(name):
    r = R.ROWS[name]
    ref = R.conv_ref(name)
    ys, _, kernel = _conv_call(name)
    again, _, _ = _conv_call(name)
    print('[pin] %-22s ran %s' % (name, kernel))
    assert kernel == r['kernel'], (name, kernel, r['kernel'])
    for i, (y, y2) in enumerate(zip(ys, again)):
        dec = value(y, ref.e[i])
        worst, b = score(name, 'y%d' % i, dec, ref.y[i], ref.n[i], bool(r['fmt'][i]))
        assert worst <= b, (name, i, worst, b)
        assert torch.equal(bits(y), bits(y2)), (name, i, 'a second call differs')
        if r['fmt'][i]:
            check_slot(name, y, ref.e[i], dec)
    if r['inplace']:
        # BasicBlock3D's form: the conv adds onto its residual in place, bit-equal to the out-of-place run
        P, o = R.operands(r['ops']), R.OPSETS[r['ops']]
        c0, _ = R.row_split(name)
        y0 = ops.H2(T(ref.resbuf), slot(ref.e[0]))
        wpk, inv = ops.pack_conv_weight_h2(T(P.w))
        ops.conv3d_h2(ops.H2(T(P.xbuf), slot(P.ex)), wpk, T(P.scale) * inv, T(ref.bias), residual=y0, cout0=c0, relu0=r['relu'][0],
                      out0=y0, ksize=o['k'], stride=o['stride'], algo=r['algo'])
        assert ran() == r['kernel'], (name, 'in place', ran())
        assert torch.equal(bits(y0), bits(ys[0])), (name, 'in place differs from out of place')
    if 'slice' in r['checks']:
        sl, wides, kernel = _conv_call(name, sliced=True)
        assert kernel == r['kernel'], (name, 'slice', kernel)
        for y, d, (wide, c) in zip(sl, ys, wides):
            assert torch.equal(bits(y), bits(d)), (name, 'a channel-slice destination differs from the dense one')
            fresh = torch.full_like(wide, float('nan')).view(torch.int32)
            w32 = wide.view(torch.int32)
            assert torch.equal(w32[..., :c], fresh[..., :c]) and torch.equal(w32[..., 2 * c:], fresh[..., 2 * c:]), (name, 'wrote outside')
    if 'scale' in r['checks']:
        # range exponents (and a power of two on fp32 inputs) fold in as exact powers of two: bit for bit
        assert r['zero_bias'] and r['res'] is None and r['fmt'] == (0, 0)
        for k in (20, -20):
            (yk,), _, kernel = _conv_call(name, x_exp_shift=k)
            assert kernel == r['kernel'], (name, 'scale', kernel)
            assert torch.equal(yk, ys[0] * 2.0 ** k), (name, 'conv(2^%d x) != 2^%d conv(x)' % (k, k))


# ------------------------------------------------------------------------------------------------ OccHead rows
def _occ_args(P):
    w0, s0, b0, w1, s1, b1, w2 = [T(a) for a in (P.w0, P.s0, P.b0, P.w1, P.s1, P.b1, P.w2)]
    return w0, s0, b0, w1, s1, b1, w2


def run_occ(name):
    r = R.ROWS[name]
    B, D, H, W = r['shape']
    P = R.occ_operands(r['shape'], r['regime'])
    ref, _ = R.occ_ref(r['shape'], r['regime'])
    w0, s0, b0, w1, s1, b1, w2 = _occ_args(P)
    if r['api'] == 'h2':
        wpk, inv = ops.pack_occ_weight_h2(w0)
        hargs = ((s0 * inv).contiguous(), b0) + ops.pack_occ_tail_h2(w1, s1, b1, w2) + (ops.occ_head_bounds(w0, s0, b0, w1, s1, b1),)
        xh = ops.H2(T(P.xbuf), slot(P.ex))
        full = lambda: ops.occ_head_h2(xh, wpk, *hargs, want_logits=True, want_geo=True)
    else:
        pk = ops.pack_conv_weight16(w0) if r['api'] == 'f32' else ops.pack_conv_weight_wino(w0, cout_total=16)
        full = lambda: ops.occ_head_fused(T(P.x), pk, ops._pad32(s0, 1.0), ops._pad32(b0, 0.0), w1, s1, b1, w2, want_logits=True,
                                          want_geo=True)
    occ, lg, geo = full()
    kernel = ran()
    occ2, lg2, geo2 = full()
    if r['strided']:
        # the (D, H, W) result written as the transposed (W, H, D) array into rows of a gapped buffer, without logits
        buf = torch.full((B, 2, W, H, D + 3), 255, dtype=torch.uint8, device=DEV)
        o_s, g_s = ops.occ_head_h2(xh, wpk, *hargs, occ=buf[..., :D][:, 0].permute(0, 3, 2, 1), geo=buf[..., :D][:, 1].permute(0, 3, 2, 1))
        kernel = ran()
        assert torch.equal(o_s, occ) and torch.equal(g_s, geo), (name, 'strided destinations differ from the contiguous run')
        assert bool((buf[..., D:] == 255).all()), (name, 'wrote into the gaps')
    print('[pin] %-22s ran %s' % (name, kernel))
    assert kernel == r['kernel'], (name, kernel, r['kernel'])
    assert torch.equal(occ, occ2) and torch.equal(bits(lg), bits(lg2)) and torch.equal(geo, geo2), (name, 'a second call differs')
    lgn, occn = lg.cpu().numpy().astype(np.float64), occ.cpu().numpy()
    worst, b = score(name, 'logits', lgn, ref.logits, ref.n, False)
    assert worst <= b, (name, worst, b)
    assert np.array_equal(occn, np.argmax(lg.cpu().numpy(), -1)), (name, 'occ is not the first maximum of the kernel logits')
    tie = R.near_tie(ref, b).numpy()
    flips = occn != ref.occ
    print('[pin] %-22s occ: %d of %d voxels differ from the float64 argmax, %d near-ties (%.2f %%), %d entirely clamped' % (
        name, int(flips.sum()), flips.size, int(tie.sum()), 100.0 * tie.mean(), int(ref.dead.sum())))
    assert not (flips & ~tie).any(), (name, 'occ differs from the float64 argmax away from a near-tie')
    dead = ref.dead.numpy() & (lgn == 0).all(-1)
    assert dead.any() and (occn[dead] == 0).all(), (name, 'an entirely clamped voxel must give 18 zero logits and class 0')
    assert np.array_equal(geo.cpu().numpy(), np.where(occn != 17, 0, 17).astype(np.uint8)), (name, 'geo')


# ------------------------------------------------------------------------------------------------ neck rows
def run_fpn(name):
    r = R.ROWS[name]
    ref = R.fpn_ref(name)
    w8 = T(ref.w8)

    def call():
        if r['h2']:
            wpk, inv = ops.pack_conv_weight_h2(w8)
            out = ops.H2(torch.empty(ref.x.shape, device=DEV), slot(ref.e))
            # the three partial sums share ONE epilogue scale, scale * inv: the coarse levels come pre-divided by inv (LSSFPN3D.operands
            # folds that power of two into the laterals' scale)
            return ops.fpn3d_fuse(ops.H2(T(ref.xbuf), slot(ref.ex)), wpk, T(ref.y16) / inv, T(ref.y32) / inv, T(ref.scale) * inv,
                                  T(ref.bias), relu=True, out=out, out_h2=True)
        return ops.fpn3d_fuse(T(ref.x), ops.pack_conv_weight(w8), T(ref.y16), T(ref.y32), T(ref.scale), T(ref.bias), relu=True)
    y = call()
    kernel = ran()
    y2 = call()
    print('[pin] %-22s ran %s' % (name, kernel))
    assert kernel == r['kernel'], (name, kernel, r['kernel'])
    dec = value(y, ref.e)
    worst, b = score(name, 'y', dec, ref.y, ref.n, r['h2'])
    assert worst <= b, (name, worst, b)
    assert torch.equal(bits(y), bits(y2)), (name, 'a second call differs')
    if r['h2']:
        check_slot(name, y, ref.e, dec)


@pytest.mark.parametrize('name', list(R.ROWS))
def test_infer_row(name):
    cus = ops.device_info()['cu_count']
    assert cus == R.CUS, 'the case table is laid out for %d CUs (nt2_batch, the MT and NG thresholds); this device has %d' % (R.CUS, cus)
    with torch.no_grad():
        {'conv': run_conv, 'occ': run_occ, 'fpn': run_fpn}[R.ROWS[name]['kind']](name)
