"""GPU: k_render_views<0|1|2> (preworld_amd/csrc/pw_render_views.hip) -- fp32 grid, bf16-stored grid, uint8 label grid -- through
ops.render_views / ops.render_label_views against the float64 yardstick of tests/_render_views_ref64.py: small anisotropic grids, two
channel layouts, five sample tables, partial blocks and tiles, V = 1 / 2 / 3, cameras inside, outside the unit ball and across a grid face.

Bounds are 4 x FLOORS (the error of the existing fp32 CPU checker against the same yardstick, asserted on the CPU by
test_render_views_ref64_cpu.py), never a number taken from the kernel.  Every call asserts the instantiation that ran
(pw_last_kernel).  Each comparison prints a '[parity]' line with err / bound: a record, not a threshold."""
import numpy as np
import pytest
import torch

import _render_views_ref64 as V
from preworld_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PRE = 4.0                    # allowed multiple of the CPU checker's floor
ALL = ('depth', 'cls', 'sem', 'color', 'alphainv_last', 'rgb8')
LABEL_ALL = ('depth', 'cls', 'alphainv_last', 'rgb8')
PALETTE = np.random.RandomState(3).randint(0, 256, (18, 3)).astype(np.uint8)


def T(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


def ran():
    return _lib.lib().pw_last_kernel().decode()


def render(name, grid=None, bf16=False, outputs=ALL, hw=None, origin=None, stride=None, views=None, **kw):
    """ops.render_views on a case (its packed grid unless `grid` is given), asserting the instantiation by name"""
    x, case = V.inputs(name), V.CASES[name]
    lay = case['layout']
    g = T(x['grid'] if grid is None else grid)
    if bf16:
        g = g.to(torch.bfloat16)
    K, c2w = T(x['K']), T(x['c2w'])
    if views is not None:
        K, c2w = K[views].contiguous(), c2w[views].contiguous()
    if 'rgb8' in outputs:
        kw.setdefault('palette', T(PALETTE))
    out = ops.render_views(g, K, c2w, hw or case['hw'], [float(v) for v in x['consts']], T(x['t']), stride=stride or case['stride'],
                           origin=origin or case['origin'], outputs=outputs, c_sigma=lay[1], c_sem=lay[2], n_sem=V.N_SEM, c_rgb=lay[3], **kw)
    assert ran() == 'k_render_views<%d>' % int(g.dtype == torch.bfloat16), ran()
    return out


def flat(out, k):
    a = out[k].cpu()
    return a.reshape((-1,) + tuple(a.shape[3:]))


def bits_equal(a, b):
    """bit for bit, NaN payloads included"""
    if a.dtype == torch.float32:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def check_soft(name, tag, out, ref, grid_read):
    """the kernel's outputs against the yardstick `ref` (run on `grid_read`, the values the kernel read).
    cls: the float64 argmax wherever cls_margin > 2 x (4 x floor_sem) x max |sem| off the tie pixels, elsewhere one of the top two.
    DEVIATION from "one of the top two", with its reason: where three or more classes lie within that margin of the top, fp32
    arithmetic may rank any of them first -- the fp32 CPU checker itself picks a third class on c5_96_plain, whose semantic floor is
    3e-3 -- so a class outside the top two is accepted if, and only if, its float64 sum is within the margin of the top."""
    tie, mtie = ref['tie'], ref['mask_tie']
    ok = ~tie
    got = {k: flat(out, k) for k in ALL}
    for k in V.OUTPUTS:
        assert bool(torch.isfinite(got[k]).all()), (name, tag, k)
    assert float(got['alphainv_last'].min()) >= 0 and float(got['alphainv_last'].max()) <= 1, (name, tag)
    assert float(got['depth'].min()) > 0 and float(got['depth'].max()) <= float(V.inputs(name)['consts'][26]), (name, tag)
    err = V.output_errors(got, ref)
    frac = {k: err[k] / (PRE * f) for k, f in zip(V.OUTPUTS, V.FLOORS[name])}
    print('[parity] %-20s %-5s %s  worst %.0f%%  (%d tie pixels of %d)' % (name, tag, ' '.join('%s %.2e / %.1e' % (k, err[k], PRE * f) for k, f in zip(V.OUTPUTS, V.FLOORS[name])),
                                                                           100 * max(frac.values()), int(tie.sum()), tie.numel()))
    # near-tie pixels that are no mask ties: within what samples of total weight 1.1e-3 can move (the yardstick's docstring)
    near = tie & ~mtie
    if near.any():
        for k, bound in V.near_tie_bounds(name, grid_read, ref, PRE).items():
            r = ref[V.REF_KEY[k]]
            assert float((got[k].double().reshape(r.shape)[near] - r[near]).abs().max()) <= bound, (name, tag, k, 'near-tie pixels')
    for k in V.OUTPUTS:
        assert frac[k] <= 1.0, (name, tag, k, err[k], 'bound', PRE * dict(zip(V.OUTPUTS, V.FLOORS[name]))[k])
    # the class map
    cls = got['cls'].long()
    margin_ok = ok & (ref['cls_margin'] > 2 * (PRE * V.FLOORS[name][1]) * float(ref['semantic'][ok].abs().max()))
    print('[parity] %-20s %-5s cls: %d of %d pixels decided by margin, %d differ from the float64 argmax' % (
        name, tag, int(margin_ok.sum()), cls.numel(), int((cls != ref['cls']).sum())))
    assert torch.equal(cls[margin_ok], ref['cls'][margin_ok]), (name, tag, 'cls')
    # elsewhere: one of the top two -- or, where more than two classes lie within that margin of the top (the transparent scene:
    # the floor there is 3e-3 of sums that differ by less), any of those contenders; on tie pixels the margin is the near-tie bound
    top = ref['semantic'].max(-1).values
    behind = top - ref['semantic'].gather(1, cls[:, None])[:, 0]
    slack = torch.where(tie, torch.full_like(top, 2 * V.near_tie_bounds(name, grid_read, ref, PRE)['sem']),
                        torch.full_like(top, 2 * (PRE * V.FLOORS[name][1]) * float(ref['semantic'][ok].abs().max())))
    third = (cls != ref['cls']) & (cls != ref['second'])
    assert bool((behind[third] <= slack[third]).all()), (name, tag, 'cls is neither one of the top two nor within the bound of the top', int(third.sum()))
    assert np.array_equal(got['cls'].numpy(), got['sem'].numpy().argmax(-1)), (name, tag)                       # the argmax of the kernel's own sums
    assert torch.equal(got['rgb8'], torch.from_numpy(PALETTE)[cls]), (name, tag, 'rgb8')
    return frac


@pytest.mark.parametrize('name', list(V.CASES))
def test_soft_mode_fp32_and_bf16_storage(name):
    """<0> against the yardstick; <1> against the yardstick on the bf16-rounded grid, and bit-equal to <0> on that rounded grid"""
    x = V.inputs(name)
    check_soft(name, 'fp32', render(name), V.reference(name), x['grid'])
    rounded = V.bf16_round(x['grid'])
    out16 = render(name, bf16=True)
    check_soft(name, 'bf16', out16, V.reference(name, bf16=True), rounded)
    outr = render(name, grid=rounded)
    for k in ALL:
        assert bits_equal(out16[k], outr[k]), (name, k)


@pytest.mark.parametrize('min_opacity', V.MIN_OPACITY[1])
def test_min_opacity_cuts_where_the_float64_opacity_is_below_it(min_opacity):
    """cls == 17 exactly where the float64 opacity 1 - alphainv_last < min_opacity.  Excused and counted: pixels within 4 x floor of
    the cut; near-tie pixels within 1.1e-3 + 4 x floor of it (their alphainv_last may move by a sample of that weight); mask-tie
    pixels (nothing downstream of the mask is pinned there).  At least 10 % of the pixels are decided on each side."""
    name = V.MIN_OPACITY[0]
    ref = V.reference(name)
    plain = render(name)
    cut = render(name, min_opacity=min_opacity)
    gap = (ref['opacity'] - min_opacity).abs()
    floor = PRE * V.FLOORS[name][3] * float(ref['alphainv_last'].abs().max())
    excused = (gap <= floor) | (ref['near_tie'] & (gap <= V.W_TIE + floor)) | ref['mask_tie']
    below, above = (ref['opacity'] < min_opacity) & ~excused, (ref['opacity'] >= min_opacity) & ~excused
    cls, base = flat(cut, 'cls').long(), flat(plain, 'cls').long()
    print('[parity] %-20s min_opacity %.2f: %d below, %d above, %d excused of %d pixels; %d cut' % (
        name, min_opacity, int(below.sum()), int(above.sum()), int(excused.sum()), cls.numel(), int((cls == 17).sum())))
    assert float(below.double().mean()) >= 0.10 and float(above.double().mean()) >= 0.10
    assert bool((cls[below] == 17).all()) and torch.equal(cls[above], base[above]) and int(base.max()) <= 16
    assert bool(((cls == 17) | (cls == base)).all())
    for k in V.OUTPUTS:
        assert bits_equal(cut[k], plain[k]), k                              # the cut changes the class map only
    assert torch.equal(flat(cut, 'rgb8'), torch.from_numpy(PALETTE)[cls])


@pytest.mark.parametrize('name,bf16', [('full417_mixed', False), ('three_views_stride3', True)])
def test_each_output_alone_equals_the_all_outputs_launch(name, bf16):
    """the kernel branches on null output pointers: every output requested alone is the all-outputs launch's, bit for bit"""
    full = render(name, bf16=bf16)
    for k in ALL:
        one = render(name, bf16=bf16, outputs=(k,))
        assert list(one) == [k] and bits_equal(one[k], full[k]), (name, k)


def test_label_outputs_alone_equal_the_all_outputs_launch():
    name = 'lab_mixed'
    full = render_labels(name)
    for k in LABEL_ALL:
        one = render_labels(name, outputs=(k,))
        assert list(one) == [k] and bits_equal(one[k], full[k]), k


def test_views_strides_and_windows_are_bit_exact_at_the_new_shapes():
    """V = 3 == three V = 1 launches; stride 3 == [::3, ::3] of stride 1; the (1, 1) and (8, 8) windows == crops of the (19, 37) render
    of the same rig, grid and table (fp32 and bf16 storage)"""
    name = 'three_views_stride3'
    x0, y0 = V.CASES[name]['origin']
    for bf16 in (False, True):
        three = render(name, bf16=bf16)
        dense = render(name, bf16=bf16, hw=V.HW, stride=1)
        for k in ALL:
            assert bits_equal(three[k], dense[k][:, ::3, ::3].contiguous()), (k, bf16)
        for v in range(3):
            one = render(name, bf16=bf16, views=[v])
            for k in ALL:
                assert one[k].shape[0] == 1 and bits_equal(one[k][0], three[k][v]), (k, v, bf16)
        assert not bits_equal(three['depth'][0], three['depth'][1]) and not bits_equal(three['depth'][1], three['depth'][2])
        for small in ('one_pixel', 'layout_one_wave'):
            (h, w), (sx, sy) = V.CASES[small]['hw'], V.CASES[small]['origin']
            win = render(small, bf16=bf16)
            whole = render(small, bf16=bf16, hw=V.HW, origin=V.ORIGIN)
            i0, j0 = sy - V.ORIGIN[1], sx - V.ORIGIN[0]
            for k in ALL:
                assert bits_equal(win[k], whole[k][:, i0:i0 + h, j0:j0 + w].contiguous()), (small, k, bf16)


# ------------------------------------------------------------------------------------ label mode
def render_labels(name, outputs=LABEL_ALL, layout='xyz'):
    x, case = V.inputs(name), V.LABEL_CASES[name]
    if layout == 'xyz':
        lab = T(x['labels'])                                                   # (X,Y,Z)-contiguous
    else:
        lab = T(x['labels'].transpose(2, 1, 0)).permute(2, 1, 0)               # the permuted view of a (Z,Y,X) buffer
    assert tuple(lab.shape) == case['grid'] and lab.is_contiguous() == (layout == 'xyz')
    kw = {}
    if 'rgb8' in outputs:
        kw['palette'] = T(PALETTE[:case['n_palette']])
    out = ops.render_label_views(lab, T(x['K']), T(x['c2w']), case['hw'], [float(v) for v in x['consts']], T(x['t']), empty_idx=case['empty_idx'],
                                 stride=case['stride'], origin=case['origin'], outputs=outputs, **kw)
    assert ran() == 'k_render_views<2>', ran()
    return out


@pytest.mark.parametrize('name', list(V.LABEL_CASES))
def test_label_mode(name):
    """<2> through both stride layouts (bit-equal).  Off the fragile pixels: cls and alphainv_last exactly the yardstick's, depth the fp32
    expression of the yardstick's hit at rtol 1e-6 (and within LABEL_DEPTH_ABS radius of the float64 value, whose 1 - 1 / (1 + t) does
    not cancel as the fp32 one does).  On fragile pixels: cls a label that is present or empty_idx, depth the value of some table
    entry or the miss value.  rgb8 == palette[min(cls, n_palette - 1)] everywhere."""
    x, case, ref = V.inputs(name), V.LABEL_CASES[name], V.label_reference(name)
    a, b = render_labels(name), render_labels(name, layout='zyx-view')
    for k in LABEL_ALL:
        assert bits_equal(a[k], b[k]), (name, k)
    cls, depth, last = flat(a, 'cls').long().numpy(), flat(a, 'depth').numpy(), flat(a, 'alphainv_last').numpy()
    frag = ref['fragile'].numpy()
    ok = ~frag
    radius = float(x['consts'][26])
    want_depth = V.label_depth_fp32(ref['first'].numpy(), x['t'], x['consts'])
    derr = np.abs(depth[ok].astype(np.float64) - ref['depth'].numpy()[ok]).max()
    print('[parity] %-20s label: %d pixels, %d hits, %d fragile; cls differs on %d; depth vs float64 %.2e / %.1e' % (
        name, cls.size, int((ref['first'] >= 0).sum()), int(frag.sum()), int((cls != ref['cls'].numpy()).sum()), derr, V.LABEL_DEPTH_ABS * radius))
    np.testing.assert_array_equal(cls[ok], ref['cls'].numpy()[ok])
    np.testing.assert_array_equal(last[ok], ref['alphainv_last'].numpy()[ok])
    np.testing.assert_allclose(depth[ok], want_depth[ok], rtol=1e-6)
    assert derr <= V.LABEL_DEPTH_ABS * radius
    present = np.union1d(np.unique(x['labels']), [case['empty_idx']])
    assert np.isin(cls[frag], present).all(), name
    entries = np.concatenate([V.label_depth_fp32(np.arange(len(x['t'])), x['t'], x['consts']), V.label_depth_fp32(np.array([-1]), x['t'], x['consts'])])
    nearest = np.abs(depth[frag][:, None].astype(np.float64) - entries[None].astype(np.float64)).min(1) if frag.any() else np.zeros(0)
    assert (nearest <= 1e-6 * np.abs(depth[frag])).all(), name
    assert set(np.unique(last)) <= {0.0, 1.0} and ((last == 1) == (cls == case['empty_idx'])).all()
    pal = PALETTE[:case['n_palette']]
    np.testing.assert_array_equal(flat(a, 'rgb8').numpy(), pal[np.minimum(cls, case['n_palette'] - 1)])


# ------------------------------------------------------------------------------------ non-finite attributes
@pytest.mark.parametrize('bf16', [False, True])
def test_nan_attributes_reach_exactly_the_pixels_that_read_them(bf16):
    """one NaN in a semantic channel and one in a colour channel of one voxel: the pixels the yardstick says read the voxel (a kept
    sample has it as an in-bounds corner, V.voxel_pixels `sure`) carry NaN in that channel of sem / color; every pixel that cannot
    see it (no masked sample within a cell of it) is bit-identical to the clean render in every output; depth, alphainv_last and
    the other channels are bit-identical EVERYWHERE (the density is clean); rgb8 == palette[cls] still holds everywhere.
    A NaN DENSITY is out of scope: `alpha > thres` is false for NaN, so the sample is culled, in the reference as well."""
    name, (vx, vy, vz), k_sem, k_rgb = V.NAN_PROBE
    x, case = V.inputs(name), V.CASES[name]
    _, _, c_sem, c_rgb = case['layout']
    ref = V.reference(name, bf16)
    sure, maybe = V.voxel_pixels(ref, x['t'], x['consts'], case['grid'], (vx, vy, vz))
    bad = x['grid'].copy()
    bad[vz, vy, vx, c_sem + k_sem] = np.nan
    bad[vz, vy, vx, c_rgb + k_rgb] = np.nan
    clean, got = render(name, bf16=bf16), render(name, grid=bad, bf16=bf16)
    sem, col = flat(got, 'sem'), flat(got, 'color')
    print('[parity] %-20s %-5s NaN voxel: %d pixels surely read it, %d may, %d carry NaN in sem, %d in color' % (
        name, 'bf16' if bf16 else 'fp32', int(sure.sum()), int(maybe.sum()), int(torch.isnan(sem[:, k_sem]).sum()), int(torch.isnan(col[:, k_rgb]).sum())))
    assert bool(torch.isnan(sem[sure][:, k_sem]).all()) and bool(torch.isnan(col[sure][:, k_rgb]).all())
    far = ~maybe
    for k in ALL:
        assert bits_equal(flat(got, k)[far], flat(clean, k)[far]), (k, 'a pixel that cannot see the voxel changed')
    for k in ('depth', 'alphainv_last'):
        assert bits_equal(got[k], clean[k]), k
    others_s = [c for c in range(V.N_SEM) if c != k_sem]
    others_c = [c for c in range(3) if c != k_rgb]
    assert bits_equal(sem[:, others_s].contiguous(), flat(clean, 'sem')[:, others_s].contiguous())
    assert bits_equal(col[:, others_c].contiguous(), flat(clean, 'color')[:, others_c].contiguous())
    # where the poisoned channel is not NaN it is the clean value
    fin = ~torch.isnan(sem[:, k_sem])
    assert bits_equal(sem[fin][:, k_sem].contiguous(), flat(clean, 'sem')[fin][:, k_sem].contiguous()) and not bool(torch.isnan(sem[far]).any())
    cls = flat(got, 'cls').long()
    assert int(cls.max()) <= 16
    assert torch.equal(flat(got, 'rgb8'), torch.from_numpy(PALETTE)[cls])
