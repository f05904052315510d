"""CPU half of the float64 pin of the dense view renderer (tests/_render_views_ref64.py): the yardstick reproduces the fixture recorded
from the reference's own get_rays + NerfHead, its pixel rays are the fp32 restatement's to fp32 rounding, every case is in the regime
it claims and under its caps from the yardstick alone, the existing fp32 CPU checker agrees with it in masks off the tie pixels,
every entry of FLOORS is that checker's error (asserted from both sides), and label_views64 agrees with the fp32 restatement
(tests/_render_views_np.label_views) off the fragile pixels of both.  No GPU."""
import numpy as np
import pytest
import torch

import _render_views_np as RV
import _render_views_ref64 as V
from preworld_amd import synth as S


def test_cases_hygiene():
    assert set(V.FLOORS) == set(V.CASES) and all(len(f) == len(V.OUTPUTS) for f in V.FLOORS.values())
    tables = {c['table'] for c in V.CASES.values()}
    assert {('sub', 2), ('c5', 96), ('dense', 128), ('full', 417), ('ext', 448)} <= tables
    shapes = {(c['hw'], c['origin'], c['stride']) for c in V.CASES.values()}
    assert ((19, 37), (3, 2), 1) in shapes and {(1, 1), (8, 8), (17, 16)} <= {s[0] for s in shapes}
    assert any(s[2] == 3 and s[1] != (0, 0) for s in shapes)
    assert {c['grid'] for c in V.CASES.values()} == {(11, 7, 5), (3, 2, 2)}
    assert any(c['layout'] == (32, 5, 8, 27) for c in V.CASES.values())
    assert {c['scene'] for c in V.CASES.values()} == {'mixed', 'plain', 'clear'}
    views = set()
    for name in list(V.CASES) + list(V.LABEL_CASES):
        x, case = V.inputs(name), V._case(name)
        K, c2w = x['K'], x['c2w']
        views.add(len(K))
        assert K.dtype == np.float32 and c2w.dtype == np.float32 and K.shape[1:] == (3, 3) and c2w.shape == (len(K), 4, 4)
        for a in range(len(K)):
            for b in range(a + 1, len(K)):
                assert not np.array_equal(c2w[a], c2w[b]), name
        assert (V.face_window(x['consts'], case['grid']) <= V.FACE_CAP).all(), name
        t = x['t']
        assert t.dtype == np.float32 and 2 <= len(t) <= 448 and (np.diff(t) > 0).all()
        if 'grid' in x:
            X, Y_, Z = case['grid']
            assert x['grid'].shape == (Z, Y_, X, case['layout'][0])
    assert views == {1, 2, 3}
    K, c2w = V.rig('three')
    assert len({tuple(k.reshape(-1)) for k in K}) == 3                        # three different K: a wrong v * 9 shows
    # the (1, 1) and (8, 8) windows lie inside the (19, 37) window of their rig
    for name in ('one_pixel', 'layout_one_wave'):
        (h, w), (x0, y0) = V.CASES[name]['hw'], V.CASES[name]['origin']
        assert V.ORIGIN[0] <= x0 and x0 + w <= V.ORIGIN[0] + V.HW[1] and V.ORIGIN[1] <= y0 and y0 + h <= V.ORIGIN[1] + V.HW[0]
    lab = {n: V.inputs(n)['labels'] for n in V.LABEL_CASES}
    assert V.LABEL_CASES['lab_empty0']['empty_idx'] == 0 and int(lab['lab_255'].max()) == 255 and V.LABEL_CASES['lab_255']['n_palette'] == 5
    for n, a in lab.items():
        assert a.dtype == np.uint8 and a.shape == V.LABEL_CASES[n]['grid']


@pytest.mark.parametrize('rig', ['pair', 'one', 'three', 'outside', 'face'])
def test_pixel_rays64_against_the_fp32_restatement(rig):
    """origins equal; a direction component is a sum of three products of magnitude <= |rd| built from two divisions: within
    8 x 2^-24 |rd| of the float64 value (five roundings, doubled)"""
    K, c2w = V.rig(rig, (8.0, 10.0, 9.0))
    for hw, stride, origin in ((V.HW, 1, V.ORIGIN), ((7, 13), 3, (3, 2)), ((1, 1), 1, (23, 11))):
        ro, rd = V.pixel_rays64(K, c2w, hw, stride, origin)
        rows = RV.pixel_rays(K, c2w, hw, stride, origin).reshape(-1, 9).astype(np.float64)
        np.testing.assert_array_equal(ro.numpy(), rows[:, 0:3])
        nrm = np.linalg.norm(rows[:, 3:6], axis=1, keepdims=True)
        assert (np.abs(rd.numpy() - rows[:, 3:6]) <= 8 * 2.0 ** -24 * nrm).all()


def test_pixel_rays64_against_the_reference_rows(golden):
    """the rows the reference's own get_rays produced (tests/golden/render_views_small.npz)"""
    g = golden('render_views_small.npz')
    hw, origin = tuple(int(v) for v in g['hw']), tuple(int(v) for v in g['origin'])
    for K, c2w, rows in ((g['K'], g['c2w'], g['rays']), (g['clear_K'], g['clear_c2w'], g['clear_rays'])):
        ro, rd = V.pixel_rays64(K, c2w, hw, 1, origin)
        rows = rows.reshape(-1, 9).astype(np.float64)
        np.testing.assert_array_equal(ro.numpy(), rows[:, 0:3])
        nrm = np.linalg.norm(rows[:, 3:6], axis=1, keepdims=True)
        assert (np.abs(rd.numpy() - rows[:, 3:6]) <= 8 * 2.0 ** -24 * nrm).all()
        np.testing.assert_allclose((rd / rd.norm(dim=1, keepdim=True)).numpy(), rows[:, 6:9], rtol=0, atol=8 * 2.0 ** -24)


@pytest.mark.parametrize('tag', ['soft', 'mixed', 'clear'])
def test_views64_reproduces_the_reference_fixture(golden, tag):
    """views64 on the fixture's scenes (200 x 200 x 16, the reference's get_rays rows and render outputs) at the bounds
    test_gpu_render_views.py::test_views_against_reference_fixture uses, on non-tie pixels.  `soft` is nearly empty (alpha = 5e-7 per
    sample): there the fp32 rounding of the reference's own alpha formula is 1e-2 of every output, so alpha's VALUES are rounded as
    the reference rounds them (fp32_alpha, _render_ref64.render64's docstring)."""
    g = golden('render_views_small.npz')
    hw, origin = tuple(int(v) for v in g['hw']), tuple(int(v) for v in g['origin'])
    grids = {'soft': S.render_grids, 'mixed': S.render_grids_mixed, 'clear': RV.clear_scene}[tag](int(g[tag + '_seed']))
    K, c2w = (g['clear_K'], g['clear_c2w']) if tag == 'clear' else (g['K'], g['c2w'])
    grid = V.pack(*grids, V.DEFAULT_LAYOUT)
    ref = V.views64(K, c2w, hw, 1, origin, V.Y.full_table(), grid, V.standard_constants(g['bda']), fp32_alpha=(tag == 'soft'))
    ok = ~ref['tie'].numpy()
    print('[parity] views64 vs render_views_small/%s: %d tie pixels of %d' % (tag, int((~ok).sum()), ok.size))
    assert (~ok).mean() <= V.TIE_CAP
    for key, name, rtol, atol in (('depth', 'depth', 1e-3, 1e-4), ('semantic', 'semantic', 1e-3, 1e-3), ('color', 'color', 1e-3, 1e-3),
                                  ('alphainv_last', 'alphainv_last', 1e-3, 1e-5)):
        want = g['%s_%s' % (tag, name)].reshape((ok.size,) + g['%s_%s' % (tag, name)].shape[3:])
        np.testing.assert_allclose(ref[key].numpy()[ok], want[ok], rtol=rtol, atol=atol, err_msg='%s %s' % (tag, key))
    if tag == 'clear':
        sem = g['clear_semantic'].reshape(-1, 17)
        clear = ok & (g['clear_margin'].reshape(-1) > 2 * (1e-3 * np.abs(sem).max(-1) + 1e-3))
        assert clear.mean() > 0.8
        np.testing.assert_array_equal(ref['cls'].numpy()[clear], sem.argmax(-1)[clear])


def check_regime(name, ref):
    case = V.CASES[name]
    R, S_ = ref['mask'].shape
    V_ = len(V.inputs(name)['K'])
    assert R == V_ * case['hw'][0] * case['hw'][1]
    assert int(ref['tie'].sum()) <= int(V.TIE_CAP * R), (name, int(ref['near_tie'].sum()), int(ref['mask_tie'].sum()))
    if case['scene'] == 'mixed' and S_ >= 96:
        assert float((ref['alphainv_last'] < V.Y.T_STOP).double().mean()) >= 0.10, name
    if case['scene'] == 'plain':
        assert float(ref['alphainv_last'].min()) > 0.9, name
    if case['rig'] == 'outside':                                  # view 0: every sample of every pixel is contracted
        inner = ref['inner'].reshape(V_, -1)
        assert not bool(inner[0].any()) and bool(inner[1].any())
        assert int(ref['kept'].reshape(V_, -1)[0].sum()) > 0
    if case['rig'] == 'face':
        n = ref['n_inb'][ref['kept']]
        # (an axis-aligned grid leaves 1, 2, 4 or 8 corners in bounds: beyond a corner, an edge, a face, or inside)
        assert all(int((n == k).sum()) > 0 for k in (0, 4, 8)) and int(((n >= 1) & (n <= 7)).sum()) > 100, (name, torch.bincount(n, minlength=9).tolist())
    if case['scene'] == 'clear':
        ok = ~ref['tie']
        assert len(torch.unique(ref['cls'][ok])) >= 10, name
        small = ref['cls_margin'] <= 2 * (4 * V.FLOORS[name][1]) * float(ref['semantic'][ok].abs().max())
        assert float((small | ref['tie']).double().mean()) <= 0.10, name
    if name == V.MIN_OPACITY[0]:
        for m in V.MIN_OPACITY[1]:
            near = (ref['opacity'] - m).abs() <= 4 * V.FLOORS[name][3]
            assert float(((ref['opacity'] < m) & ~near).double().mean()) >= 0.10 and float(((ref['opacity'] >= m) & ~near).double().mean()) >= 0.10


@pytest.mark.parametrize('name', list(V.CASES))
def test_case_regime_tie_cap_checker_and_floors(name):
    ref = V.reference(name)
    check_regime(name, ref)
    rb = V.reference(name, bf16=True)                      # the bf16-rounded grid is a scene of its own: same cap
    assert int(rb['tie'].sum()) <= int(V.TIE_CAP * rb['mask'].shape[0]), (name, 'bf16', int(rb['tie'].sum()))
    out = V.checker_fp32(name)
    assert not ((out['mask'] != ref['mask']).any(1) & ~ref['mask_tie']).any(), name           # masks equal off the mask-tie pixels
    err = V.output_errors(out, ref)
    print('[floor] %-20s (%d tie pixels of %d): %s' % (name, int(ref['tie'].sum()), ref['tie'].numel(), ' '.join('%s %.3e' % (k, err[k]) for k in V.OUTPUTS)))
    for k, floor in zip(V.OUTPUTS, V.FLOORS[name]):
        assert floor / 1.1 <= err[k] <= floor, (name, k, err[k], floor)
    # cls of the checker: the float64 argmax wherever the margin clears the bound the GPU test uses
    sem = out['sem'].double()
    clear = ~ref['tie'] & (ref['cls_margin'] > 2 * (4 * V.FLOORS[name][1]) * float(ref['semantic'][~ref['tie']].abs().max()))
    assert torch.equal(sem.argmax(-1)[clear], ref['cls'][clear]), name


def test_nan_probe_regime():
    name, voxel, k_sem, k_rgb = V.NAN_PROBE
    x, case = V.inputs(name), V.CASES[name]
    for bf16 in (False, True):
        sure, maybe = V.voxel_pixels(V.reference(name, bf16), x['t'], x['consts'], case['grid'], voxel)
        assert int(sure.sum()) >= 100 and int((~maybe).sum()) >= 100 and not bool((sure & ~maybe).any())
    assert 1 <= k_sem < 17 and 0 <= k_rgb < 3


@pytest.mark.parametrize('name', list(V.LABEL_CASES))
def test_label_views64_against_the_fp32_restatement(name):
    case, x, ref = V.LABEL_CASES[name], V.inputs(name), V.label_reference(name)
    R = ref['cls'].numel()
    assert int(ref['fragile'].sum()) <= int(V.FRAGILE_CAP * R), (name, int(ref['fragile'].sum()))
    assert int((ref['first'] >= 0).sum()) >= R // 10 and int((ref['first'] < 0).sum()) >= R // 20, name         # hits and misses
    assert len(torch.unique(ref['cls'])) >= 4
    if name == 'lab_255':
        assert int((ref['cls'] >= case['n_palette']).sum()) > R // 10 and int((ref['cls'] < case['n_palette'] - 1).sum()) > 0   # the palette clamp is exercised
    rows = RV.pixel_rays(x['K'], x['c2w'], case['hw'], case['stride'], case['origin']).reshape(-1, 9)
    cls, depth, last, first, fragile = RV.label_views(x['labels'], rows[:, 0:3], rows[:, 3:6], x['consts'], x['t'], case['empty_idx'])
    ok = ~(ref['fragile'].numpy() | fragile)
    print('[parity] %s: %d pixels, %d hits, fragile %d (float64) / %d (fp32 restatement)' % (name, R, int((ref['first'] >= 0).sum()),
                                                                                         int(ref['fragile'].sum()), int(fragile.sum())))
    np.testing.assert_array_equal(ref['cls'].numpy()[ok], cls[ok])
    np.testing.assert_array_equal(ref['first'].numpy()[ok], first[ok])
    np.testing.assert_array_equal(ref['alphainv_last'].numpy()[ok], last[ok])
    # depth: the restatement's fp32 value is the fp32 expression of the yardstick's hit; the float64 value within the derived bound
    np.testing.assert_allclose(depth[ok], V.label_depth_fp32(ref['first'].numpy(), x['t'], x['consts'])[ok], rtol=1e-6)
    assert np.abs(depth[ok] - ref['depth'].numpy()[ok]).max() <= V.LABEL_DEPTH_ABS * float(x['consts'][26])
