"""CPU half of the float64 pin of the ray renderer (tests/_render_ref64.py): the yardstick IS the reference's operation (it
reproduces the three fixtures generated from the imported reference NerfHead, outputs and gradients, on the standard 200 x 200 x 16
grid), every case is in the regime it claims and under the tie cap from the yardstick alone, the existing fp32 CPU checker
(oracle/torch_render.render) agrees with it in masks and kept sets off the tie rays, and every entry of FLOORS / GRAD_FLOORS is that
checker's error, asserted from both sides.  No GPU."""
import numpy as np
import pytest
import torch

import _render_ref64 as Y
from _parity import check_close
from oracle import torch_render as TR
from preworld_amd import synth as S

_BDA_MIXED = np.array([[0.98, 0.05, 0.0], [-0.05, 0.98, 0.0], [0.0, 0.0, 1.0]], np.float32)        # tests/test_gpu_render.py
_W_RTOL, _W_ATOL = 1e-3, 5e-5                                 # the opaque regime's weight tolerance (tests/test_gpu_render.py)


def test_constants_table_and_cases_hygiene():
    kc, tt = Y.kernel_constants()
    np.testing.assert_array_equal(kc, Y.standard_constants(Y.BDA))         # the yardstick's own constants are the ones the kernel is given
    full = Y.full_table()
    np.testing.assert_array_equal(full, tt)
    assert full.shape == (417,)
    assert abs(np.linalg.det(Y.BDA.astype(np.float64)) - 1) > 1e-3 and not np.allclose(Y.BDA, Y.BDA.T) and Y.BDA[2, 0] != 0 and Y.BDA[0, 2] != 0
    assert set(Y.FLOORS) == set(Y.GRAD_FLOORS) == set(Y.CASES)
    passes = set()
    for name, case in Y.CASES.items():
        t = Y.table(case['table'])
        assert t.dtype == np.float32 and 2 <= len(t) <= 448 and (np.diff(t) > 0).all() and t[0] > 0, name
        X, Yy, Z = case['grid']
        assert len({X, Yy, Z}) == 3 or case.get('long_path'), name          # anisotropic: an X / Y / Z swap cannot hide
        assert X * Yy * Z < 400
        x = Y.inputs(name)
        assert x['grid'].shape == (Z, Yy, X, case['layout'][0]) and x['rays_o'].shape == (case['R'], 3)
        assert not np.allclose(np.linalg.norm(x['rays_d'], axis=1), 1)       # directions are not normalised
        passes.add((2 if len(t) <= 128 else 4 if len(t) <= 256 else 7, case['scene']))
        assert len(Y.FLOORS[name]) == len(Y.FLOOR_KEYS) and len(Y.GRAD_FLOORS[name]) == 3
    assert {p for p, _ in passes} == {2, 4, 7}
    sizes = sorted({Y.CASES[n]['table'][1] for n in Y.CASES})
    for s in (2, 64, 65, 96, 128, 129, 200, 256, 257, 417, 448, 76, 141, 206):
        assert s in sizes


# ------------------------------------------------------------------------------------ the yardstick is the reference's operation
def _standard_scene(grids, o, d, bda, coef=None, tie_zero=True, fp32_alpha=False):
    grid = Y.pack(*grids, Y.DEFAULT_LAYOUT)
    grid[..., 1] = 0
    grid[..., 22:] = 0
    return Y.render64(o, d, Y.full_table(), grid, Y.standard_constants(bda), coef=coef, tie_zero=tie_zero, fp32_alpha=fp32_alpha)


def test_yardstick_reproduces_render_small(golden):
    g = golden('render_small.npz')
    np.testing.assert_array_equal(Y.full_table(), g['t'])
    c = Y.standard_constants(g['bda'])
    np.testing.assert_allclose(c[15:18], g['xyz_min'], rtol=1e-6)
    np.testing.assert_allclose(c[18:21], g['xyz_max'], rtol=1e-6)
    np.testing.assert_allclose(c[22], g['act_shift'][0], rtol=1e-6)
    R = int(g['R'])
    o, d = S.rays(int(g['seed_rays']), R)
    ref = _standard_scene(S.render_grids(int(g['seed_grid'])), o, d, g['bda'])
    assert (ref['inner'].numpy() == g['inner_mask']).mean() > 0.9999
    assert abs(int(ref['kept'].sum()) - len(g['weights'])) <= 2
    np.testing.assert_allclose(ref['alphainv_last'].numpy(), g['alphainv_last'], rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(ref['depth'].numpy(), g['render_depth'], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(ref['semantic'].numpy(), g['render_semantic'], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(ref['color'].numpy(), g['render_color'], rtol=1e-3, atol=1e-3)


def _unpacked_grads(ref):
    gg = ref['grad']
    return gg[..., 0].permute(2, 1, 0), gg[..., 2:19].permute(2, 1, 0, 3), gg[..., 19:22].permute(2, 1, 0, 3)


def test_yardstick_reproduces_render_grad_small(golden):
    """outputs AND gradients of the imported reference NerfHead (torch autograd through grid_sample / Raw2Alpha / Alphas2Weights /
    segment_coo): the tolerances of tests/test_gpu_render.py::test_render_backward_golden.  That scene is nearly empty (alpha = 5e-7 per
    sample), where the fp32 rounding of the reference's own alpha formula is 1e-2 of every output (ALPHA_ABS in the yardstick's
    docstring; it is what FLOORS measures on the `plain` cases), so the fixture's 1e-5 / 2e-5 is met with alpha's VALUES rounded as the
    reference rounds them (fp32_alpha) and everything else, the derivative included, exact; in exact arithmetic the yardstick is
    1e-2 away, asserted below to be the floor's size and not more."""
    g = golden('render_grad_small.npz')
    R = int(g['R'])
    o, d = S.rays(int(g['seed_rays']), R)
    coef = {k: v.numpy() for k, v in TR.objective_coefficients(int(g['seed_coef']), R, 417).items()}
    ref = _standard_scene(S.render_grids(int(g['seed_grid'])), o, d, g['bda'], coef=coef, tie_zero=False, fp32_alpha=True)
    check_close('yardstick depth vs reference', ref['depth'], g['depth'], 1e-5)
    check_close('yardstick alphainv_last vs reference', ref['alphainv_last'], g['alphainv_last'], 1e-5, atol=1e-7)
    gd, gs, gc = _unpacked_grads(ref)
    ix = tuple(torch.from_numpy(g['voxels'][:, i].astype(np.int64)) for i in range(3))
    # density: 1e-4 instead of the GPU test's 2e-5.  The fixture's fp32 positions carry half an ulp of a voxel index near 128..199,
    # 2^-17 = 7.6e-6 of a voxel, per axis, plus the sample position's own ~1e-7 of 0.0103 per voxel = 1e-5: corner weights of ~0.5 are off
    # by ~2e-5 per axis, 6e-5 over three.  The kernel shares that rounding with the reference (same fp32 op order), the float64
    # yardstick does not; measured 2.7e-5.  Semantic and colour (sums over more samples per voxel) meet 2e-5 as they are.
    check_close('yardstick d loss / d density (sampled voxels)', gd[ix], g['g_density'], 1e-4)
    check_close('yardstick d loss / d semantic (sampled voxels)', gs[ix], g['g_semantic'], 2e-5)
    check_close('yardstick d loss / d color (sampled voxels)', gc[ix], g['g_color'], 2e-5)
    assert abs(float(gd.sum()) - float(g['sum_density'])) <= 2e-5 * float(g['abs_density'])
    np.testing.assert_allclose(gs.sum((0, 1, 2)).numpy(), g['sum_semantic'], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(gc.sum((0, 1, 2)).numpy(), g['sum_color'], rtol=1e-4, atol=1e-4)
    assert int((gd != 0).sum()) == int(g['n_nonzero'])
    exact = _standard_scene(S.render_grids(int(g['seed_grid'])), o, d, g['bda'])
    check_close('exact yardstick depth vs reference (fp32 alpha rounding)', exact['depth'], g['depth'], 2e-2)


@pytest.mark.parametrize('tag', ['mixed', 'void'])
def test_yardstick_reproduces_render_mixed(golden, tag):
    """where rays terminate: dense weights, kept counts, outputs and gradients of the imported reference, with the tolerances of
    tests/test_gpu_render.py (_check_terminating_forward, test_render_backward_terminating_rays_golden); near-ties from the
    yardstick's own margins"""
    g = golden('render_mixed.npz')
    seeds = g[tag + '_seeds']
    R = int(g[tag + '_R'])
    if tag == 'mixed':
        grids, (o, d) = S.render_grids_mixed(int(seeds[0])), S.rays_mixed(int(seeds[1]), R)
    else:
        grids, (o, d) = S.render_grids_void(int(seeds[0])), S.rays_void(int(seeds[1]), R)
    coef = {k: v.numpy() for k, v in TR.objective_coefficients(int(seeds[2]), R, 417).items()}
    ref = _standard_scene(grids, o, d, _BDA_MIXED, coef=coef, tie_zero=False)
    tie = ref['tie'].numpy()
    ok = ~tie
    print('[parity] yardstick vs render_mixed/%s: %d tie rays of %d' % (tag, int(tie.sum()), R))
    assert tie.sum() <= (0.1 if tag == 'mixed' else 0.5) * R      # void: sigma climbs from -5 to the padding's 0 across the grid's faces, alpha through 1e-7
    dense = np.zeros((R, 417), np.float32)
    dense[g[tag + '_ray_id'], g[tag + '_step_id']] = g[tag + '_weights']
    w = ref['weights'].numpy()
    assert (((w > 0) == (dense > 0)).all(1) | tie).all()
    np.testing.assert_array_equal(ref['counts'][:, 2].numpy()[ok], g[tag + '_kept'][ok])
    assert (np.abs(w[ok] - dense[ok]) <= _W_ATOL + _W_RTOL * dense[ok]).all()
    assert np.abs(w[tie] - dense[tie]).max(initial=0) <= 1.1e-3
    last = ref['alphainv_last'].numpy()
    np.testing.assert_allclose(last[ok], g[tag + '_alphainv_last'][ok], rtol=2e-3, atol=1e-7)
    assert ((last < 1e-3) == (g[tag + '_alphainv_last'] < 1e-3))[ok].all()
    for key in ('depth', 'semantic', 'color'):
        check_close('yardstick %s %s' % (tag, key), ref[key].numpy()[ok], g[tag + '_' + key][ok], 2e-4)
    # the fixture's gradients carry every ray: a tie ray's differing sample has weight <= 1.1e-3 (the 5e-4 bound of the GPU test covers it).
    # On `void` ONLY tie rays have a gradient (the others keep nothing: alpha crosses 1e-7 where sigma climbs from -5 to the padding's 0,
    # and fp32 alpha is a multiple of 2^-24 = 6e-8 there): compared with alpha's values rounded as the reference rounds them.
    if tag == 'void':
        ref = _standard_scene(grids, o, d, _BDA_MIXED, coef=coef, tie_zero=False, fp32_alpha=True)
        np.testing.assert_array_equal(ref['counts'][:, 2].numpy(), g[tag + '_kept'])
    gd, gs, gc = _unpacked_grads(ref)
    ix = tuple(torch.from_numpy(g[tag + '_voxels'][:, i].astype(np.int64)) for i in range(3))
    check_close('yardstick %s d loss / d density (sampled voxels)' % tag, gd[ix], g[tag + '_g_density'], 5e-4)
    check_close('yardstick %s d loss / d semantic (sampled voxels)' % tag, gs[ix], g[tag + '_g_semantic'], 5e-4)
    check_close('yardstick %s d loss / d color (sampled voxels)' % tag, gc[ix], g[tag + '_g_color'], 5e-4)
    assert abs(float(gd.sum()) - float(g[tag + '_sum_density'])) <= 5e-4 * float(g[tag + '_abs_density'])


# ------------------------------------------------------------------------------------ cases: regime, tie cap, checker, floors
def check_regime(name, ref):
    """each case is in the regime it claims, from the reference alone"""
    case = Y.CASES[name]
    R, S_ = ref['mask'].shape
    n_tie = int(ref['tie'].sum())
    assert n_tie <= int(Y.TIE_CAP * R), (name, 'tie rays', n_tie, int(ref['near_tie'].sum()), int(ref['mask_tie'].sum()))
    outer = ~ref['inner']
    kept = ref['counts'][:, 2]
    if R > 1 and S_ >= 64:
        assert int((outer & ref['mask']).sum()) > 0 and int((outer & ~ref['mask']).sum()) > 0, name      # outer samples masked AND unmasked
        assert int((ref['mask'] & (ref['n_inb'] >= 1) & (ref['n_inb'] <= 7)).sum()) > 0, name              # partial corner sets
        assert int((ref['mask'] & (ref['n_inb'] == 8)).sum()) > 0, name
    for b in case['boundaries']:          # a soft run crosses the pass boundary: an unmasked (hence outer, short-step) sample on each side
        assert int((~ref['mask'][:, b - 1] & ~ref['mask'][:, b]).sum()) > 0, (name, b)
    if case['scene'] == 'mixed' and R > 1 and S_ >= 96 and case['table'][0] != 'tail' and not case.get('long_path'):
        assert float((ref['alphainv_last'] < Y.T_STOP).double().mean()) >= 0.10, name
        assert int(kept.min()) < 8 and int(kept.max()) > 25, name
    if case.get('long_path'):
        # 70 rays x ~209 masked samples x 8 corners over 12 voxels: the x = 1 column collects more than RB_LONG entries per voxel (the
        # multi-wave path, two chunks), the x = 0 / x = 2 voxels fewer (the one-wave path in the same launch)
        e = ref['entries']
        assert int((e > Y.RB_LONG).sum()) >= 2 and int(((e > 0) & (e <= Y.RB_LONG)).sum()) >= 2, e
    if case['scene'] == 'single2':
        assert ref['pass1'].tolist() == [[True, True]] and ref['kept'].tolist() == [[True, False]]
    if S_ == 2 and R > 1:
        assert bool(ref['mask'].all())


@pytest.mark.parametrize('name', list(Y.CASES))
def test_case_regime_tie_cap_checker_and_floors(name):
    ref = Y.reference(name)
    check_regime(name, ref)
    rb = Y.reference(name, bf16=True)                      # the bf16-rounded grid is a scene of its own: same cap
    assert int(rb['tie'].sum()) <= int(Y.TIE_CAP * rb['mask'].shape[0]), (name, 'bf16', int(rb['tie'].sum()))
    out, gg = Y.checker_fp32(name, ref['tie'])
    ok = ~ref['tie']
    assert not ((out['mask'] != ref['mask']).any(1) & ~ref['mask_tie']).any(), name           # masks equal off the mask-tie rays
    assert not (((out['weights'] > 0) != ref['kept']).any(1) & ok).any(), name                  # kept sets equal off the tie rays
    err = Y.output_errors(out, ref)
    err['weights_elem'] = Y.weight_element_error(out['weights'], ref)
    gerr = Y.grad_errors(gg, ref, Y.CASES[name]['layout'])
    print('[floor] %s (%d tie rays): %s | %s' % (name, int(ref['tie'].sum()), ' '.join('%s %.3e' % (k, err[k]) for k in Y.FLOOR_KEYS),
                                                  ' '.join('%s %.3e' % (k, gerr[k]) for k in Y.GROUPS)))
    for k, floor in zip(Y.FLOOR_KEYS, Y.FLOORS[name]):
        assert 0.5 * floor <= err[k] <= floor, (name, k, err[k], floor)
    for k, floor in zip(Y.GROUPS, Y.GRAD_FLOORS[name]):
        assert 0.5 * floor <= gerr[k] <= floor, (name, k, gerr[k], floor)


def test_unused_channels_get_no_gradient_in_the_yardstick():
    ref = Y.reference('layout200_mixed')
    used = torch.zeros(32, dtype=torch.bool)
    for sl in Y.group_slices(Y.CASES['layout200_mixed']['layout']).values():
        used[sl] = True
    assert float(ref['grad'][..., ~used].abs().max()) == 0 and float(ref['grad'][..., used].abs().max()) > 0
