"""Camera frames to network input, the part that needs no GPU: the numpy restatement (tests/_image_prep_np.py) against the
reference fixture (tests/golden/image_prep_small.npz, tools/gen_golden_images.py) and against the installed Pillow, the host plan
of ops.image_prep_plan, the transform's sampling and bookkeeping, argument validation and registration.

Bounds: uint8 images, post_rots / post_trans and the augmentation tuples are compared with array_equal.  The float output is
held to 5e-7 absolute against the fixture: the fixture's normalise is float32((float64(px) - mean) / std), the restatement's is
two float32 roundings (a subtract, a multiply by the rounded reciprocal) at |v| <= 2.64, the largest normalised value."""
import numpy as np
import pytest
import torch

import _image_prep_np as IP
from preworld_amd import _lib, ops, transforms

FLOAT_TOL = 5e-7
CASE_NAMES = ['test', 'train0', 'train1', 'train2']


@pytest.fixture(scope='module')
def fx(golden):
    return golden('image_prep_small.npz')


@pytest.fixture(scope='module')
def sample(fx):
    H, W = [int(v) for v in fx['src_size']]
    return IP.synthetic_sample(int(fx['sample_seed']), H, W, n_adj=1)


def _aug(row):
    return (int(row[1]), int(row[2])), tuple(int(v) for v in row[3:7]), int(row[7]), float(row[8])


def fixture_job(fx, sample, name):
    """(frame, aug) of the 12 images of img_inputs, in order"""
    augs = fx[name + '_augs']
    return [(sample['frames'][i], _aug(augs[i // 2])) for i in range(12)]


@pytest.mark.parametrize('name', CASE_NAMES)
def test_restatement_vs_fixture(fx, sample, name):
    job = fixture_job(fx, sample, name)
    want_cv, want = fx[name + '_canvas'], fx[name + '_imgs']
    worst = 0.0
    for i, (frame, aug) in enumerate(job):
        cv, out = IP.prepare(frame, aug)
        if i % 2 == 0:
            assert np.array_equal(cv, want_cv[i // 2]), (name, i)
        worst = max(worst, float(np.abs(out.astype(np.float64) - want[i]).max()))
    print('%s: largest float difference to the fixture %.3g' % (name, worst))
    assert worst <= FLOAT_TOL
    assert float(np.abs(want).max()) <= 2.6401


def test_fixture_says_what_it_is(fx):
    assert int(fx['normalize_restated']) == 1 and str(fx['pil_version'])
    a = np.concatenate([fx[n + '_augs'][:6] for n in CASE_NAMES])
    fW = int(fx['input_size'][1])
    assert (a[:, 1] < fW).any() and (a[:, 1] > fW).any() and (a[:, 7] == 1).any() and (a[:, 8] > 1).any() and (a[:, 8] < -1).any()


@pytest.mark.parametrize('case', IP.CASES, ids=lambda c: '%dx%d_%dx%d_%g_%g_%d' % c)
def test_restatement_vs_pil(case):
    Image = pytest.importorskip('PIL.Image')
    H, W, fH, fW, off, angle, flip = case
    aug = IP.eval_aug(H, W, fH, fW, off, angle, flip)
    img = IP.synthetic_frames(3, 1, H, W)[0]
    p = Image.fromarray(img).resize(aug[0]).crop(aug[1])
    if flip:
        p = p.transpose(method=Image.FLIP_LEFT_RIGHT)
    want = np.array(p.rotate(angle))
    got = IP.canvas(img, aug)
    assert want.min() == 0 and want.max() == 255                     # the frames do reach both clips
    assert np.array_equal(got, want), '%d mismatching bytes' % int((got != want).sum())


def test_host_plan_equals_restatement():
    for n_in, n_out in [(80, 64), (45, 36), (80, 60), (40, 72), (30, 54), (83, 62), (64, 64), (1600, 1408), (900, 792), (1600, 1312)]:
        b, c = ops.image_resize_table(n_in, n_out)
        wb, wc = IP.axis_table(n_in, n_out)
        assert b.dtype == np.int32 and c.dtype == np.int32 and np.array_equal(b, wb) and np.array_equal(c, wc), (n_in, n_out)
    for angle in (3.7, -5.4, 5.4, -0.01, 2.25, 4.0):
        for w, h in ((64, 24), (67, 25), (1408, 512)):
            assert ops.image_rotation_fixed(angle, w, h) == IP.rotation_fixed(angle, w, h)
    augs = [IP.eval_aug(900, 1600, 512, 1408), ((1312, 738), (0, 226, 1408, 738), 1, -5.4)]
    H, W, fH, fW, params, tables, offsets, rows_max = ops._image_prep_host((900, 1600), (512, 1408), augs)
    assert params.shape == (2, ops.IMAGE_PREP_NPARAM) and list(params[0, :6]) == [1408, 792, 0, 280, 0, 0]
    assert list(params[1, :6]) == [1312, 738, 0, 226, 1, 1] and tuple(params[1, 6:12]) == IP.rotation_fixed(-5.4, 1408, 512)
    for i, (n_in, n_out) in enumerate([(1600, 1408), (900, 792)]):
        off, ks = offsets[(n_in, n_out)]
        assert (off, ks) == tuple(params[0, 12 + 2 * i:14 + 2 * i])
        wb, wc = IP.axis_table(n_in, n_out)
        assert np.array_equal(tables[off:off + 2 * n_out].reshape(-1, 2), wb)
        assert np.array_equal(tables[off + 2 * n_out:off + (2 + ks) * n_out].reshape(-1, ks), wc)
    vb = IP.axis_table(900, 792)[0]
    assert rows_max >= int(vb[311, 0] + vb[311, 1] - vb[280, 0]) and rows_max <= 224
    with pytest.raises(_lib.PreworldHipError):
        ops._image_prep_host((900, 1600), (512, 1408), [((1408, 792), (0, 280, 1408, 792), 0, 45.0)])       # |angle| >= 45
    with pytest.raises(_lib.PreworldHipError):
        ops._image_prep_host((900, 1600), (512, 1408), [((1408, 792), (0, 280, 1400, 792), 0, 0)])          # crop is not input_size
    with pytest.raises(_lib.PreworldHipError):
        ops._image_prep_host((9000, 1600), (32, 1408), [((1408, 32), (0, 0, 1408, 32), 0, 0)])              # band too tall for LDS


class _NoPixels(transforms.PrepareImageInputs4DTraj):
    def _run(self, job):
        self.job = job
        fH, fW = self.data_config['input_size']
        return torch.zeros(len(job), 3, fH, fW), torch.zeros(len(job), fH, fW, 3, dtype=torch.uint8)


@pytest.mark.parametrize('name', CASE_NAMES)
def test_transform_sampling_and_bookkeeping(fx, sample, name):
    """the same seed draws the reference's augmentations; post_rots / post_trans and the poses are bit-equal to its tensors"""
    is_train = name != 'test'
    t = _NoPixels(dict(IP.DATA_CONFIG), is_train=is_train, sequential=True, device='cpu')
    np.random.seed(int(name[5:]) if is_train else 0)
    res = t({k: sample[k] for k in ('curr', 'adjacent', 'temporal_ann_infos', 'frames')})
    want = fx[name + '_augs']
    assert len(t.job) == 84 and want.shape == (42, 9)
    got = np.array([[0.0, a[0][0], a[0][1]] + list(a[1]) + [float(a[2]), a[3]] for _, a in t.job[::2]])
    assert np.array_equal(got[:, 1:], want[:, 1:])
    imgs, s2e, e2g, intr, pr, pt = res['img_inputs']
    assert imgs.shape == (12, 3, 24, 64) and list(res['cam_names']) == IP.CAM_NAMES
    for got_t, key in ((s2e, 'sensor2egos'), (e2g, 'ego2globals'), (intr, 'intrins'), (pr, 'post_rots'), (pt, 'post_trans')):
        assert got_t.dtype == torch.float32 and np.array_equal(got_t.numpy(), fx['%s_%s' % (name, key)]), key
    assert np.array_equal(res['gt_depths'].numpy(), fx[name + '_gt_depths'])
    for k in range(1, 7):
        ti = res['temporal_img_inputs'][k]
        assert ti[0].shape == (12, 3, 24, 64)
        assert np.array_equal(ti[4].numpy(), fx['%s_t%d_post_rots' % (name, k)]) and np.array_equal(ti[5].numpy(), fx['%s_t%d_post_trans' % (name, k)])
        assert np.array_equal(ti[2].numpy(), fx['%s_t%d_ego2globals' % (name, k)])
    # frame order: camera-major, frame-minor, the files in the order the reference opens them
    for i, (f, _) in enumerate(t.job):
        assert f is sample['frames'][i]


class _NoPixelsBase(transforms.PrepareImageInputs):
    _run = _NoPixels._run


@pytest.mark.parametrize('name', ['test', 'train1'])
def test_base_class_call(fx, sample, name):
    """PrepareImageInputs itself (the non-temporal class): the same draws and tensors as the first group of the 4DTraj
    class, which consumes np.random first for the current sample"""
    is_train = name != 'test'
    t = _NoPixelsBase(dict(IP.DATA_CONFIG), is_train=is_train, sequential=True, device='cpu')
    np.random.seed(int(name[5:]) if is_train else 0)
    res = t({k: sample[k] for k in ('curr', 'adjacent')} | dict(frames=sample['frames'][:12]))
    assert len(t.job) == 12 and 'temporal_img_inputs' not in res and list(res['cam_names']) == IP.CAM_NAMES
    got = np.array([[a[0][0], a[0][1]] + list(a[1]) + [float(a[2]), a[3]] for _, a in t.job[::2]])
    assert np.array_equal(got, fx[name + '_augs'][:6, 1:])
    assert all(a == b for (_, a), (_, b) in zip(t.job[::2], t.job[1::2]))          # the adjacent frame shares the augmentation
    imgs, s2e, e2g, intr, pr, pt = res['img_inputs']
    assert imgs.shape == (12, 3, 24, 64) and len(res['canvas']) == 6 and res['canvas'][0].shape == (24, 64, 3)
    for got_t, key in ((s2e, 'sensor2egos'), (e2g, 'ego2globals'), (intr, 'intrins'), (pr, 'post_rots'), (pt, 'post_trans')):
        assert np.array_equal(got_t.numpy(), fx['%s_%s' % (name, key)]), key
    assert np.array_equal(res['gt_depths'].numpy(), fx[name + '_gt_depths'])
    # without adjacent frames: 6 images, 6 rows of everything
    t = _NoPixelsBase(dict(IP.DATA_CONFIG), is_train=False, sequential=False, device='cpu')
    res = t(dict(curr=sample['curr'], frames=sample['frames'][:12:2]))
    assert len(t.job) == 6 and all(x.shape[0] == 6 for x in res['img_inputs'])
    assert np.array_equal(res['img_inputs'][4].numpy(), fx['test_post_rots'][:6])


def test_load_depth_and_loader():
    with pytest.raises(NotImplementedError):
        transforms.PrepareImageInputs(dict(IP.DATA_CONFIG), load_depth=True)
    seen = []
    t = _NoPixels(dict(IP.DATA_CONFIG), sequential=False, device='cpu',
                  loader=lambda p: (seen.append(p), np.zeros((45, 80, 3), np.uint8))[1])
    s = IP.synthetic_sample(1, 45, 80, n_adj=0)
    t({k: s[k] for k in ('curr', 'adjacent', 'temporal_ann_infos')})
    assert len(seen) == 42 and seen[:6] == [s['curr']['cams'][n]['data_path'] for n in IP.CAM_NAMES]
    with pytest.raises(ValueError):
        t(dict(curr=s['curr'], temporal_ann_infos=s['temporal_ann_infos'], frames=[np.zeros((45, 80, 3), np.float32)] * 42))


def test_new_entry_points_validate_before_any_hip_call():
    l = _lib.lib()
    one = 0x1000                                     # a non-null address that is never dereferenced: validation fails first
    ok = dict(src=one, M=12, H=900, W=1600, fH=512, fW=1408, params=one, tables=one, n_table=1000, rows_max=43, any_rot=0, ws=None,
              out=one, canvas=None, launches_host=None, stream=None)
    bad = [dict(src=None), dict(params=None), dict(tables=None), dict(out=None), dict(M=0), dict(M=70000), dict(H=0), dict(W=40000),
           dict(fH=0), dict(fW=-3), dict(n_table=0), dict(rows_max=0), dict(rows_max=225), dict(any_rot=1), dict(out=0x1002)]
    for b in bad:
        rc = l.pw_image_prep(*dict(ok, **b).values())
        assert rc == -1, (b, rc)
        assert b'pw_image_prep' in l.pw_last_error(), (b, l.pw_last_error())
    assert l.pw_image_prep_ws_bytes(12, 512, 1408, 0) == 0
    assert l.pw_image_prep_ws_bytes(12, 512, 1408, 1) >= 12 * 512 * 1408 * 3
    with pytest.raises(_lib.PreworldHipError):
        ops.image_prep_plan((45, 80), (24, 64), [], device='cpu')
    plan = ops.image_prep_plan((45, 80), (24, 64), [IP.eval_aug(45, 80, 24, 64)], device='cpu')
    assert plan.any_rot is False and plan.ws is None and plan.M == 1
    with pytest.raises(_lib.PreworldHipError):
        ops.prepare_images(torch.zeros(1, 45, 81, 3, dtype=torch.uint8), plan)                # wrong frame size
    with pytest.raises(_lib.PreworldHipError):
        ops.prepare_images(torch.zeros(1, 45, 80, 3, dtype=torch.uint8), plan)                # not on the device


def test_registration():
    class Reg:
        def __init__(self):
            self.d = {}

        def register_module(self, name=None, force=False, module=None):
            assert force
            self.d[name] = module
    reg = Reg()
    assert transforms.register_image_pipelines(reg) == ['PrepareImageInputs', 'PrepareImageInputs4DTraj']
    assert reg.d == dict(PrepareImageInputs=transforms.PrepareImageInputs, PrepareImageInputs4DTraj=transforms.PrepareImageInputs4DTraj)
    reg = Reg()
    assert transforms.register_pipelines(reg) == ['PointToMultiViewDepth'] and list(reg.d) == ['PointToMultiViewDepth']
