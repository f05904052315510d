"""Camera frames to network input on the device (ops.prepare_images / csrc/pw_image_prep.hip, transforms.PrepareImageInputs4DTraj)
against the reference fixture tests/golden/image_prep_small.npz and the numpy restatement tests/_image_prep_np.py, which
tests/test_image_prep_cpu.py pins byte for byte to Pillow.  No PIL and no reference here.

Bounds: the uint8 image (`canvas`) is array_equal; the float output is BIT-equal to the float32 formula
(canvas[..., ::-1].astype(f32) - mean32) * stdinv32 and within 5e-7 absolute of the fixture's float64-formula floats (two float32
roundings at |v| <= 2.64).  The kernel's tile is 32 rows x 64 columns of the output (PW_IMAGE_PREP_TH / _TW), a thread owns 4
neighbouring pixels of a row, and float4 / dword stores are used only when fW % 4 == 0: the shapes below cover one exact tile,
several tiles, ragged tiles with fW % 4 != 0, and flips of each."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _image_prep_np as IP  # noqa: E402
from preworld_amd import ops, transforms  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
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


def run(frames, augs, input_size):
    """one call for all frames -> (canvas uint8 (M,fH,fW,3), out float32 (M,3,fH,fW), launches) as numpy"""
    H, W = frames[0].shape[:2]
    plan = ops.image_prep_plan((H, W), input_size, augs, device=DEV)
    src = torch.from_numpy(np.stack(frames)).to(DEV)
    canvas = torch.full((len(frames),) + tuple(input_size) + (3,), 77, dtype=torch.uint8, device=DEV)
    out = torch.full((len(frames), 3) + tuple(input_size), float('nan'), device=DEV)
    got = ops.prepare_images(src, plan, out=out, canvas=canvas)
    assert got is out
    return canvas.cpu().numpy(), out.cpu().numpy(), plan.launches


def check_against_restatement(frames, augs, input_size, cv, out):
    for i, (f, a) in enumerate(zip(frames, augs)):
        want_cv, want = IP.prepare(f, a)
        assert np.array_equal(cv[i], want_cv), 'image %d: %d mismatching bytes' % (i, int((cv[i] != want_cv).sum()))
        assert np.array_equal(out[i].view(np.uint32), want.view(np.uint32)), 'image %d: float output differs in bits' % i


@pytest.mark.parametrize('name', CASE_NAMES)
def test_fixture_cases(fx, sample, name):
    augs = [_aug(fx[name + '_augs'][i // 2]) for i in range(12)]
    frames = sample['frames'][:12]
    cv, out, launches = run(frames, augs, (24, 64))
    assert np.array_equal(cv[::2], fx[name + '_canvas'])
    formula = np.moveaxis((cv[..., ::-1].astype(np.float32) - IP.MEAN32) * IP.STDINV32, -1, 1)
    assert np.array_equal(out.view(np.uint32), np.ascontiguousarray(formula).view(np.uint32))
    worst = float(np.abs(out.astype(np.float64) - fx[name + '_imgs']).max())
    print('%s: largest float difference to the fixture %.3g, %d launches' % (name, worst, launches))
    assert worst <= FLOAT_TOL
    assert launches == (1 if name == 'test' else 2)


SIX = [((64, 36), (0, 12, 64, 36), 0, 0.0),          # scale down, the test-time augmentation
       ((88, 49), (12, 25, 76, 49), 0, 0.0),         # scale up
       ((60, 33), (0, 9, 64, 33), 0, 0.0),           # crop wider than the resized image: zero columns on the right
       ((69, 39), (2, 15, 66, 39), 1, 0.0),          # flip
       ((72, 40), (4, 16, 68, 40), 0, 5.4),          # rotation, both signs
       ((60, 33), (0, 9, 64, 33), 1, -5.4)]


def test_one_call_for_twelve_images():
    frames = IP.synthetic_frames(5, 12, 45, 80)
    augs = [SIX[i // 2] for i in range(12)]
    cv, out, launches = run(frames, augs, (24, 64))
    assert launches == 2
    check_against_restatement(frames, augs, (24, 64), cv, out)
    for i in range(12):                                               # every image once more as a call of its own
        cv1, out1, l1 = run([frames[i]], [augs[i]], (24, 64))
        assert l1 == (2 if augs[i][3] else 1)
        assert np.array_equal(cv1[0], cv[i]) and np.array_equal(out1[0].view(np.uint32), out[i].view(np.uint32))
    unrot = [a for a in augs if not a[3]]
    cv, out, launches = run(frames[:len(unrot)], unrot, (24, 64))
    assert launches == 1                                               # no rotated image: one launch, no intermediate
    check_against_restatement(frames[:len(unrot)], unrot, (24, 64), cv, out)


@pytest.mark.parametrize('H,W,fH,fW', [(47, 83, 25, 67), (90, 160, 48, 128), (45, 80, 32, 64), (30, 40, 40, 64)],
                         ids=['ragged', 'two_by_two_tiles', 'one_exact_tile', 'upscale'])
def test_tile_edges(H, W, fH, fW):
    augs = [IP.eval_aug(H, W, fH, fW, 0.0, 0.0, 0), IP.eval_aug(H, W, fH, fW, 0.03, 0.0, 1), IP.eval_aug(H, W, fH, fW, -0.06, -0.01, 0),
            IP.eval_aug(H, W, fH, fW, 0.11, 5.4, 1), IP.eval_aug(H, W, fH, fW, 0.2, 4.0, 1), IP.eval_aug(H, W, fH, fW, -0.05, -5.4, 0)]
    # a crop that starts above and left of the resized image: zero rows on top, zero columns on the left
    augs.append(((augs[0][0]), (-3, -2, fW - 3, fH - 2), 1, 2.25))
    frames = IP.synthetic_frames(9, len(augs), H, W)
    cv, out, launches = run(frames, augs, (fH, fW))
    assert launches == 2
    check_against_restatement(frames, augs, (fH, fW), cv, out)


def test_band_near_the_lds_limit():
    """6.1 x down-scaling in y: a 32-row band of the output stages 214 source rows, a dynamic-LDS launch near the 224-row
    (56 KiB) limit; 1.5 x in x"""
    frames = IP.synthetic_frames(13, 3, 256, 96)
    augs = [((64, 42), (0, 5, 64, 37), 0, 0.0), ((64, 42), (0, 5, 64, 37), 1, 3.7), ((64, 43), (0, 11, 64, 43), 0, -2.25)]
    plan = ops.image_prep_plan((256, 96), (32, 64), augs, device=DEV)
    assert 200 <= plan.rows_max <= 224
    cv, out, launches = run(frames, augs, (32, 64))
    assert launches == 2
    check_against_restatement(frames, augs, (32, 64), cv, out)


def test_real_size_once():
    """900 x 1600 -> 512 x 1408 at the test-time augmentation and at a rotated, flipped training augmentation with newW < 1408"""
    frame = IP.synthetic_frames(2, 1, 900, 1600)[0]
    augs = [IP.eval_aug(900, 1600, 512, 1408), ((1312, 738), (0, 226, 1408, 738), 1, -5.4)]
    assert augs[0] == ((1408, 792), (0, 280, 1408, 792), 0, 0.0)
    cv, out, launches = run([frame, frame], augs, (512, 1408))
    assert launches == 2
    check_against_restatement([frame, frame], augs, (512, 1408), cv, out)
    assert (cv[1][:, :64] == 0).all() or (cv[1][:, -64:] == 0).all()         # the zero-filled columns are there


def test_capture_and_replay():
    frames_a, frames_b = IP.synthetic_frames(21, 4, 45, 80), IP.synthetic_frames(22, 4, 45, 80)
    augs = [SIX[0], SIX[3], SIX[4], SIX[5]]
    plan = ops.image_prep_plan((45, 80), (24, 64), augs, device=DEV)
    src = torch.from_numpy(np.stack(frames_a)).to(DEV)
    out = torch.zeros(4, 3, 24, 64, device=DEV)
    canvas = torch.zeros(4, 24, 64, 3, dtype=torch.uint8, device=DEV)
    ops.prepare_images(src, plan, out=out, canvas=canvas)              # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.prepare_images(src, plan, out=out, canvas=canvas)
    src.copy_(torch.from_numpy(np.stack(frames_b)).to(DEV))
    out.zero_()
    canvas.zero_()
    g.replay()
    torch.cuda.synchronize()
    got, got_cv = out.cpu().numpy().copy(), canvas.cpu().numpy().copy()
    eager_cv, eager, _ = run(frames_b, augs, (24, 64))
    assert np.array_equal(got_cv, eager_cv) and np.array_equal(got.view(np.uint32), eager.view(np.uint32))
    check_against_restatement(frames_b, augs, (24, 64), got_cv, got)


@pytest.mark.parametrize('name', ['test', 'train0'])
def test_pipeline_end_to_end(fx, sample, name):
    import _e2e_stub as E
    from preworld_amd import harness, synth as S
    is_train = name != 'test'
    t = transforms.PrepareImageInputs4DTraj(dict(IP.DATA_CONFIG), is_train=is_train, sequential=True, device=DEV)
    np.random.seed(0)
    res = t({k: sample[k] for k in ('curr', 'adjacent', 'temporal_ann_infos', 'frames')})
    imgs, s2e, e2g, intr, pr, pt = res['img_inputs']
    assert imgs.is_cuda and imgs.dtype == torch.float32 and imgs.shape == (12, 3, 24, 64)
    for got_t, key in ((s2e, 'sensor2egos'), (e2g, 'ego2globals'), (intr, 'intrins'), (pr, 'post_rots'), (pt, 'post_trans')):
        assert not got_t.is_cuda and np.array_equal(got_t.numpy(), fx['%s_%s' % (name, key)]), key
    # camera-major, frame-minor: image 2 c is camera c's key frame (the canvas), 2 c + 1 its adjacent frame
    assert len(res['canvas']) == 6 and np.array_equal(np.stack(res['canvas']), fx[name + '_canvas'])
    assert float((imgs.cpu().numpy().astype(np.float64) - fx[name + '_imgs']).__abs__().max()) <= FLOAT_TOL
    assert res['gt_depths'].shape == (6, 1) and sorted(res['temporal_img_inputs']) == [1, 2, 3, 4, 5, 6]
    for k in range(1, 7):
        ti = res['temporal_img_inputs'][k]
        assert ti[0].is_cuda and ti[0].shape == (12, 3, 24, 64)
        assert np.array_equal(ti[4].numpy(), fx['%s_t%d_post_rots' % (name, k)]) and np.array_equal(ti[2].numpy(), fx['%s_t%d_ego2globals' % (name, k)])
    if name == 'train0':
        for j, k in enumerate((1, 6)):
            assert float(np.abs(res['temporal_img_inputs'][k][0].cpu().numpy().astype(np.float64) - fx['train0_t_imgs'][j]).max()) <= FLOAT_TOL
    # the detector takes it as it is: batch dimension and the BEV augmentation added, as the collate / LoadAnnotations steps do
    net = harness.build_model(E.model_cfg('PreWorld4DTraj', True, True), S.synth_state_dict(0), DEV)
    inputs = tuple(x[None].to(DEV) for x in res['img_inputs']) + (torch.eye(3, device=DEV)[None],)
    prep = net.prepare_inputs(inputs, stereo=True, num_frame=2, temporal_frame=1, extra_ref_frames=1)
    assert len(prep[0]) == 2 and tuple(prep[0][0].shape) == (1, 6, 3, 24, 64) and tuple(prep[1][0].shape) == (1, 6, 4, 4)
    assert torch.equal(prep[0][1][0, 2], imgs[5])                      # frame 1 of camera 2 is image 2 * 2 + 1
