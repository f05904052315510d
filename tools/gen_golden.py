"""Generate tests/golden/*.npz by importing the reference's Python modules.

Runs ONLY in the development container (needs /root/reference, which does not exist
on the GPU box).  It contains no reference source: it pre-seeds sys.modules with
minimal stand-ins for the packages the reference imports but this image lacks
(mmcv, mmdet, torch_scatter, ...), loads the reference files with importlib and
records inputs -> outputs as data fixtures.  The three native extensions the
reference binds (bev_pool_v2_ext, render_utils_cuda, ub360_utils_cuda) are CUDA-only
and cannot be built here, so they are bound to oracle/pw_oracle.c; for those three
the fixtures pin the reference's *Python wrappers + composition*, and the only
independent pin of the kernel arithmetic itself is the reference KAT
(mmdet3d/ops/bev_pool_v2/bev_pool.py:145-176) recorded in kat_bev_pool_v2.npz.

    python tools/gen_golden.py            # writes tests/golden/*.npz
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
OUT = os.path.join(REPO, 'tests', 'golden')
sys.path.insert(0, REPO)
from oracle import oracle as O  # noqa: E402
from preworld_amd import synth as S  # noqa: E402


# ----------------------------------------------------------------------------- shim
def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__path__ = []
    sys.modules[name] = m
    return m


class _Registry:
    def __init__(self, *a, **k):
        self.d = {}

    def register_module(self, name=None, force=False, module=None):
        def deco(cls):
            self.d[name or cls.__name__] = cls
            return cls
        return deco(module) if module is not None else deco


def _build_norm_layer(cfg, num_features, postfix=''):
    t = cfg['type']
    assert t in ('BN3d', 'BN', 'SyncBN', 'BN2d', 'BN1d', 'LN')
    if t == 'LN':
        return 'ln' + str(postfix), nn.LayerNorm(num_features)
    layer = {'BN3d': nn.BatchNorm3d, 'SyncBN': nn.BatchNorm3d, 'BN': nn.BatchNorm2d,
             'BN2d': nn.BatchNorm2d, 'BN1d': nn.BatchNorm1d}[t](num_features)
    return 'bn' + str(postfix), layer


def _build_conv_layer(cfg, *args, **kwargs):
    cfg = dict(cfg or dict(type='Conv2d'))
    t = cfg.pop('type')
    layer = {'Conv2d': nn.Conv2d, 'Conv3d': nn.Conv3d, 'Conv1d': nn.Conv1d,
             'deconv3d': nn.ConvTranspose3d}[t]
    return layer(*args, **kwargs, **cfg)


class _ConvModule(nn.Module):
    """mmcv-full 1.6.0 ConvModule defaults: order conv->norm->act, act_cfg=ReLU,
    bias='auto' (= no norm).  Third-party semantics, parity unpinned."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                 groups=1, bias='auto', conv_cfg=None, norm_cfg=None,
                 act_cfg=dict(type='ReLU'), inplace=True, **kw):
        super().__init__()
        if bias == 'auto':
            bias = norm_cfg is None
        self.conv = _build_conv_layer(conv_cfg, in_channels, out_channels, kernel_size,
                                      stride=stride, padding=padding, dilation=dilation,
                                      groups=groups, bias=bias)
        self.with_norm = norm_cfg is not None
        if self.with_norm:
            _, self.bn = _build_norm_layer(norm_cfg, out_channels)
        self.with_act = act_cfg is not None
        if self.with_act:
            assert act_cfg['type'] == 'ReLU'
            self.activate = nn.ReLU(inplace=act_cfg.get('inplace', inplace))

    def forward(self, x):
        x = self.conv(x)
        if self.with_norm:
            x = self.bn(x)
        if self.with_act:
            x = self.activate(x)
        return x


def _identity_deco(*a, **k):
    if len(a) == 1 and callable(a[0]) and not k:
        return a[0]
    return lambda f: f


class _NativeStubs:
    """Bind the reference's three CUDA-only extensions to the C oracle."""

    @staticmethod
    def bev_pool_v2_forward(depth, feat, out, ranks_depth, ranks_feat, ranks_bev,
                            interval_lengths, interval_starts):
        o = out.numpy()
        O.bev_pool_v2_forward(depth.numpy(), feat.numpy(), o, ranks_depth.numpy(),
                              ranks_feat.numpy(), ranks_bev.numpy(), interval_lengths.numpy(),
                              interval_starts.numpy())

    @staticmethod
    def bev_pool_v2_backward(out_grad, depth_grad, feat_grad, depth, feat, ranks_depth,
                             ranks_feat, ranks_bev, interval_lengths, interval_starts):
        import ctypes
        c = feat.shape[-1]
        O.lib().pwo_bev_pool_v2_backward(
            c, len(interval_lengths), O._p(out_grad.numpy()), O._p(depth.numpy()),
            O._p(feat.numpy()), O._p(ranks_depth.numpy(), O.c_i32p),
            O._p(ranks_feat.numpy(), O.c_i32p), O._p(ranks_bev.numpy(), O.c_i32p),
            O._p(interval_starts.numpy(), O.c_i32p), O._p(interval_lengths.numpy(), O.c_i32p),
            O._p(depth_grad.numpy()), O._p(feat_grad.numpy()))

    @staticmethod
    def raw2alpha(density, shift, interval):
        e, a = O.raw2alpha(density.detach().numpy(), float(shift), float(interval))
        return torch.from_numpy(e), torch.from_numpy(a)

    @staticmethod
    def raw2alpha_backward(exp, grad_back, interval):
        return torch.from_numpy(O.raw2alpha_backward(exp.numpy(), grad_back.numpy(), float(interval)))

    @staticmethod
    def alpha2weight(alpha, ray_id, n_rays):
        return tuple(torch.from_numpy(x) for x in
                     O.alpha2weight(alpha.detach().numpy(), ray_id.numpy(), int(n_rays)))

    @staticmethod
    def alpha2weight_backward(alpha, weight, T, last, i_s, i_e, n_rays, gw, gl):
        return torch.from_numpy(O.alpha2weight_backward(
            alpha.detach().numpy(), weight.numpy(), T.numpy(), last.numpy(), i_s.numpy(),
            i_e.numpy(), int(n_rays), gw.contiguous().numpy(), gl.contiguous().numpy()))

    @staticmethod
    def cumdist_thres(dist, thres):
        return torch.from_numpy(O.cumdist_thres(dist.numpy(), float(thres)))


def _segment_coo(src, index, out, reduce='sum'):
    assert reduce == 'sum'
    return out.index_add_(0, index, src)


_REG = _Registry()


def _build_from_cfg(cfg):
    """what mmdet3d.models.builder.build_{backbone,neck,head} do for the reference classes the shim has loaded"""
    if cfg is None:
        return None
    cfg = dict(cfg)
    return _REG.d[cfg.pop('type')](**cfg)


def install_shim():
    reg = _REG
    _mod('mmcv')
    _mod('mmcv.cnn', build_conv_layer=_build_conv_layer, build_norm_layer=_build_norm_layer,
         build_upsample_layer=None, ConvModule=_ConvModule, MODELS=reg)
    _mod('mmcv.cnn.bricks')
    _mod('mmcv.cnn.bricks.conv_module', ConvModule=_ConvModule)
    _mod('mmcv.runner', BaseModule=nn.Module, force_fp32=_identity_deco, auto_fp16=_identity_deco)
    _mod('mmcv.utils', Registry=_Registry)
    _mod('mmdet')
    _mod('mmdet.models', NECKS=reg, HEADS=reg, BACKBONES=reg, DETECTORS=reg)
    _mod('mmdet.models.builder', build_loss=lambda cfg: None)
    _mod('mmdet.models.backbones')
    _mod('mmdet.models.backbones.resnet', BasicBlock=nn.Module, Bottleneck=nn.Module,
         ResNet=nn.Module)
    _mod('mmdet.core', reduce_mean=lambda x: x)
    _mod('torch_scatter', segment_coo=_segment_coo)
    _mod('torch_efficient_distloss', flatten_eff_distloss=None)
    _mod('cv2')
    _mod('termcolor', colored=lambda s, *a, **k: s)
    _mod('mmdet3d')
    bld = _mod('mmdet3d.models.builder', NECKS=reg, HEADS=reg, BACKBONES=reg, DETECTORS=reg, build_backbone=_build_from_cfg,
               build_neck=_build_from_cfg, build_head=_build_from_cfg, build_loss=lambda cfg: None)
    _mod('mmdet3d.models', builder=bld)
    _mod('mmdet3d.models.necks')
    _mod('mmdet3d.models.backbones')
    _mod('mmdet3d.models.heads')
    _mod('mmdet3d.models.nerf')
    _mod('mmdet3d.ops')
    _mod('mmdet3d.ops.bev_pool_v2', bev_pool_v2_ext=_NativeStubs)


def load_ref(modname, relpath):
    spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
    m = importlib.util.module_from_spec(spec)
    sys.modules[modname] = m
    spec.loader.exec_module(m)
    return m


def randomize_bn(module, gen):
    for m in module.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=gen) + 0.5)


def sd_np(module, prefix=''):
    return {prefix + k: v.detach().numpy().copy() for k, v in module.state_dict().items()
            if 'num_batches_tracked' not in k}


def save(name, **arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrays)
    print('wrote', path, '%.1f KB' % (os.path.getsize(path) / 1024))


# ----------------------------------------------------------------------------- generators
def gen_kat(bp):
    """G1: the reference's own known-answer test, run through its Python wrapper on CPU."""
    depth = torch.tensor([0.3, 0.4, 0.2, 0.1, 0.7, 0.6, 0.8, 0.9]).view(1, 1, 2, 2, 2).requires_grad_()
    feat = torch.ones(1, 1, 2, 2, 2, requires_grad=True)
    rd = torch.tensor([0, 4, 1, 6]).int()
    rf = torch.tensor([0, 0, 1, 2]).int()
    rb = torch.tensor([0, 0, 1, 1]).int()
    kept = torch.ones(4, dtype=torch.bool)
    kept[1:] = rb[1:] != rb[:-1]
    st = torch.where(kept)[0].int()
    ln = torch.zeros_like(st)
    ln[:-1] = st[1:] - st[:-1]
    ln[-1] = 4 - st[-1]
    out = bp.bev_pool_v2(depth, feat, rd, rf, rb, (1, 1, 2, 2, 2), st, ln)
    loss = out.sum()
    loss.backward()
    # expected values as asserted by the reference (bev_pool.py:169-176)
    assert abs(loss.item() - 4.4) < 1e-6
    exp_dg = np.array([2., 2., 0., 0., 2., 0., 2., 0.], np.float32).reshape(1, 1, 2, 2, 2)
    exp_fg = np.array([1.0, 1.0, 0.4, 0.4, 0.8, 0.8, 0., 0.], np.float32).reshape(1, 1, 2, 2, 2)
    assert np.allclose(depth.grad.numpy(), exp_dg) and np.allclose(feat.grad.numpy(), exp_fg)
    save('kat_bev_pool_v2.npz', depth=depth.detach().numpy(), feat=feat.detach().numpy(),
         ranks_depth=rd.numpy(), ranks_feat=rf.numpy(), ranks_bev=rb.numpy(),
         interval_starts=st.numpy(), interval_lengths=ln.numpy(), out=out.detach().numpy(),
         loss=np.float32(4.4), depth_grad=exp_dg, feat_grad=exp_fg)


def make_vt(vtm, grid_config, input_size, downsample, C):
    vt = vtm.LSSViewTransformer(grid_config=grid_config, input_size=input_size,
                                downsample=downsample, in_channels=8, out_channels=C,
                                collapse_z=False)
    return vt


def gen_geometry(vtm):
    """G2/G3: geometry + ranks + pooling through the reference's LSSViewTransformer."""
    g = torch.Generator().manual_seed(0)
    # reduced config, full tensors (2 cams, D=8, 4x11 feature map, 20x20x4 grid, C=8)
    grid_small = {'x': [-40, 40, 4.0], 'y': [-40, 40, 4.0], 'z': [-1, 5.4, 1.6],
                  'depth': [1.0, 45.0, 5.5]}
    rig = S.synthetic_rig(6)
    sel = [1, 4]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    s2e = t(rig['sensor2ego'][:, sel]); K = t(rig['intrin'][:, sel])
    pr = t(rig['post_rot'][:, sel]).clone(); pt = t(rig['post_tran'][:, sel]).clone()
    pr[:, :, 0, 0] = 0.25; pr[:, :, 1, 1] = 0.25     # 64x176 input / 1600x900 sensor-ish
    pt[:, :, 1] = -80.0
    bda = torch.tensor([[[0.98, 0.05, 0.0], [-0.05, 0.98, 0.0], [0.0, 0.0, 1.0]]])
    vt = make_vt(vtm, grid_small, (64, 176), 16, 8)
    D = vt.D
    coor = vt.get_lidar_coor(s2e, None, K, pr, pt, bda)
    rb, rd, rf, st, ln = vt.voxel_pooling_prepare_v2(coor)
    depth = torch.softmax(torch.randn(1, 2, D, 4, 11, generator=g), 2)
    feat = torch.randn(1, 2, 8, 4, 11, generator=g)
    depth_g = depth.clone().requires_grad_()
    feat_g = feat.clone().requires_grad_()
    bev = vt.voxel_pooling_v2(coor, depth_g, feat_g)
    gout = torch.randn(bev.shape, generator=g)
    (bev * gout).sum().backward()
    save('lss_small.npz', sensor2ego=s2e.numpy(), intrin=K.numpy(), post_rot=pr.numpy(),
         post_tran=pt.numpy(), bda=bda.numpy(),
         inv_post_rot=torch.inverse(pr).numpy(),
         combine=s2e[:, :, :3, :3].matmul(torch.inverse(K)).numpy(),
         frustum=vt.frustum.numpy(), coor=coor.numpy(),
         ranks_bev=rb.numpy(), ranks_depth=rd.numpy(), ranks_feat=rf.numpy(),
         interval_starts=st.numpy(), interval_lengths=ln.numpy(),
         depth=depth.numpy(), feat=feat.numpy(), bev_feat=bev.detach().numpy(),
         out_grad=gout.numpy(), depth_grad=depth_g.grad.numpy(), feat_grad=feat_g.grad.numpy(),
         grid_x=np.array(grid_small['x']), grid_y=np.array(grid_small['y']),
         grid_z=np.array(grid_small['z']), grid_depth=np.array(grid_small['depth']),
         input_size=np.array([64, 176]), downsample=np.array(16))

    # full-size config: statistics + sampled rows only
    grid_full = {'x': [-40, 40, 0.4], 'y': [-40, 40, 0.4], 'z': [-1, 5.4, 0.4],
                 'depth': [1.0, 45.0, 0.5]}
    vt = make_vt(vtm, grid_full, (512, 1408), 16, 32)
    args = [t(rig[k]) for k in ('sensor2ego', 'intrin', 'post_rot', 'post_tran', 'bda')]
    coor = vt.get_lidar_coor(args[0], None, args[1], args[2], args[3], args[4])
    rb, rd, rf, st, ln = vt.voxel_pooling_prepare_v2(coor)
    coorv = ((coor - vt.grid_lower_bound) / vt.grid_interval)
    n_trunc_not_floor = int(((coorv.long() != coorv.floor().long()).any(-1)
                             & (coorv.long() >= 0).all(-1)
                             & (coorv.long()[..., 0] < 200) & (coorv.long()[..., 1] < 200)
                             & (coorv.long()[..., 2] < 16)).sum())
    depth, feat = [torch.from_numpy(a) for a in S.lift_inputs(5)]
    bev = vt.voxel_pooling_v2(coor, depth, feat)           # (1,32,16,200,200)
    idx = torch.randint(0, 640000, (1024,), generator=g)
    rows = bev[0].reshape(32, -1)[:, idx].T.contiguous()   # (1024, 32)
    # per-voxel multiset signature of the sort (order inside a voxel is unspecified)
    lens_hist = np.bincount(ln.numpy(), minlength=1)
    save('lss_full_stats.npz', P_kept=np.int64(len(rb)), n_intervals=np.int64(len(st)),
         max_len=np.int64(ln.max()), lens_hist=lens_hist,
         sum_ranks_bev=np.int64(rb.long().sum()), sum_ranks_depth=np.int64(rd.long().sum()),
         sum_ranks_feat=np.int64(rf.long().sum()),
         n_trunc_not_floor=np.int64(n_trunc_not_floor),
         coor_sample_idx=idx.numpy(), coor_sample=coor.reshape(-1, 3)[idx * 2].numpy(),
         interval_starts_head=st[:64].numpy(), interval_lengths_head=ln[:64].numpy(),
         ranks_bev_head=rb[:256].numpy(), ranks_bev_tail=rb[-256:].numpy(),
         bev_sum=np.float64(bev.double().sum()), bev_abs_sum=np.float64(bev.double().abs().sum()),
         sample_voxel_idx=idx.numpy(), sample_rows=rows.numpy(), seed_lift=np.int64(5))


def load_sd(module, sd, prefix):
    """Copy the numpy state dict (reference key names) into a reference module."""
    own = module.state_dict()
    for k in own:
        if 'num_batches_tracked' in k:
            continue
        own[k].copy_(torch.from_numpy(sd[prefix + k]))


def gen_conv_stack(res, fpn, occ):
    """G4/G6: CustomResNet3D / LSSFPN3D / final_conv / OccHead at reduced spatial size with
    weights from preworld_amd.synth.synth_state_dict(seed=11) (regenerated by the tests)."""
    sd = S.synth_state_dict(11)
    pre = res.CustomResNet3D(numC_input=32, with_cp=False, num_layer=[1], num_channels=[32],
                             stride=[1], backbone_output_ids=[0]).eval()
    enc = res.CustomResNet3D(numC_input=64, num_layer=[1, 2, 4], with_cp=False,
                             num_channels=[32, 64, 128], stride=[1, 2, 2],
                             backbone_output_ids=[0, 1, 2]).eval()
    neck = fpn.LSSFPN3D(in_channels=224, out_channels=32).eval()
    head = occ.OccHead(with_cp=False, use_deblock=False,
                       norm_cfg=dict(type='SyncBN', requires_grad=True), soft_weights=True,
                       final_occ_size=[200, 200, 16], empty_idx=17, num_level=1,
                       in_channels=[32], out_channel=18,
                       point_cloud_range=[-40, -40, -1, 40, 40, 5.4]).eval()
    fconv = _ConvModule(32, 32, kernel_size=3, stride=1, padding=1, bias=True,
                        conv_cfg=dict(type='Conv3d')).eval()
    with torch.no_grad():
        load_sd(pre, sd, 'pre_process_net.')
        load_sd(enc, sd, 'img_bev_encoder_backbone.')
        load_sd(neck, sd, 'img_bev_encoder_neck.')
        load_sd(head, sd, 'occupancy_head.')
        load_sd(fconv, sd, 'final_conv.')
        Z, Y, X = 8, 16, 16
        rs = np.random.RandomState(12)
        bev_key = torch.from_numpy(rs.standard_normal((1, 32, Z, Y, X)).astype(np.float32))
        bev_adj = torch.from_numpy(rs.standard_normal((1, 32, Z, Y, X)).astype(np.float32))
        pk = pre(bev_key)[0]
        pa = pre(bev_adj)[0]
        feats = enc(torch.cat([pa, pk], 1))
        nk = neck(feats)
        fc = fconv(nk)
        vf = fc.permute(0, 4, 3, 2, 1).contiguous()                 # (1,X,Y,Z,C)
        logits = head([vf[0].permute(3, 0, 1, 2).unsqueeze(0)])['output_voxels'][0]
        occ_pred = logits[0].permute(1, 2, 3, 0).argmax(-1).to(torch.uint8)
    save('conv_stack_small.npz', seed_sd=np.int64(11), seed_in=np.int64(12),
         shape=np.array([Z, Y, X]), pre_key=pk.numpy(), pre_adj=pa.numpy(),
         enc0=feats[0].numpy(), enc1=feats[1].numpy(), enc2=feats[2].numpy(), neck=nk.numpy(),
         final_conv=fc.numpy(), logits=logits.numpy(), occ=occ_pred.numpy())


def gen_forecast():
    """G5: forecast recursion + attribute MLPs: torch modules with the reference's layer
    shapes (preworld_temporal_traj.py:81-132) driven exactly as :329-368 does (the detector
    class itself cannot be imported -- SURVEY 8c)."""
    sd = S.synth_state_dict(11)
    plan = nn.Sequential(nn.Linear(21, 256), nn.ReLU(inplace=True), nn.Linear(256, 256),
                         nn.ReLU(inplace=True), nn.Linear(256, 32))
    fusion = nn.Sequential(nn.Linear(64, 128), nn.Softplus(), nn.Linear(128, 32))
    dens = nn.Sequential(nn.Linear(32, 64), nn.Softplus(), nn.Linear(64, 2), nn.Softplus())
    sem = nn.Sequential(nn.Linear(32, 64), nn.Softplus(), nn.Linear(64, 17))
    col = nn.Sequential(nn.Linear(32, 64), nn.Softplus(), nn.Linear(64, 3))
    with torch.no_grad():
        for name, m in (('plan_head', plan), ('fusion_head', fusion), ('density_mlp', dens),
                        ('semantic_mlp', sem), ('color_mlp', col)):
            load_sd(m, sd, name + '.')
        rs = np.random.RandomState(13)
        v = torch.from_numpy(rs.standard_normal((1, 8, 8, 4, 32)).astype(np.float32))
        ego = torch.from_numpy(S.ego_state(14))
        states = [v]
        x_, y_, z_ = 8, 8, 4
        vf = v
        for _ in range(6):
            es = ego.reshape(1, 21)
            ef = plan(es).unsqueeze(1).unsqueeze(1).unsqueeze(1)
            ef = ef.repeat_interleave(z_, dim=3).repeat_interleave(y_, dim=2).repeat_interleave(x_, dim=1)
            fused = fusion(torch.cat([vf, ef], dim=-1)) + vf
            states.append(fused)
            vf = fused.clone()
        d = dens(v)
        s = sem(v)
        c = col(v)
        ego_feat = plan(ego.reshape(1, 21))
    save('forecast_small.npz', seed_sd=np.int64(11), seed_v=np.int64(13), seed_ego=np.int64(14),
         ego_feat=ego_feat.numpy(), states=np.stack([s_.numpy() for s_ in states]),
         density=d.numpy(), semantic=s.numpy(), color=c.numpy())


def gen_traj(occ):
    """G9 (A20): trajectory branch -- the reference's DownScaleModule3DCustom
    (occupancy_head.py:180-200) imported as is; ego_fusion_head / traj_head are nn.Sequential
    stacks with the reference's shapes (preworld_temporal_traj.py:136-150), driven as :457-470."""
    sd = S.synth_state_dict(11)
    down = occ.DownScaleModule3DCustom(in_dim=32)
    efh = nn.Sequential(nn.Linear(160, 256), nn.Softplus(), nn.Linear(256, 128), nn.Softplus(),
                        nn.Linear(128, 64), nn.Softplus(), nn.Linear(64, 32))
    th = nn.Sequential(nn.Linear(32, 64), nn.Softplus(), nn.Linear(64, 2))
    plan = nn.Sequential(nn.Linear(21, 256), nn.ReLU(inplace=True), nn.Linear(256, 256),
                         nn.ReLU(inplace=True), nn.Linear(256, 32))
    with torch.no_grad():
        load_sd(down, sd, 'downscale.')
        load_sd(efh, sd, 'ego_fusion_head.')
        load_sd(th, sd, 'traj_head.')
        load_sd(plan, sd, 'plan_head.')
        rs = np.random.RandomState(15)
        fused = torch.from_numpy(rs.standard_normal((1, 16, 16, 8, 32)).astype(np.float32))   # (B,X,Y,Z,C)
        ego = torch.from_numpy(S.ego_state(14))
        identity = plan(ego.reshape(1, 21))
        d = down(fused).squeeze(1).squeeze(1).squeeze(1)
        res_ego = efh(torch.cat([identity, d], dim=-1))
        fused_ego = identity + res_ego
        traj = th(fused_ego)
    save('traj_small.npz', seed_sd=np.int64(11), seed_v=np.int64(15), seed_ego=np.int64(14),
         identity=identity.numpy(), down=d.numpy(), fused_ego=fused_ego.numpy(), traj=traj.numpy())


def gen_rays():
    """G10: mmdet3d/datasets/ray.py generate_rays -- the table with use_wrs=False
    and the WRS weights captured from the sampler the reference constructs (ray.py:116)."""
    ray = load_ref('ref_ray', 'mmdet3d/datasets/ray.py')
    coors, depths, segs, imgs, c2ws, Ks = [[torch.from_numpy(a) for a in l] for l in S.ray_label_inputs(31)]
    time_ids = {0: [0, 1], 1: [2, 3]}
    dyn = torch.tensor([0, 1, 3, 4, 5, 7, 9, 10])
    table = ray.generate_rays(coors, depths, segs, imgs, c2ws, Ks, max_ray_nums=0, time_ids=time_ids,
                              dynamic_class=dyn, use_wrs=False)
    captured = {}

    class Capture:
        def __init__(self, weights, num_samples, replacement):
            captured['w'] = weights.clone()
            self.n = num_samples

        def __iter__(self):
            return iter(range(self.n))
    ray.WeightedRandomSampler = Capture
    ray.generate_rays(coors, depths, segs, imgs, c2ws, Ks, max_ray_nums=100, time_ids=time_ids,
                      dynamic_class=dyn, balance_weight=None, weight_adj=0.3, weight_dyn=0.0, use_wrs=True)
    w_batch = captured['w'].numpy()
    bw = torch.exp(0.005 * (torch.arange(1, 18).float().max() / torch.arange(1, 18).float() - 1))
    ray.generate_rays(coors, depths, segs, imgs, c2ws, Ks, max_ray_nums=100, time_ids=time_ids,
                      dynamic_class=dyn, balance_weight=bw, weight_adj=0.25, weight_dyn=0.1, use_wrs=True)
    save('rays_small.npz', seed=np.int64(31), table=table.numpy(), weights_batch=w_batch,
         balance_weight=bw.numpy(), weights_given=captured['w'].numpy())


def gen_ray_labels():
    """Stage B of the ray supervision ("Ray supervision from the sweep"): the reference's OWN get_rays
    (mmdet3d/datasets/nuscenes_dataset_occ.py:197-270 with its load_depth / load_seg_label / load_img / get_sensor_transforms and
    ray.py's generate_rays) run on the .bin files that tests/_ray_labels_np.py's stage A writes for a synthetic two-frame,
    two-camera sample -- the dataset module is loaded under the shim (pyquaternion's Quaternion and torchvision's ToTensor /
    Normalize are stood in for: transforms.quaternion_rotation_matrix, and permute + (x - mean) / std in float32; load_img's
    array conversion is respelled for NumPy 2), get_rays is
    called unbound on a plain object carrying the attributes it reads.  The frames go through lossless PNG files.  The sampler
    weights are captured as gen_rays does."""
    import tempfile
    from PIL import Image
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import _ray_labels_np as RN
    from preworld_amd import transforms as TF

    class Quaternion:
        def __init__(self, *q):
            self.rotation_matrix = TF.quaternion_rotation_matrix(q[0] if len(q) == 1 else q)
    _mod('pyquaternion', Quaternion=Quaternion)
    _mod('tqdm', tqdm=lambda x, *a, **k: x)
    _mod('PIL', Image=Image) if 'PIL' not in sys.modules else None
    mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
    tvt = _mod('torchvision.transforms', Compose=None, ToTensor=None, Normalize=None)
    _mod('torchvision', transforms=tvt)
    _mod('mmdet3d.datasets')
    _mod('mmdet3d.datasets.builder', DATASETS=_REG)
    _mod('mmdet3d.datasets.nuscenes_dataset', NuScenesDataset=object)
    _mod('mmdet3d.datasets.occ_metrics', Metric_mIoU=None, Metric_FScore=None)
    ray = load_ref('mmdet3d.datasets.ray', 'mmdet3d/datasets/ray.py')
    ds = load_ref('mmdet3d.datasets.nuscenes_dataset_occ', 'mmdet3d/datasets/nuscenes_dataset_occ.py')

    seed, T, N, P, H, W, focal = 41, 2, 2, 3001, 48, 80, 40.0
    S_ = RN.synthetic_sample(seed, T=T, N=N, P=P, H=H, W=W, focal=focal)
    depth_lists, seg_lists = RN.stage_a(S_['points'], S_['labels'], RN.LUT, S_['poses'], N, H, W)
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'depth'))
        os.makedirs(os.path.join(tmp, 'seg'))
        for t, info in enumerate(S_['infos']):
            for c, name in enumerate(S_['cam_names']):
                v = t * N + c
                path = os.path.join(tmp, 'frame_%d.png' % v)
                Image.fromarray(S_['frames'][v], 'RGB').save(path)
                info['cams'][name]['data_path'] = path
                depth_lists[v].flatten().tofile(os.path.join(tmp, 'depth', 'frame_%d.png.bin' % v))
                seg_lists[v].flatten().tofile(os.path.join(tmp, 'seg', 'frame_%d.png.bin' % v))
        real_load_seg = ds.load_seg_label
        ds.load_seg_label = lambda path, gt, img_size=[H, W], mode='lidarseg': real_load_seg(path, gt, img_size=img_size, mode=mode)
        # the reference's load_img asks numpy for a conversion without a copy, which NumPy 2 refuses (1.x, which the reference
        # stack runs, copies silently); stood in for by the same behaviour: the decoded RGB frame as float32, divided by 255 in
        # float32
        ds.load_img = lambda path: np.asarray(Image.open(path).convert('RGB'), dtype=np.float32) / 255.0
        recorded = {}
        real_generate = ds.generate_rays

        def recording_generate(*a, **k):
            recorded['args'], recorded['kw'] = a, k
            return real_generate(*a, **k)
        ds.generate_rays = recording_generate

        class Self:
            data_infos = S_['infos']
            aux_frames = [1]
            semantic_gt_path = os.path.join(tmp, 'seg')
            depth_gt_path = os.path.join(tmp, 'depth')
            max_ray_nums = 0
            WRS_balance_weight = None
            dynamic_class = torch.tensor(ds.dynamic_class)
            normalize_rgb = staticmethod(lambda img: (torch.from_numpy(img).permute(2, 0, 1).contiguous() - mean[:, None, None]) / std[:, None, None])
        table = ds.NuScenesDatasetOccpancy.get_rays(Self(), 0)
    coors, depths, segs, imgs, c2w, Ks = recorded['args'][:6]
    time_ids, dyn = recorded['kw']['time_ids'], recorded['kw']['dynamic_class']
    captured = {}

    class Capture:
        def __init__(self, weights, num_samples, replacement):
            captured['w'] = weights.clone()
            self.n = num_samples

        def __iter__(self):
            return iter(range(self.n))
    ray.WeightedRandomSampler = Capture
    ray.generate_rays(coors, depths, segs, imgs, c2w, Ks, max_ray_nums=100, time_ids=time_ids, dynamic_class=dyn,
                      balance_weight=None, weight_adj=0.3, weight_dyn=0.0, use_wrs=True)
    w_batch = captured['w'].numpy()
    bw = torch.exp(0.005 * (torch.arange(1, 18).float().max() / torch.arange(1, 18).float() - 1))
    ray.generate_rays(coors, depths, segs, imgs, c2w, Ks, max_ray_nums=100, time_ids=time_ids, dynamic_class=dyn,
                      balance_weight=bw, weight_adj=0.25, weight_dyn=0.1, use_wrs=True)
    assert {int(k): list(v) for k, v in time_ids.items()} == {0: [0, 1], 1: [2, 3]}
    save('ray_labels_small.npz', seed=np.int64(seed), shape=np.array([T, N, P, H, W], np.int64), focal=np.float64(focal),
         depth_list=np.concatenate(depth_lists), seg_list=np.concatenate(seg_lists), view_off=RN.offsets(depth_lists),
         frames=S_['frames'], c2w=c2w.numpy(), K=torch.stack(Ks).numpy(), dynamic_class=dyn.numpy().astype(np.int32),
         table=table.numpy(), weights_batch=w_batch, balance_weight=bw.numpy(), weights_given=captured['w'].numpy(),
         weight_adj_dyn=np.array([0.25, 0.1]))


def gen_stereo(vtm):
    """G12: DepthNet.gen_grid + calculate_cost_volumn (view_transformer.py:546-604)
    called as plain functions (the DepthNet constructor needs mmcv; the two methods only read self.bias)."""
    prev, curr, k2s, K, pr, pt, frustum = [torch.from_numpy(a) for a in S.stereo_inputs(51)]
    outs = {}
    for bias in (0.0, 5.0):
        me = types.SimpleNamespace(bias=bias)
        me.gen_grid = lambda *a, **k: vtm.DepthNet.gen_grid(me, *a, **k)
        metas = dict(k2s_sensor=k2s, intrins=K, post_rots=pr, post_trans=pt, frustum=frustum,
                     cv_feat_list=[prev, curr])
        with torch.no_grad():
            outs['cv_bias%d' % int(bias)] = vtm.DepthNet.calculate_cost_volumn(me, metas).numpy()
    save('stereo_small.npz', seed=np.int64(51), **outs)


def gen_losses():
    """G11: mmdet3d/models/detectors/loss.py CE_ssc_loss / sem_scal_loss /
    geo_scal_loss values and their autograd gradients w.r.t. the logits."""
    ls = load_ref('ref_loss', 'mmdet3d/models/detectors/loss.py')
    pred_np, target_np, cam_np = S.voxel_loss_inputs(41)
    cw = torch.cat([torch.from_numpy(1 / np.log(np.array([1163161, 2309034, 188743, 2997643, 20317180, 852476,
                    243808, 2457947, 497017, 2731022, 7224789, 214411435, 5565043, 63191967, 76098082,
                    128860031, 141625221], np.float64) + 0.001)).float(), torch.tensor([0.])])
    out = {}
    for tag, cam in (('cam', torch.from_numpy(cam_np)), ('nocam', None)):
        pred = torch.from_numpy(pred_np).clone().requires_grad_()
        target = torch.from_numpy(target_np)
        ce = ls.CE_ssc_loss(pred, target, cw, 255)
        sem = ls.sem_scal_loss(pred, target, 255, camera_mask=cam)
        geo = ls.geo_scal_loss(pred, target, 255, non_empty_idx=17, camera_mask=cam)
        total = 1.0 * ce + 0.7 * sem + 1.3 * geo
        total.backward()
        out['ce_' + tag], out['sem_' + tag], out['geo_' + tag] = ce.item(), sem.item(), geo.item()
        out['grad_' + tag] = pred.grad.numpy().copy()
    save('voxel_losses.npz', seed=np.int64(41), class_weights=cw.numpy(), **{k: np.asarray(v) for k, v in out.items()})


def gen_losses2():
    """G11b (the finetune configs' other two voxel losses): CustomFocalLoss
    (mmdet3d/models/loss_utils/focal_loss.py:163-262, CPU branch = py_sigmoid_focal_loss) on a (1,18,200,200,2) grid
    (the class hard-codes the 200x200 radial map) -- loss value + every 97th gradient element -- and lovasz_softmax
    (mmdet3d/models/detectors/lovasz_softmax.py:157-232) on the small voxel-loss inputs with full gradients."""
    _mod('mmcv.ops', sigmoid_focal_loss=None)
    _mod('mmdet.models.losses')
    _mod('mmdet.models.losses.utils', weight_reduce_loss=None)
    sys.modules['mmdet.models.builder'].LOSSES = _Registry()
    fl = load_ref('ref_focal', 'mmdet3d/models/loss_utils/focal_loss.py')
    lv = load_ref('ref_lovasz', 'mmdet3d/models/detectors/lovasz_softmax.py')
    cw = torch.from_numpy(np.load(os.path.join(OUT, 'voxel_losses.npz'))['class_weights'])
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self          # CustomFocalLoss.__init__ moves its map to the GPU
    try:
        focal = fl.CustomFocalLoss()
    finally:
        torch.Tensor.cuda = real_cuda
    out = {}
    pred_np, target_np, cam_np = S.voxel_loss_inputs(43, shape=(1, 18, 200, 200, 2))
    for tag, cam in (('cam', torch.from_numpy(cam_np)), ('nocam', None)):
        pred = torch.from_numpy(pred_np).clone().requires_grad_()
        loss = focal(pred, torch.from_numpy(target_np), cw, 255, camera_mask=cam)
        loss.backward()
        out['focal_' + tag] = loss.item()
        out['focal_grad_' + tag] = pred.grad.numpy().reshape(-1)[::97].copy()
    pred_np, target_np, cam_np = S.voxel_loss_inputs(41)
    for tag, cam in (('cam', torch.from_numpy(cam_np)), ('nocam', None)):
        pred = torch.from_numpy(pred_np).clone().requires_grad_()
        loss = lv.lovasz_softmax(torch.softmax(pred, dim=1), torch.from_numpy(target_np), ignore=17, camera_mask=cam)
        loss.backward()
        out['lovasz_' + tag] = loss.item()
        out['lovasz_grad_' + tag] = pred.grad.numpy().copy()
    save('voxel_losses2.npz', seed_focal=np.int64(43), seed_lovasz=np.int64(41), **{k: np.asarray(v) for k, v in out.items()})


class _RefBasicBlock(nn.Module):
    """mmdet 2.24 ResNet BasicBlock (third-party, absent here) for the reference DepthNet: conv1/bn1/conv2/bn2/downsample."""

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, **kw):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        out = self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x)))))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class _RefBaseModule(nn.Module):
    def __init__(self, init_cfg=None):
        super().__init__()


class _RefFFN(nn.Module):
    """mmcv-full 1.6.0 FFN (third-party, absent here), num_fcs=2, add_identity=True."""

    def __init__(self, embed_dims, feedforward_channels, num_fcs=2, ffn_drop=0., dropout_layer=None, act_cfg=None,
                 add_identity=True, init_cfg=None):
        super().__init__()
        self.layers = nn.Sequential(nn.Sequential(nn.Linear(embed_dims, feedforward_channels), nn.GELU(), nn.Dropout(ffn_drop)),
                                    nn.Linear(feedforward_channels, embed_dims), nn.Dropout(ffn_drop))

    def forward(self, x, identity=None):
        return (x if identity is None else identity) + self.layers(x)


def gen_image_branch(vtm, fpn):
    """G12: the reference SwinTransformer (backbones/swin.py), FPN_LSS (necks/lss_fpn.py) and DepthNet
    (necks/view_transformer.py) at reduced sizes with seeded weights (synth.seeded_module_state) -> outputs only."""
    _mod('mmcv.cnn.bricks.transformer', FFN=_RefFFN, build_dropout=lambda cfg: nn.Identity())
    _mod('mmcv.cnn.utils')
    _mod('mmcv.cnn.utils.weight_init', constant_init=None)
    _mod('mmcv.cnn.bricks.registry', ATTENTION=_Registry())
    _mod('mmcv.runner.base_module', BaseModule=_RefBaseModule, ModuleList=nn.ModuleList)
    sys.modules['mmcv.runner']._load_checkpoint = None
    sys.modules['mmcv.cnn'].trunc_normal_init = None
    _mod('mmseg'); _mod('mmseg.ops', resize=None)
    _mod('mmdet3d.utils', get_root_logger=None)
    sys.modules['mmdet3d.models.builder'].BACKBONES = sys.modules['mmdet3d.models.builder'].NECKS
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sw = load_ref('mmdet3d.models.backbones.swin', 'mmdet3d/models/backbones/swin.py')
        cfg = S.small_swin_cfg()
        net = sw.SwinTransformer(**cfg, with_cp=False)
        net.eval()                      # the reference's train() override returns None
    net.load_state_dict(S.seeded_module_state(net, 51), strict=False)
    x = torch.from_numpy(np.random.RandomState(52).standard_normal((2, 3, 64, 96)).astype(np.float32))
    with torch.no_grad():
        outs = net(x)
        # extract_stereo_ref_feat's Swin branch (bevdet.py:589-603)
        t = net.drop_after_pos(net.patch_embed(x))
        _, _, o0, hw0 = net.stages[0](t, (net.patch_embed.DH, net.patch_embed.DW))
        ref0 = o0.view(-1, *hw0, net.num_features[0]).permute(0, 3, 1, 2).contiguous()
    neck = fpn.FPN_LSS(in_channels=64 + 128, out_channels=24, extra_upsample=None, input_feature_index=(0, 1), scale_factor=2).eval()
    neck.load_state_dict(S.seeded_module_state(neck, 53))
    with torch.no_grad():
        nout = neck(outs[1:])
    vtm.BasicBlock = _RefBasicBlock
    dn = vtm.DepthNet(16, 16, 4, 12, use_dcn=False, aspp_mid_channels=8, stereo=True, bias=5.0).eval()
    dn.load_state_dict(S.seeded_module_state(dn, 54))
    st = dict(zip(('prev', 'curr', 'k2s_sensor', 'intrins', 'post_rots', 'post_trans', 'frustum'),
                  S.stereo_inputs(55, C=8, H=8, W=12, D=12, n_cams=2)))
    rs = np.random.RandomState(56)
    xin = torch.from_numpy(rs.standard_normal((2, 16, 2, 3)).astype(np.float32))
    mlp = torch.from_numpy(rs.standard_normal((1, 2, 27)).astype(np.float32))
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    metas = dict(k2s_sensor=T(st['k2s_sensor']), intrins=T(st['intrins']), post_rots=T(st['post_rots']),
                 post_trans=T(st['post_trans']), frustum=T(st['frustum']), cv_downsample=4, downsample=16,
                 cv_feat_list=[T(st['prev']), T(st['curr'])])
    with torch.no_grad():
        d_st = dn(xin, mlp, metas)
        metas['cv_feat_list'] = [None, T(st['curr'])]
        d_no = dn(xin, mlp, metas)
    save('image_branch_small.npz', swin_stereo=outs[0].numpy(), swin_s2=outs[1].numpy(), swin_s3=outs[2].numpy(),
         swin_ref0=ref0.numpy(), neck=nout.numpy(), depthnet_stereo=d_st.numpy(), depthnet_nostereo=d_no.numpy(),
         swin_keys=np.array(sorted(net.state_dict().keys())), neck_keys=np.array(sorted(neck.state_dict().keys())),
         depthnet_keys=np.array(sorted(dn.state_dict().keys())))


def gen_render(nh):
    """G7: NerfHead.sample_ray / render_one_scene / render_* through the reference Python."""
    head = nh.NerfHead(point_cloud_range=[-40, -40, -1, 40, 40, 5.4], voxel_size=0.4,
                       scene_center=[0, 0, 2.2], radius=39, use_depth_sup=True,
                       weight_depth=1.0, weight_semantic=1.0, weight_color=1.0)
    density, semantic, color = [torch.from_numpy(a) for a in S.render_grids(21)]
    R = 64
    o, d = [torch.from_numpy(a) for a in S.rays(22, R)]
    bda = torch.tensor([[0.98, 0.05, 0.0], [-0.05, 0.98, 0.0], [0.0, 0.0, 1.0]])
    with torch.no_grad():
        pts, inner, t = nh.sample_ray(o, d, head.step_size, head.scene_center, head.scene_radius,
                                      head.bg_len, head.world_len, bda)
        res = head.render_one_scene(o, d, bda, density, semantic, color, mask=None)
        res['N_ray'] = R
        depth = head.render_depth(res)
        sem = head.render_semantic(res)
        col = head.render_color(res)
    save('render_small.npz', seed_grid=np.int64(21), seed_rays=np.int64(22), R=np.int64(R),
         bda=bda.numpy(), t=t.numpy(), ray_pts=pts.numpy()[:, ::8].copy(),
         inner_mask=inner.numpy(),
         weights=res['weights'].numpy(), ray_id=res['ray_id'].numpy(), s=res['s'].numpy(),
         alphainv_last=res['alphainv_last'].numpy(), render_depth=depth.numpy(),
         render_semantic=sem.numpy(), render_color=col.numpy(),
         xyz_min=head.xyz_min.numpy(), xyz_max=head.xyz_max.numpy(),
         act_shift=head.act_shift.numpy(), bg_len=np.float32(head.bg_len),
         scene_center=head.scene_center.numpy())


def gen_render_grad(nh):
    """Gradients of the render head w.r.t. the density / semantic / color grids: the imported reference NerfHead under torch
    autograd (grid_sample backward, Raw2Alpha / Alphas2Weights backward through the bound C restatements) against the
    differentiable checker oracle/torch_render.py, same inputs; the fixture keeps the reference's gradients at sampled
    voxels plus their sums."""
    from oracle import torch_render as TR
    head = nh.NerfHead(point_cloud_range=[-40, -40, -1, 40, 40, 5.4], voxel_size=0.4, scene_center=[0, 0, 2.2], radius=39,
                       use_depth_sup=True, weight_depth=1.0, weight_semantic=1.0, weight_color=1.0)
    R, S_ = 48, 417
    density, semantic, color = [torch.from_numpy(a).requires_grad_() for a in S.render_grids(23)]
    o_np, d_np = S.rays(24, R)
    bda_np = np.array([[0.98, 0.05, 0.0], [-0.05, 0.98, 0.0], [0.0, 0.0, 1.0]], np.float32)
    coef = TR.objective_coefficients(25, R, S_)
    res = head.render_one_scene(torch.from_numpy(o_np), torch.from_numpy(d_np), torch.from_numpy(bda_np), density, semantic,
                                color, mask=None)
    res['N_ray'] = R
    # dense (R, S) weights need the step ids, which render_one_scene does not return: recover them from t (strictly
    # increasing sample table) -- pure indexing, no arithmetic on the reference's values
    t_tab = torch.from_numpy(O.NerfConsts().t_table())
    step_id = torch.searchsorted(t_tab, res['t'])
    out = dict(depth=head.render_depth(res), semantic=head.render_semantic(res), color=head.render_color(res),
               alphainv_last=res['alphainv_last'],
               weights=torch.zeros(R, S_).index_put((res['ray_id'], step_id), res['weights']))
    TR.scalar_objective(out, coef).backward()
    ref = [density.grad.clone(), semantic.grad.clone(), color.grad.clone()]
    d2, s2, c2 = [torch.from_numpy(a).requires_grad_() for a in S.render_grids(23)]
    out2 = TR.render(o_np, d_np, bda_np, d2, s2, c2)
    for k in out:
        np.testing.assert_allclose(out2[k].detach().numpy(), out[k].detach().numpy(), rtol=1e-6, atol=1e-7, err_msg=k)
    TR.scalar_objective(out2, coef).backward()
    for a, b, name in zip(ref, (d2.grad, s2.grad, c2.grad), ('density', 'semantic', 'color')):
        np.testing.assert_allclose(b.numpy(), a.numpy(), rtol=1e-5, atol=1e-7, err_msg=name)
    rng = np.random.RandomState(26)
    nz = torch.nonzero(ref[0].abs() > 0).numpy()
    pick = nz[rng.choice(len(nz), 4096, replace=False)]
    ix = tuple(torch.from_numpy(pick[:, i]) for i in range(3))
    save('render_grad_small.npz', seed_grid=np.int64(23), seed_rays=np.int64(24), seed_coef=np.int64(25), R=np.int64(R),
         bda=bda_np, voxels=pick.astype(np.int32), g_density=ref[0][ix].numpy(), g_semantic=ref[1][ix].numpy(),
         g_color=ref[2][ix].numpy(), sum_density=np.float64(ref[0].double().sum()), sum_semantic=ref[1].double().sum((0, 1, 2)).numpy(),
         sum_color=ref[2].double().sum((0, 1, 2)).numpy(), abs_density=np.float64(ref[0].double().abs().sum()),
         n_nonzero=np.int64(len(nz)), depth=out['depth'].detach().numpy(), alphainv_last=out['alphainv_last'].detach().numpy())


def _ref_head(nh):
    return nh.NerfHead(point_cloud_range=[-40, -40, -1, 40, 40, 5.4], voxel_size=0.4, scene_center=[0, 0, 2.2], radius=39,
                       use_depth_sup=True, weight_depth=1.0, weight_semantic=1.0, weight_color=1.0)


def gen_render_mixed(nh):
    """the reference NerfHead on scenes whose rays TERMINATE.  'mixed' = S.render_grids_mixed (ground slab +
    boxes with density ~U(10,22), one density-30 box; of 256 rays ~116 end at T < 1e-3 (render_utils_kernel.cu:591-603 through
    the bound C restatement), ~53 end partly opaque, the rest stay transparent; kept samples per ray 1 .. 209); 'void' =
    density -5 everywhere (every in-grid sample culled by the first compaction, horizontal rays keep NOTHING).  Forward:
    compacted weights with (ray, step) ids, alphainv_last, rendered depth / semantic / colour, kept counts.  Backward: the
    reference's autograd gradients of a seeded scalar objective at sampled voxels + sums, cross-checked here against
    oracle/torch_render.py."""
    from oracle import torch_render as TR
    head = _ref_head(nh)
    bda_np = np.array([[0.98, 0.05, 0.0], [-0.05, 0.98, 0.0], [0.0, 0.0, 1.0]], np.float32)
    t_tab = torch.from_numpy(O.NerfConsts().t_table())
    S_ = int(t_tab.numel())
    out = dict(bda=bda_np)
    for tag, grids_np, (o_np, d_np), seeds in (
            ('mixed', S.render_grids_mixed(61), S.rays_mixed(62, 256), (61, 62, 65)),
            ('void', S.render_grids_void(63), S.rays_void(64, 16), (63, 64, 66))):
        R = len(o_np)
        density, semantic, color = [torch.from_numpy(a).requires_grad_() for a in grids_np]
        res = head.render_one_scene(torch.from_numpy(o_np), torch.from_numpy(d_np), torch.from_numpy(bda_np), density, semantic,
                                    color, mask=None)
        res['N_ray'] = R
        step_id = torch.searchsorted(t_tab, res['t'])
        assert torch.equal(t_tab[step_id], res['t'])
        fw = dict(depth=head.render_depth(res), semantic=head.render_semantic(res), color=head.render_color(res),
                  alphainv_last=res['alphainv_last'],
                  weights=torch.zeros(R, S_).index_put((res['ray_id'], step_id), res['weights']))
        coef = TR.objective_coefficients(seeds[2], R, S_)
        TR.scalar_objective(fw, coef).backward()
        ref = [density.grad.clone(), semantic.grad.clone(), color.grad.clone()]
        # the oracle (C restatement) and the differentiable checker on the same scene
        ores = O.render_one_scene(o_np, d_np, bda_np, *grids_np, O.NerfConsts())
        od, osem, ocol = O.render_outputs(ores, O.NerfConsts())
        np.testing.assert_array_equal(ores['ray_id'], res['ray_id'].numpy())
        np.testing.assert_array_equal(ores['step_id'], step_id.numpy())
        # Conditioning of the opaque regime: at a free / occupied face the density changes by ~20 per voxel, a sample position is
        # known to ~6e-6 voxels in fp32 (|ind_norm| ~ 1 over 100 voxels), so sigma moves by ~1e-4 between two fp32 evaluation
        # orders and every opaque sample multiplies T by (1 + e^(sigma - 13.8))^-0.5: ~5e-5 relative per sample.  Two correct fp32
        # implementations (torch grid_sample vs the C restatement) differ by that much; the GPU tests use the same bound.
        wdiff = np.abs(ores['weights'] - res['weights'].detach().numpy())
        print('  render_%s: oracle vs reference weights: max abs %.2e, max rel (w > 1e-3) %.2e' % (
            tag, wdiff.max() if len(wdiff) else 0, (wdiff / np.maximum(ores['weights'], 1e-3)).max() if len(wdiff) else 0))
        np.testing.assert_allclose(ores['weights'], res['weights'].detach().numpy(), rtol=1e-3, atol=1e-7)
        np.testing.assert_allclose(ores['alphainv_last'], res['alphainv_last'].detach().numpy(), rtol=1e-3, atol=1e-7)
        np.testing.assert_allclose(od, fw['depth'].detach().numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(osem, fw['semantic'].detach().numpy(), rtol=1e-4, atol=5e-5)
        np.testing.assert_allclose(ocol, fw['color'].detach().numpy(), rtol=1e-4, atol=5e-5)
        g2 = [torch.from_numpy(a).requires_grad_() for a in grids_np]
        out2 = TR.render(o_np, d_np, bda_np, *g2)
        for k in fw:
            np.testing.assert_allclose(out2[k].detach().numpy(), fw[k].detach().numpy(), rtol=1e-3, atol=5e-5, err_msg=tag + k)
        TR.scalar_objective(out2, coef).backward()
        for a, b, name in zip(ref, g2, ('density', 'semantic', 'color')):
            np.testing.assert_allclose(b.grad.numpy(), a.numpy(), rtol=1e-3, atol=2e-6 * float(a.abs().max()) + 1e-12,
                                       err_msg=tag + name)
        last = res['alphainv_last'].detach().numpy()
        kept = np.bincount(res['ray_id'].numpy(), minlength=R)
        print('  render_%s: %d rays, %d terminated (T < 1e-3), %d partly opaque, %d transparent; kept samples per ray %d .. %d'
              % (tag, R, int((last < 1e-3).sum()), int(((last >= 1e-3) & (last < 0.99)).sum()), int((last >= 0.99).sum()),
                 kept.min(), kept.max()))
        rng = np.random.RandomState(seeds[2] + 100)
        nz = torch.nonzero(ref[0].abs() > 0).numpy()
        pick = nz[rng.choice(len(nz), min(4096, len(nz)), replace=False)]
        ix = tuple(torch.from_numpy(pick[:, i]) for i in range(3))
        out.update({tag + '_' + k: v for k, v in dict(
            seeds=np.array(seeds, np.int64), R=np.int64(R), weights=res['weights'].detach().numpy(),
            ray_id=res['ray_id'].numpy().astype(np.int32), step_id=step_id.numpy().astype(np.int16), alphainv_last=last,
            kept=kept.astype(np.int32), depth=fw['depth'].detach().numpy(), semantic=fw['semantic'].detach().numpy(),
            color=fw['color'].detach().numpy(), voxels=pick.astype(np.int16), g_density=ref[0][ix].numpy(),
            g_semantic=ref[1][ix].numpy(), g_color=ref[2][ix].numpy(), sum_density=np.float64(ref[0].double().sum()),
            abs_density=np.float64(ref[0].double().abs().sum()), sum_semantic=ref[1].double().sum((0, 1, 2)).numpy(),
            sum_color=ref[2].double().sum((0, 1, 2)).numpy(), abs_semantic=ref[1].double().abs().sum((0, 1, 2)).numpy(),
            abs_color=ref[2].double().abs().sum((0, 1, 2)).numpy(), n_nonzero=np.int64(len(nz))).items()})
    save('render_mixed.npz', **out)


def gen_metric(om):
    """G8: Metric_mIoU on seeded random labels."""
    rng = np.random.RandomState(4)
    m = om.Metric_mIoU(num_classes=18, use_image_mask=True)
    preds, gts, masks = [], [], []
    for _ in range(3):
        gt = rng.randint(0, 18, (200, 200, 16)).astype(np.uint8)
        pred = np.where(rng.rand(200, 200, 16) < 0.6, gt, rng.randint(0, 18, gt.shape)).astype(np.uint8)
        mc = rng.rand(200, 200, 16) < 0.7
        m.add_batch(pred, gt, None, mc)
        preds.append(pred[::8, ::8]); gts.append(gt[::8, ::8]); masks.append(mc[::8, ::8])
    import io, contextlib
    with contextlib.redirect_stdout(io.StringIO()):
        _, iu, cnt, miou = m.count_miou()
    # small-sample version for the committed fixture
    m2 = om.Metric_mIoU(num_classes=18, use_image_mask=True)
    for p, g_, k in zip(preds, gts, masks):
        m2.add_batch(p, g_, None, k)
    with contextlib.redirect_stdout(io.StringIO()):
        _, iu2, _, miou2 = m2.count_miou()
    save('metric_miou.npz', pred=np.stack(preds), gt=np.stack(gts), mask=np.stack(masks),
         hist=m2.hist, iou=iu2, miou=np.float64(miou2))


def _fscore_scene(rng, X=200, Y=200, Z=16):
    """a structured occupancy scene: a ground slab of classes 11-16 under boxes of classes 1-10, the rest free (17); and a
    prediction of it with boxes shifted by one or two voxels, dropped and invented, and noise voxels at exactly sqrt(2) and sqrt(3)
    lattice units from ground-truth voxels (0.566 / 0.693 m at 0.4 m voxels: either side of the default 0.6 m)."""
    gt = np.full((X, Y, Z), 17, np.uint8)
    p = max(4, X // 10)
    cls = rng.randint(11, 17, (-(-X // p), -(-Y // p)))
    gt[:, :, 0] = np.kron(cls, np.ones((p, p), np.int64))[:X, :Y]
    gt[:, :, 1] = np.where(rng.rand(X, Y) < 0.5, gt[:, :, 0], 17)
    boxes = []
    for _ in range(X * Y // 1000):
        sx, sy, sz = rng.randint(2, 9), rng.randint(2, 9), rng.randint(1, max(2, Z // 3))
        x0, y0, z0 = rng.randint(0, X - sx), rng.randint(0, Y - sy), rng.randint(1, 3)
        c = rng.randint(1, 11)
        gt[x0:x0 + sx, y0:y0 + sy, z0:z0 + sz] = c
        boxes.append((x0, y0, z0, sx, sy, sz, c))
    pred = gt.copy()
    for (x0, y0, z0, sx, sy, sz, c) in boxes:
        r = rng.rand()
        if r < 0.4:                                            # shifted by one or two voxels along x, y or z
            pred[x0:x0 + sx, y0:y0 + sy, z0:z0 + sz] = 17
            d = [0, 0, 0]
            d[rng.randint(0, 3)] = rng.choice([-2, -1, 1, 2])
            xa, ya, za = max(0, x0 + d[0]), max(0, y0 + d[1]), max(0, z0 + d[2])
            pred[xa:x0 + sx + d[0], ya:y0 + sy + d[1], za:z0 + sz + d[2]] = c
        elif r < 0.55:                                         # dropped
            pred[x0:x0 + sx, y0:y0 + sy, z0:z0 + sz] = 17
    for _ in range(len(boxes) // 3):                           # invented
        sx, sy, sz = rng.randint(2, 6), rng.randint(2, 6), rng.randint(1, 3)
        x0, y0, z0 = rng.randint(0, X - sx), rng.randint(0, Y - sy), rng.randint(2, Z - sz)
        pred[x0:x0 + sx, y0:y0 + sy, z0:z0 + sz] = rng.randint(1, 11)
    occ = np.argwhere((gt != 17) & (gt != 255))
    for dist2 in (2, 3):                                       # noise at sqrt(2) / sqrt(3) lattice units from a gt voxel
        pick = occ[rng.randint(0, len(occ), X * Y // 6)]
        offs = np.array([o for o in np.ndindex(3, 3, 3) if sum((np.array(o) - 1) ** 2) == dist2]) - 1
        q = pick + offs[rng.randint(0, len(offs), len(pick))]
        q = q[np.all((q >= 0) & (q < (X, Y, Z)), axis=1)]
        q = q[gt[q[:, 0], q[:, 1], q[:, 2]] == 17]
        # keep only noise whose nearest gt voxel is exactly that far: no gt voxel at a smaller lattice distance
        ok = np.ones(len(q), bool)
        for o in np.ndindex(3, 3, 3):
            o = np.array(o) - 1
            if 0 < (o ** 2).sum() < dist2:
                r_ = q + o
                inb = np.all((r_ >= 0) & (r_ < (X, Y, Z)), axis=1)
                g_ = np.full(len(q), 17)
                g_[inb] = gt[r_[inb, 0], r_[inb, 1], r_[inb, 2]]
                ok &= (g_ == 17) | (g_ == 255)
        q = q[ok]
        pred[q[:, 0], q[:, 1], q[:, 2]] = rng.randint(1, 17, len(q))
    return pred, gt


def _fscore_masks(rng, X, Y, Z):
    """camera mask: a field of view (a wedge in x / y) with per-voxel dropout; lidar mask: a range ring with dropout"""
    xs, ys = np.meshgrid(np.arange(X) - X / 2 + 0.5, np.arange(Y) - Y / 2 + 0.5, indexing='ij')
    cam = (np.abs(np.arctan2(ys, xs)) < 2.2)[:, :, None] & (rng.rand(X, Y, Z) < 0.9)
    rr = np.hypot(xs, ys)
    lid = ((rr > X * 0.05) & (rr < X * 0.45))[:, :, None] & (rng.rand(X, Y, Z) < 0.85)
    return cam, lid


def gen_fscore(om):
    """Metric_FScore (occ_metrics.py:322-410, the imported reference with its sklearn KDTrees) on structured scenes.  Per case:
    the grids, every sample's (acc, cmpl, f) -- the tot_* of a fresh reference metric per sample, i.e. tot_* minus 0 -- and the
    totals of one reference metric over the case's samples in order.  The reference writes 255 into its inputs under a mask:
    it gets copies."""
    import contextlib
    import io
    rng = np.random.RandomState(61)
    cases = []                                                 # (name, metric kwargs, samples [(pred, gt, mask_lidar, mask_camera)])

    def scenes(n, X=200, Y=200, Z=16):
        out = []
        for _ in range(n):
            pred, gt = _fscore_scene(rng, X, Y, Z)
            cam, lid = _fscore_masks(rng, X, Y, Z)
            out.append((pred, gt, lid, cam))
        return out
    cases.append(('plain', dict(), scenes(2)))
    cases.append(('camera', dict(use_image_mask=True), scenes(2)))
    cases.append(('lidar', dict(use_lidar_mask=True), scenes(1)))
    cases.append(('camera_void17', dict(use_image_mask=True, void=[17]), scenes(1)))
    cases.append(('thr', dict(threshold_acc=1.0, threshold_complete=0.45), scenes(1)))
    cases.append(('voxel', dict(voxel_size=[0.5, 0.5, 0.25]), scenes(1)))
    s = scenes(1)[0]
    gt = s[1].copy()
    gt[:60, :, 4:] = np.where(gt[:60, :, 4:] == 17, 255, gt[:60, :, 4:])     # unobserved space
    gt[150:, 150:, :] = 255
    cases.append(('gt255', dict(), [(s[0], gt, s[2], s[3])]))
    s = scenes(1)[0]
    cases.append(('allfree', dict(), [(np.full_like(s[0], 17), s[1], s[2], s[3])]))
    cases.append(('small', dict(use_image_mask=True), scenes(2, 100, 100, 8)))
    out = {'cases': np.array([c[0] for c in cases])}
    for name, kw, samples in cases:
        ref = om.Metric_FScore(**kw)
        per = []
        for pred, gt, lid, cam in samples:
            one = om.Metric_FScore(**kw)
            one.add_batch(pred.copy(), gt.copy(), lid.copy(), cam.copy())
            ref.add_batch(pred.copy(), gt.copy(), lid.copy(), cam.copy())
            per.append((one.tot_acc - 0.0, one.tot_cmpl - 0.0, one.tot_f1_mean - 0.0))
        with contextlib.redirect_stdout(io.StringIO()):
            ref.count_fscore()
        full = om.Metric_FScore(**kw)
        pre = name + '_'
        out[pre + 'pred'] = np.stack([t[0] for t in samples])
        out[pre + 'gt'] = np.stack([t[1] for t in samples])
        if full.use_lidar_mask:
            out[pre + 'mask_lidar'] = np.stack([t[2] for t in samples])
        if full.use_image_mask:
            out[pre + 'mask_camera'] = np.stack([t[3] for t in samples])
        out[pre + 'per_sample'] = np.array(per, np.float64)
        out[pre + 'totals'] = np.array([ref.tot_acc, ref.tot_cmpl, ref.tot_f1_mean], np.float64)
        out[pre + 'cnt'] = np.int64(ref.cnt)
        out[pre + 'thresholds'] = np.array([full.threshold_acc, full.threshold_complete], np.float64)
        out[pre + 'voxel_size'] = np.array(full.voxel_size, np.float64)
        out[pre + 'void'] = np.array(full.void, np.int64)
        out[pre + 'masks'] = np.array([full.use_lidar_mask, full.use_image_mask])
        print('fscore %-14s %s  per-sample %s' % (name, out[pre + 'totals'], out[pre + 'per_sample'].tolist()))
    save('fscore.npz', **out)


# ----------------------------------------------------------------------------- configs -> resolved model dicts
def _merge_cfg(a, b):
    """mmcv Config._merge_a_into_b: child `a` over base `b`, dicts merged recursively unless a['_delete_']."""
    b = dict(b)
    for k, v in a.items():
        if isinstance(v, dict) and isinstance(b.get(k), dict) and not v.get('_delete_', False):
            b[k] = _merge_cfg(v, b[k])
        elif isinstance(v, dict):
            b[k] = {kk: vv for kk, vv in v.items() if kk != '_delete_'}
        else:
            b[k] = v
    return b


def _load_cfg(path):
    """mmcv Config.fromfile restricted to what the PreWorld configs use: python files, `_base_` inheritance."""
    ns = {}
    exec(compile(open(path).read(), path, 'exec'), ns)
    cfg = {k: v for k, v in ns.items() if not k.startswith('__') and not isinstance(v, types.ModuleType)
           and not callable(v)}
    bases = cfg.pop('_base_', [])
    bases = [bases] if isinstance(bases, str) else bases
    base_cfg = {}
    for b in bases:
        base_cfg = _merge_cfg(_load_cfg(os.path.normpath(os.path.join(os.path.dirname(path), b))), base_cfg)
    return _merge_cfg(cfg, base_cfg)


def _jsonable(v):
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (np.floating,)):
        return float(v)
    return v


def gen_configs():
    """The `model` dict of each of the six configs/preworld/**.py files with `_base_` inheritance resolved (data: the
    values the reference's registry would be asked to build) -> tests/golden/preworld_configs.json."""
    import glob
    import json
    out = {}
    for path in sorted(glob.glob(os.path.join(REF, 'configs', 'preworld', '*', '*.py'))):
        cfg = _load_cfg(path)
        out[os.path.relpath(path, os.path.join(REF, 'configs'))] = _jsonable(cfg['model'])
    assert len(out) == 6, sorted(out)
    with open(os.path.join(OUT, 'preworld_configs.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('preworld_configs.json', {k: v['type'] for k, v in out.items()})


def gen_bevdepth(vtm):
    """LSSViewTransformerBEVStereo host-side methods (view_transformer.py:713-789, :807-813): get_mlp_input,
    get_downsampled_gt_depth, get_depth_loss, cv_frustum on seeded inputs."""
    gc = dict(S.GRID_CONFIG_FULL)
    vtm.BasicBlock = _RefBasicBlock
    vt = vtm.LSSViewTransformerBEVStereo(grid_config=gc, input_size=(64, 96), in_channels=16, out_channels=8, sid=False,
                                         collapse_z=False, loss_depth_weight=0.05, downsample=16,
                                         depthnet_cfg=dict(use_dcn=False, aspp_mid_channels=8, stereo=True, bias=5.0))
    g = torch.Generator().manual_seed(11)
    B, N = 2, 3
    s2e = torch.randn(B, N, 4, 4, generator=g)
    e2g = torch.randn(B, N, 4, 4, generator=g)
    K = torch.randn(B, N, 3, 3, generator=g)
    pr = torch.randn(B, N, 3, 3, generator=g)
    pt = torch.randn(B, N, 3, generator=g)
    bda = torch.randn(B, 3, 3, generator=g)
    mlp = vt.get_mlp_input(s2e, e2g, K, pr, pt, bda)
    gt = torch.rand(B, N, 64, 96, generator=g) * 60.0
    gt[torch.rand(B, N, 64, 96, generator=g) < 0.7] = 0.0
    onehot = vt.get_downsampled_gt_depth(gt)
    pred = torch.rand(B * N, vt.D, 4, 6, generator=g).softmax(1)
    loss = vt.get_depth_loss(gt, pred)
    save('bevdepth_small.npz', sensor2ego=s2e.numpy(), ego2global=e2g.numpy(), intrin=K.numpy(), post_rot=pr.numpy(),
         post_tran=pt.numpy(), bda=bda.numpy(), mlp_input=mlp.numpy(), depth_gt=gt.numpy(), onehot=onehot.numpy(),
         depth_pred=pred.numpy(), depth_loss=np.float32(loss.item()), cv_frustum=vt.cv_frustum.numpy(),
         frustum=vt.frustum.numpy())


def gen_metric_temporal(om):
    """Metric_mIoU_Temporal (occ_metrics.py:413-594) on seeded labels: dict-keyed add_batch, count_miou, count_iou."""
    import contextlib
    import io
    rng = np.random.RandomState(5)
    m = om.Metric_mIoU_Temporal(num_classes=18, use_image_mask=True)
    preds, gts, masks = [], [], []
    for _ in range(2):
        gt = {i: rng.randint(0, 18, (25, 25, 4)).astype(np.uint8) for i in (0, 2, 4, 6)}
        mk = {i: rng.rand(25, 25, 4) < 0.7 for i in (0, 2, 4, 6)}
        pred = np.stack([np.where(rng.rand(25, 25, 4) < 0.5, gt[i], rng.randint(0, 18, (25, 25, 4))).astype(np.uint8)
                         for i in (0, 2, 4, 6)])
        m.add_batch(pred, gt, mk, mk)
        preds.append(pred); gts.append(np.stack([gt[i] for i in (0, 2, 4, 6)])); masks.append(np.stack([mk[i] for i in (0, 2, 4, 6)]))
    with contextlib.redirect_stdout(io.StringIO()):
        iu1, mious = m.count_miou()
        ious = m.count_iou()
    save('metric_miou_temporal.npz', pred=np.stack(preds), gt=np.stack(gts), mask=np.stack(masks),
         hist_0s=m.hist_0s, hist_1s=m.hist_1s, hist_2s=m.hist_2s, hist_3s=m.hist_3s, occ_hist_1s=m.occ_hist_1s,
         iou_1s=iu1, mious=np.array(mious), ious=np.array(ious), cnt=np.int64(m.cnt))


def gen_encoder_train(res):
    """A6/A7 in TRAINING mode (forward_train's use of the encoder): the reference CustomResNet3D with batch-statistics BatchNorm,
    one forward + backward of a fixed scalar objective through torch autograd on the CPU.  Stored: the three stage outputs, d loss /
    d input, the gradient of every parameter and the running statistics after the step.  Inputs / weights / objective
    coefficients are regenerated from the seeds by the test."""
    sd = S.synth_state_dict(21)
    enc = res.CustomResNet3D(numC_input=64, num_layer=[1, 2, 2], with_cp=False, num_channels=[32, 64, 128], stride=[1, 2, 2],
                             backbone_output_ids=[0, 1, 2])
    own = enc.state_dict()
    with torch.no_grad():
        for k in own:
            if 'num_batches_tracked' not in k and ('img_bev_encoder_backbone.' + k) in sd:
                own[k].copy_(torch.from_numpy(sd['img_bev_encoder_backbone.' + k]))
    enc.train()
    B, Z, Y, X = 2, 6, 10, 12
    rs = np.random.RandomState(22)
    x = torch.from_numpy(rs.standard_normal((B, 64, Z, Y, X)).astype(np.float32)).requires_grad_(True)
    feats = enc(x)
    coef = [torch.from_numpy(rs.standard_normal(tuple(f.shape)).astype(np.float32)) for f in feats]
    loss = sum((f * c).sum() for f, c in zip(feats, coef))
    loss.backward()
    out = dict(seed_sd=np.int64(21), seed_in=np.int64(22), shape=np.array([B, Z, Y, X]), loss=np.float64(loss.item()),
               dx=x.grad.numpy())
    for i, f in enumerate(feats):
        out['feat%d' % i] = f.detach().numpy()
    # conv weight gradients: in full for stage 0, as 8 seeded random projections per output channel for the larger layers
    # (keeps the fixture at ~1 MB; tests/test_gpu_train.py projects its own gradient with the same matrix)
    for k, p_ in enc.named_parameters():
        g = p_.grad.numpy()
        if g.ndim == 5 and not k.startswith('layers.0.'):
            R = np.random.RandomState(23).standard_normal((g[0].size, 8)).astype(np.float64)
            out['gradproj.' + k] = g.reshape(g.shape[0], -1).astype(np.float64) @ R
        else:
            out['grad.' + k] = g
    for k, b_ in enc.named_buffers():
        if 'num_batches_tracked' not in k:
            out['buf.' + k] = b_.detach().numpy().copy()
    save('encoder_train_small.npz', **out)


def gen_neck_head_train(fpn, occ):
    """A8 / A9 / A11 in TRAINING mode, composed the way forward_train does (preworld.py:237-247): LSSFPN3D -> final_conv
    (ConvModule with bias, default ReLU) -> permute to (X,Y,Z) -> OccHead, every BatchNorm on batch statistics; one forward +
    backward of a fixed scalar objective through torch autograd on the CPU."""
    sd = S.synth_state_dict(31)
    neck = fpn.LSSFPN3D(in_channels=224, out_channels=32)
    head = occ.OccHead(with_cp=False, use_deblock=False, norm_cfg=dict(type='SyncBN', requires_grad=True), soft_weights=True,
                       final_occ_size=[200, 200, 16], empty_idx=17, num_level=1, in_channels=[32], out_channel=18,
                       point_cloud_range=[-40, -40, -1, 40, 40, 5.4])
    fconv = _ConvModule(32, 32, kernel_size=3, stride=1, padding=1, bias=True, conv_cfg=dict(type='Conv3d'))
    with torch.no_grad():
        load_sd(neck, sd, 'img_bev_encoder_neck.')
        load_sd(head, sd, 'occupancy_head.')
        load_sd(fconv, sd, 'final_conv.')
    neck.train(); head.train(); fconv.train()
    Z, Y, X = 8, 16, 12
    rs = np.random.RandomState(32)
    feats = [torch.from_numpy(rs.standard_normal((2, c, Z // d, Y // d, X // d)).astype(np.float32)).requires_grad_(True)
             for c, d in ((32, 1), (64, 2), (128, 4))]
    nk = neck(feats)
    vf = fconv(nk).permute(0, 4, 3, 2, 1)                            # (B,X,Y,Z,C)  preworld.py:238
    logits = torch.stack([head([vf[b].permute(3, 0, 1, 2).unsqueeze(0)])['output_voxels'][0].squeeze(0)
                          for b in range(vf.shape[0])], 0)          # (B,18,X,Y,Z): per batch element, like :240-247
    coef = torch.from_numpy(rs.standard_normal(tuple(logits.shape)).astype(np.float32))
    loss = (logits * coef).sum()
    loss.backward()
    out = dict(seed_sd=np.int64(31), seed_in=np.int64(32), shape=np.array([2, Z, Y, X]), loss=np.float64(loss.item()),
               neck=nk.detach().numpy(), logits=logits.detach().numpy())
    for i, f in enumerate(feats):
        out['dfeat%d' % i] = f.grad.numpy()
    for name, mod in (('neck', neck), ('final_conv', fconv), ('head', head)):
        for k, p_ in mod.named_parameters():
            if p_.grad is not None:
                out['grad.%s.%s' % (name, k)] = p_.grad.numpy()
        for k, b_ in mod.named_buffers():
            if 'num_batches_tracked' not in k:
                out['buf.%s.%s' % (name, k)] = b_.detach().numpy().copy()
    save('neck_head_train_small.npz', **out)


class _FakeCenterPoint(nn.Module):
    """stands in for mmdet3d CenterPoint / MVXTwoStageDetector / mmdet BaseDetector (class plumbing the camera -> occupancy path
    never executes): builds the image modules it is given, nothing else"""

    def __init__(self, img_backbone=None, img_neck=None, **kwargs):
        super().__init__()
        self.img_backbone = _build_from_cfg(img_backbone)
        self.img_neck = _build_from_cfg(img_neck)

    @property
    def with_img_neck(self):
        return self.img_neck is not None


def load_detectors(occ):
    """import the reference's detector classes themselves (bevdet.py, bevdet_occ.py, preworld.py, preworld_temporal_traj.py) on
    top of the sub-modules already loaded: fakes for the bases and for the debugging / plotting imports they carry"""
    pkg = _mod('mmdet3d.models.detectors')
    _mod('mmdet3d.models.detectors.centerpoint', CenterPoint=_FakeCenterPoint)
    if 'mmdet3d.models.backbones.swin' not in sys.modules:
        _mod('mmdet3d.models.backbones.swin', SwinTransformer=type('SwinTransformer', (nn.Module,), {}))
    sys.modules['mmdet.models.backbones.resnet'].ResNet = type('ResNet', (nn.Module,), {})
    _mod('IPython', embed=lambda *a, **k: None)
    _mod('matplotlib', cm=None)
    _mod('matplotlib.pyplot')
    sys.modules['mmdet3d.models.heads'].DownScaleModule3DCustom = occ.DownScaleModule3DCustom
    _mod('mmdet3d.core')
    _mod('mmdet3d.core.bbox', Box3DMode=types.SimpleNamespace(LIDAR=0), Coord3DMode=None, LiDARInstance3DBoxes=None)
    load_ref('mmdet3d.models.detectors.loss', 'mmdet3d/models/detectors/loss.py')
    load_ref('mmdet3d.models.detectors.lovasz_softmax', 'mmdet3d/models/detectors/lovasz_softmax.py')
    load_ref('mmdet3d.models.detectors.bevdet', 'mmdet3d/models/detectors/bevdet.py')
    load_ref('mmdet3d.models.detectors.bevdet_occ', 'mmdet3d/models/detectors/bevdet_occ.py')
    pw = load_ref('mmdet3d.models.detectors.preworld', 'mmdet3d/models/detectors/preworld.py')
    pt = load_ref('mmdet3d.models.detectors.preworld_temporal_traj', 'mmdet3d/models/detectors/preworld_temporal_traj.py')
    return pw, pt


def _near_ties(logits, frac=1e-3):
    """voxels of a (1, n_cls, X, Y, Z) logit tensor whose top-2 margin is below frac * max|logit|: (flat (X,Y,Z) indices, margins,
    runner-up classes) -- the only voxels a correct fp32-level implementation may decide differently"""
    lg = logits[0].reshape(logits.shape[1], -1)
    top = lg.topk(2, dim=0)
    margin = (top.values[0] - top.values[1])
    sel = torch.nonzero(margin < frac * lg.abs().max()).reshape(-1)
    return sel.numpy().astype(np.int64), margin[sel].numpy().astype(np.float32), top.indices[1][sel].numpy().astype(np.uint8)


def _run_reference_detector(E, tag, det, post_ft, with_prev, sd, inputs, variant, out, rs, shape):
    model = _build_from_cfg(E.model_cfg(det, post_ft, with_prev, variant=variant))
    own = set(model.state_dict().keys())
    state = {k: torch.from_numpy(v) for k, v in sd.items() if k in own}      # (PreWorld has no forecast / trajectory heads)
    missing, unexpected = model.load_state_dict(state, strict=False)
    hot_missing = [k for k in missing if 'depth_net' not in k and 'num_batches_tracked' not in k and not k.startswith('semantic_loss')]
    assert not hot_missing and not unexpected, (hot_missing[:5], unexpected[:5])
    model.eval()
    dn = E.install_image_side(model, seed=0, variant=variant)
    rec, logits = {}, []
    model.final_conv.register_forward_hook(lambda m, i, o: rec.update(bev=i[0].detach(), vf=o.detach()))
    model.occupancy_head.register_forward_hook(lambda m, i, o: logits.append(o['output_voxels'][0].detach()))
    with torch.no_grad():
        prep = model.prepare_inputs(inputs, stereo=True)
        res = model.simple_test(None, None, img=inputs, temporal_ego_states=E.ego_states(0))
    if tag == 'p4d_ft':
        out['prep_sensor2keyego'] = torch.stack(prep[1], 0).numpy()             # (T, B, N, 4, 4)
        out['prep_curr2adjsensor'] = torch.stack(prep[7][:2], 0).numpy()
        out['mlp_input'] = torch.stack(dn.mlp_inputs, 0).numpy()                # calls: adjacent frame, key frame
        out['sample_idx'] = rs.randint(0, shape[0] * shape[1] * shape[2], 1024).astype(np.int64)
    idx = out['sample_idx']
    # rows of the (B,C,Z,Y,X) tensors at flat voxel index z*Y*X + y*X + x
    out[tag + '_bev_rows'] = rec['bev'][0].reshape(32, -1)[:, idx].T.contiguous().numpy()
    out[tag + '_vf_rows'] = rec['vf'][0].reshape(32, -1)[:, idx].T.contiguous().numpy()
    out[tag + '_bev_abs_sum'] = np.float64(rec['bev'].double().abs().sum())
    out[tag + '_n_depthnet_calls'] = np.int64(dn.k)
    for k, v in res.items():
        assert v[0].dtype == np.uint8 and v[0].shape == shape, (k, v[0].dtype, v[0].shape)
        out[tag + '_' + k] = v[0]
    out[tag + '_keys'] = np.array(sorted(res.keys()))
    if post_ft:
        # the OccHead's own logits behind every semantic grid (round 4): the near-tie voxels -- margin below
        # 1e-3 of the largest logit -- with margin and runner-up class, so that a differing voxel can be EXPLAINED, not counted
        sem_keys = [k for k in res if k.startswith('semantic_occ')]             # insertion order = decode order
        assert len(sem_keys) == len(logits), (sem_keys, len(logits))
        for k, lg in zip(sem_keys, logits):
            assert np.array_equal(lg[0].argmax(0).numpy().astype(np.uint8), res[k][0])
            ti, tm, tc = _near_ties(lg)
            out['%s_%s_tie_idx' % (tag, k)], out['%s_%s_tie_margin' % (tag, k)], out['%s_%s_tie_cls' % (tag, k)] = ti, tm, tc
            out['%s_%s_logit_absmax' % (tag, k)] = np.float32(lg.abs().max())


def gen_e2e(vtm, occ):
    """G13 (missing 1): the reference's OWN PreWorld4DTraj.simple_test / PreWorld.simple_test
    (preworld_temporal_traj.py:212-370, preworld.py:159-226) with BEVStereo4DOCC.prepare_inputs / extract_img_feat
    (bevdet_occ.py:88-269) running end to end at a reduced grid, image side replaced by the seeded stand-ins of
    tests/_e2e_stub.py, native ops bound to the oracle.  Records prepare_inputs' pose algebra, the mlp_input handed to the
    DepthNet, sampled rows of the encoder output and of voxel_feats, every uint8 grid, and (post-finetune decode) the near-tie
    voxels of the OccHead logits.  e2e_small.npz: 2 cameras, 40 x 40 x 8, all five detector / decode combinations;
    e2e_c6.npz: 6 cameras, 100 x 100 x 8 (BASELINE.json configs[0]'s grid with the full rig), PreWorld4DTraj post-finetune;
    e2e_full.npz: 6 cameras, 200 x 200 x 16 -- the headline grid -- same detector."""
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import _e2e_stub as E
    vtm.BasicBlock = _RefBasicBlock
    load_detectors(occ)
    sd = S.synth_state_dict(0)
    inputs = E.img_inputs(0)
    rs = np.random.RandomState(77)
    out = {}
    for tag, det, post_ft, with_prev in E.RUNS:
        _run_reference_detector(E, tag, det, post_ft, with_prev, sd, inputs, 'small', out, rs, (40, 40, 8))
    save('e2e_small.npz', **out)
    out6 = {}
    _run_reference_detector(E, 'p4d_ft', 'PreWorld4DTraj', True, True, sd, E.img_inputs(0, 'c6'), 'c6', out6, np.random.RandomState(78),
                            (100, 100, 8))
    save('e2e_c6.npz', **out6)
    if os.environ.get('PW_GEN_E2E_FULL', '1') == '1':
        # the headline grid itself (200 x 200 x 16, 6 cameras, 7 states) through the reference's PreWorld4DTraj.simple_test: ~1 min of CPU.
        # geo grids are {0, 17}-valued: stored as bit masks
        outf = {}
        _run_reference_detector(E, 'p4d_ft', 'PreWorld4DTraj', True, True, sd, E.img_inputs(0, 'full'), 'full', outf,
                                np.random.RandomState(79), (200, 200, 16))
        for k in [k for k in outf if k.startswith('p4d_ft_geo_occ')]:
            g = outf.pop(k)
            assert set(np.unique(g).tolist()) <= {0, 17}
            outf[k + '_is17_bits'] = np.packbits(g.reshape(-1) == 17)
        save('e2e_full.npz', **outf)


def gen_e2e_train(vtm, occ):
    """G14 (VERDICT r03 missing 3 / next 6): the reference's OWN forward_train -- PreWorld.forward_train (preworld.py:229-309) and
    PreWorld4DTraj.forward_train (preworld_temporal_traj.py:372-530) -- run here in train() mode at the reduced grid: batch-statistics
    BatchNorm, QuickCumsumCuda with its backward (bev_pool.py:17-81, native ops bound to the oracle), which state gets which loss
    under which key (`..._{k}s`), the loss weights, the class-weighted CE / sem_scal / geo_scal / Lovasz terms of loss_voxel, the
    forecast recursion with the trajectory branch and loss_traj.  (use_focal_loss is off: CustomFocalLoss hard-codes a 200 x 200
    radial map, focal_loss.py:197-203, and is pinned at that size by voxel_losses2.npz.)  Image side = the seeded stand-ins of tests/_e2e_stub.py.
    Stored: every loss value, d sum(losses) / d final_conv.weight (all of it), d / d of one encoder and one pre_process weight
    (strided samples), and for the temporal detector the gradients of the forecast / trajectory heads."""
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import _e2e_stub as E
    vtm.BasicBlock = _RefBasicBlock
    load_detectors(occ)
    sd = S.synth_state_dict(0)
    for variant, runs, fname in (('small', (('pw', 'PreWorld'), ('p4d', 'PreWorld4DTraj')), 'e2e_train_small.npz'),
                                 ('full', (('pw', 'PreWorld'),), 'e2e_train_full.npz')):
        if variant == 'full' and os.environ.get('PW_GEN_E2E_FULL', '1') != '1':
            continue
        _gen_e2e_train_variant(E, sd, variant, runs, fname)


def _gen_e2e_train_variant(E, sd, variant, runs, fname):
    """one fixture of gen_e2e_train: `small` (2 cameras, 40 x 40 x 8, both detectors) or `full` (6 cameras, the headline 200 x 200 x 16 grid,
    PreWorld: a few minutes of the reference on this container's CPUs)"""
    inputs = E.img_inputs(0, variant)
    out = {}
    for tag, det in runs:
        cfg = E.model_cfg(det, True, True, variant=variant)
        cfg.update(E.TRAIN_CFG)
        model = _build_from_cfg(cfg)
        own = set(model.state_dict().keys())
        missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if k in own}, strict=False)
        assert not unexpected
        model.train()
        if hasattr(model, 'set_epoch'):
            model.set_epoch(E.TRAIN_EPOCH)                      # the epoch hook's call (:156-157): epoch 7 -> future intervals 0, 1, 2
        E.install_image_side(model, seed=0, variant=variant)
        kw = E.train_kwargs(0, det, variant=variant)
        losses = model.forward_train(None, [dict()], img_inputs=inputs, **kw)
        total = sum(losses.values())
        total.backward()
        out[tag + '_keys'] = np.array(sorted(losses.keys()))
        for k, v in losses.items():
            out['%s_%s' % (tag, k)] = np.float64(v.detach())
        out[tag + '_total'] = np.float64(total.detach())
        probes = dict(E.grad_probes(model, det))
        for name, p in probes.items():
            assert p.grad is not None, name
            g = p.grad.detach().reshape(-1)
            out['%s_grad_%s' % (tag, name)] = g.numpy().copy() if g.numel() <= 40000 else g[::7].numpy().copy()
            out['%s_gradnorm_%s' % (tag, name)] = np.float64(p.grad.double().norm())
        bn = model.occupancy_head.occ_convs[0][1]
        out[tag + '_occ_bn_running_mean'] = bn.running_mean.numpy().copy()
        out[tag + '_occ_bn_batches'] = np.int64(bn.num_batches_tracked)
    save(fname, **out)


def _flatten_eff_distloss(w, m, interval, ray_id):
    """torch_efficient_distloss.flatten_eff_distloss (un-vendored third-party dependency, requirements.txt:27, version unpinned;
    PARITY UNPINNED as SURVEY 8c allows): restated from the package's published algorithm -- the Mip-NeRF-360 distortion loss
    by exclusive per-ray prefix sums, loss = sum_i [(1/3) interval w_i^2 + 2 w_i (m_i W_i - WM_i)] / (max(ray_id) + 1) -- in
    differentiable torch ops (the package's hand-written backward is the analytic gradient of this expression).  ray_id sorted."""
    n_rays = ray_id.max() + 1
    wm = w * m
    first = torch.ones_like(ray_id, dtype=torch.bool)
    first[1:] = ray_id[1:] != ray_id[:-1]
    start = torch.cummax(torch.where(first, torch.arange(len(w)), torch.zeros_like(ray_id)), 0).values
    cw, cwm = torch.cumsum(w, 0), torch.cumsum(wm, 0)
    w_pre = (cw - w) - (cw - w)[start]
    wm_pre = (cwm - wm) - (cwm - wm)[start]
    return ((1 / 3) * interval * w.pow(2) + 2 * w * (m * w_pre - wm_pre)).sum() / n_rays


def _grad_samples(grads, seed, n=1024):
    """values of gradient grids at seeded non-zero voxels + sums (grads: density (X,Y,Z), semantic (X,Y,Z,17), color (X,Y,Z,3))"""
    rng = np.random.RandomState(seed)
    nz = torch.nonzero(grads[0].abs() > 0).numpy()
    pick = nz[rng.choice(len(nz), min(n, len(nz)), replace=False)]
    ix = tuple(torch.from_numpy(pick[:, i]) for i in range(3))
    return dict(voxels=pick.astype(np.int16), g_density=grads[0][ix].numpy(), g_semantic=grads[1][ix].numpy(), g_color=grads[2][ix].numpy(),
                sum_density=np.float64(grads[0].double().sum()), abs_density=np.float64(grads[0].double().abs().sum()),
                abs_semantic=grads[1].double().abs().sum((0, 1, 2)).numpy(), abs_color=grads[2].double().abs().sum((0, 1, 2)).numpy(),
                n_nonzero=np.int64(len(nz)))


def gen_nerf_losses(nh):
    """the imported reference NerfHead.forward (nerf_head.py:355-420) itself -- the gt_depth > 52 cut (:379),
    the per-batch loop and the division by the batch size (:365-419), compute_loss / compute_loss_temporal (:271-329) with
    silog_loss / l1_loss (nerf/utils.py:71-87), n_max = len(results['t']) as the distortion interval (:296-297) -- at B = 2 on two
    mixed-opacity scenes (rays that terminate), with the released config's weights (preworld-7frame-pretrain.py:22-33), once plain
    and once with if_temporal=True, interval=2.  Stored: every loss value, the gradient of sum(losses) w.r.t. the density /
    semantic / colour grids at sampled voxels + sums, per batch element.  torch_efficient_distloss is absent: see
    _flatten_eff_distloss (third-party, unpinned); the fixture also stores the run with weight_distortion=0."""
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import _e2e_stub as E
    nh.flatten_eff_distloss = _flatten_eff_distloss
    cfg = dict(E.NERF_HEAD_CFG)
    cfg.pop('type')
    B, R = 2, 192
    grids = [S.render_grids_mixed(71 + b) for b in range(B)]
    rays = np.zeros((B, R, 16), np.float32)
    rs = np.random.RandomState(73)
    for b in range(B):
        o, d = S.rays_mixed(74 + b, R)
        depth = rs.uniform(1.0, 50.0, R)
        depth[rs.rand(R) < 0.1] = 0.0
        far = rs.rand(R) < 0.12
        depth[far] = rs.uniform(52.5, 70.0, int(far.sum()))
        rays[b, :, 2], rays[b, :, 3], rays[b, :, 4:7], rays[b, :, 7:10] = depth, rs.randint(0, 17, R), o, d
        rays[b, :, 13:16] = rs.uniform(0, 1, (R, 3))
    bda = np.stack([np.array([[0.98, 0.05, 0.0], [-0.05, 0.98, 0.0], [0.0, 0.0, 1.0]], np.float32),
                    np.array([[1.01, -0.03, 0.0], [-0.03, -1.01, 0.0], [0.0, 0.0, 1.0]], np.float32)])
    out = dict(rays=rays, bda=bda, grid_seeds=np.array([71, 72], np.int64), class_weights=nh.NerfHead(**cfg).class_weights.numpy())
    for tag, extra, wd in (('plain', {}, 0.01), ('temporal', dict(if_temporal=True, interval=2), 0.01), ('nodist', {}, 0.0)):
        head = nh.NerfHead(**dict(cfg, weight_distortion=wd))
        g = [[torch.from_numpy(gr[i]) for gr in grids] for i in range(3)]
        density, semantic, color = [torch.stack(x, 0).requires_grad_() for x in g]
        r = torch.from_numpy(rays.copy())
        losses = head(density, semantic, color, rays=r, bda=torch.from_numpy(bda), **extra)
        assert bool((r[..., 2] <= 52).all())                                     # the in-place cut reached the caller's tensor
        total = sum(losses.values())
        total.backward()
        out[tag + '_keys'] = np.array(sorted(losses.keys()))
        for k, v in losses.items():
            out['%s_%s' % (tag, k)] = np.float64(v.detach())
            print('  nerf_losses %-8s %-28s %.7f' % (tag, k, float(v)))
        out[tag + '_total'] = np.float64(total.detach())
        for b in range(B):
            for k, v in _grad_samples([density.grad[b], semantic.grad[b], color.grad[b]], 75 + b).items():
                out['%s_b%d_%s' % (tag, b, k)] = v
    # what the scene does to the rays (for the record): the last run's per-ray transmittance on batch element 0
    with torch.no_grad():
        m = torch.from_numpy(rays[0, :, 2]) > 0
        m &= torch.from_numpy(rays[0, :, 2]) <= 52
        res = head.render_one_scene(torch.from_numpy(rays[0, :, 4:7]), torch.from_numpy(rays[0, :, 7:10]), torch.from_numpy(bda[0]),
                                    *[torch.from_numpy(a) for a in grids[0]], mask=m)
    last = res['alphainv_last'].numpy()
    out['b0_n_rays'], out['b0_n_terminated'] = np.int64(len(last)), np.int64((last < 1e-3).sum())
    print('  nerf_losses: batch 0 renders %d of %d rays, %d terminate' % (len(last), R, int((last < 1e-3).sum())))
    save('nerf_losses_small.npz', **out)


def _run_reference_forward_train(E, sd, det, cfg_extra, kw, inputs, variant, epoch, probes_fn, tag, out):
    cfg = E.model_cfg(det, True, True, variant=variant)
    cfg.update(cfg_extra)
    model = _build_from_cfg(cfg)
    own = set(model.state_dict().keys())
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k in own}, strict=False)
    assert not unexpected
    model.train()
    if hasattr(model, 'set_epoch'):
        model.set_epoch(epoch)
    E.install_image_side(model, seed=0, variant=variant)
    stats = []
    if getattr(model, 'if_render', False):
        # what the scene does to the rays, in train() mode: per NerfHead batch element (rays rendered, terminated at T < 1e-3, partly opaque)
        for name in ('compute_loss', 'compute_loss_temporal'):
            def wrap(results, *a, _f=getattr(model.nerf_head, name)):
                last = results['alphainv_last'].detach()
                stats.append((len(last), int((last < 1e-3).sum()), int(((last >= 1e-3) & (last < 0.99)).sum())))
                return _f(results, *a)
            setattr(model.nerf_head, name, wrap)
    losses = model.forward_train(None, [dict()] * inputs[0].shape[0], img_inputs=inputs, **kw)
    total = sum(losses.values())
    total.backward()
    if stats:
        out[tag + '_render_stats'] = np.array(stats, np.int32)
        print('  %s: (rays, terminated, partly opaque) per NerfHead batch element: %s' % (tag, stats))
    out[tag + '_keys'] = np.array(sorted(losses.keys()))
    for k, v in losses.items():
        out['%s_%s' % (tag, k)] = np.float64(v.detach())
        print('  %-6s %-30s %.7f' % (tag, k, float(v)))
    out[tag + '_total'] = np.float64(total.detach())
    for name, p in probes_fn(model, det):
        assert p.grad is not None, name
        g = p.grad.detach().reshape(-1)
        out['%s_grad_%s' % (tag, name)] = g.numpy().copy() if g.numel() <= 40000 else g[::7].numpy().copy()
        out['%s_gradnorm_%s' % (tag, name)] = np.float64(p.grad.double().norm())
    for name, bn in (('occ', model.occupancy_head.occ_convs[0][1]), ('enc', model.img_bev_encoder_backbone.layers[0][0].conv1.bn),
                     ('pre', model.pre_process_net.layers[0][0].conv1.bn)):
        out['%s_%s_bn_running_mean' % (tag, name)] = bn.running_mean.numpy().copy()
        out['%s_%s_bn_running_var' % (tag, name)] = bn.running_var.numpy().copy()
        out['%s_%s_bn_batches' % (tag, name)] = np.int64(bn.num_batches_tracked)
    return model


def gen_e2e_pretrain(vtm, occ, nh):
    """the reference's OWN PreWorld.forward_train (preworld.py:229-309) and PreWorld4DTraj.forward_train
    (preworld_temporal_traj.py:372-530) under the PRE-TRAIN flags of configs/preworld/nuscenes/preworld-7frame-pretrain.py:10-33 /
    nuscenes-temporal/preworld-7frame-pretrain-traj.py (if_render=True, if_post_finetune=False, render weights 1 / 1 / 1 / 0.01 /
    0.01, use_lss_depth_loss True / False), train() mode, **B = 2** (samples_per_gpu=2, :58), epoch 4 for the temporal detector
    (temporal_rays[1..3] feed the forecast states).  Branches run here for the first time: loss_sup_voxel x 0 (preworld.py:130-135),
    NerfHead.forward on the MLP outputs (:287-290), get_depth_loss (:303-304), the `_{k}s` render keys.  density_mlp's output row is
    rescaled (tests/_e2e_stub.py opaque_density_state) so that a good part of the rays terminate."""
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import _e2e_stub as E
    vtm.BasicBlock = _RefBasicBlock
    load_detectors(occ)
    nh.flatten_eff_distloss = _flatten_eff_distloss
    sd = E.opaque_density_state(S.synth_state_dict(0))
    inputs = E.img_inputs(0, 'small', batch=2)
    out = {}
    for tag, det in (('pw', 'PreWorld'), ('p4d', 'PreWorld4DTraj')):
        kw = E.pretrain_kwargs(0, det, batch=2)
        _run_reference_forward_train(E, sd, det, E.pretrain_cfg(det), kw, inputs, 'small', E.PRETRAIN_EPOCH, E.pretrain_grad_probes, tag, out)
    save('e2e_pretrain_small.npz', **out)


def gen_e2e_train_b2(vtm, occ):
    """the fine-tune forward_train of both reference detectors at the reference's training batch,
    samples_per_gpu = 2 (configs/preworld/nuscenes/preworld-7frame-finetune.py:58): BatchNorm statistics over two samples, the per-batch
    OccHead loop (preworld.py:240-247), (B,X,Y,Z) labels.  Same flags / epoch as e2e_train_small.npz."""
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import _e2e_stub as E
    vtm.BasicBlock = _RefBasicBlock
    load_detectors(occ)
    sd = S.synth_state_dict(0)
    inputs = E.img_inputs(0, 'small', batch=2)
    out = {}
    for tag, det in (('pw', 'PreWorld'), ('p4d', 'PreWorld4DTraj')):
        _run_reference_forward_train(E, sd, det, E.TRAIN_CFG, E.train_kwargs(0, det, batch=2), inputs, 'small', E.TRAIN_EPOCH,
                                     E.grad_probes, tag, out)
    save('e2e_train_small_b2.npz', **out)


def main():
    os.makedirs(OUT, exist_ok=True)
    install_shim()
    bp = load_ref('mmdet3d.ops.bev_pool_v2.bev_pool', 'mmdet3d/ops/bev_pool_v2/bev_pool.py')
    torch.cuda.amp.autocast_mode  # noqa: B018 (import check)
    vtm = load_ref('mmdet3d.models.necks.view_transformer', 'mmdet3d/models/necks/view_transformer.py')
    res = load_ref('mmdet3d.models.backbones.resnet', 'mmdet3d/models/backbones/resnet.py')
    fpn = load_ref('mmdet3d.models.necks.lss_fpn', 'mmdet3d/models/necks/lss_fpn.py')
    occ = load_ref('mmdet3d.models.heads.occupancy_head', 'mmdet3d/models/heads/occupancy_head.py')
    om = load_ref('ref_occ_metrics', 'mmdet3d/datasets/occ_metrics.py')
    # nerf utils JIT-compile CUDA at import: provide the module instead
    _mod('mmdet3d.models.nerf.utils')
    ut_src = types.ModuleType('mmdet3d.models.nerf.utils')
    import torch.utils.cpp_extension as cpp_ext
    real_load = cpp_ext.load
    cpp_ext.load = lambda name, **kw: _NativeStubs
    sys.modules['turtle'] = types.ModuleType('turtle')
    sys.modules['turtle'].forward = None
    try:
        ut = load_ref('mmdet3d.models.nerf.utils', 'mmdet3d/models/nerf/utils.py')
    finally:
        cpp_ext.load = real_load
    nh = load_ref('mmdet3d.models.nerf.nerf_head', 'mmdet3d/models/nerf/nerf_head.py')
    only = set(sys.argv[1:])          # e.g. `python tools/gen_golden.py configs metric_temporal` regenerates just those

    def want(name):
        return not only or name in only
    if want('configs'):
        gen_configs()
    if want('bevdepth'):
        gen_bevdepth(vtm)
    if want('metric_temporal'):
        gen_metric_temporal(om)
    if want('render_grad'):
        gen_render_grad(nh)
    if want('render_mixed'):
        gen_render_mixed(nh)
    if want('encoder_train'):
        gen_encoder_train(res)
    if want('neck_head_train'):
        gen_neck_head_train(fpn, occ)
    if want('e2e'):
        gen_e2e(vtm, occ)
    if want('e2e_train'):
        gen_e2e_train(vtm, occ)
    if want('nerf_losses'):
        gen_nerf_losses(nh)
    if want('e2e_pretrain'):
        gen_e2e_pretrain(vtm, occ, nh)
    if want('e2e_train_b2'):
        gen_e2e_train_b2(vtm, occ)
    if want('fscore'):
        gen_fscore(om)
    if want('ray_labels'):
        gen_ray_labels()
    if only:
        return
    gen_kat(bp)
    gen_geometry(vtm)
    gen_conv_stack(res, fpn, occ)
    gen_forecast()
    gen_traj(occ)
    gen_rays()
    gen_losses()
    gen_losses2()
    gen_image_branch(vtm, fpn)
    gen_stereo(vtm)
    gen_render(nh)
    gen_metric(om)


if __name__ == '__main__':
    main()
