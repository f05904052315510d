"""Detector-level drop-ins: `BEVStereo4DOCC` (composition base), `PreWorld` (single time step) and
`PreWorld4DTraj` (state-conditioned 4-D forecasting) -- the classes `configs/preworld/**.py` instantiate through
`model = dict(type=...)` (mmdet3d/models/detectors/bevdet_occ.py:45-327, preworld.py:23-226,
preworld_temporal_traj.py:26-370).  Same constructor kwargs, attribute names (= state-dict keys), `simple_test`
signature and result dicts as the reference.

Everything downstream of the image-view features runs on libpreworld_hip.so (channels-last, no permute copies); the
image backbone / neck / DepthNet are plain PyTorch-ROCm modules (image_encoder.py), as north_star prescribes.
`img_backbone` / `img_neck` are optional: the benchmarks and most parity tests start from the lifted inputs
(`simple_test_from_lift`) and need no 88 M-parameter Swin-B.  `PreWorld.forward_train` and `PreWorld4DTraj.forward_train` run the
voxel side of the training step on the HIP training kernels (preworld_amd/train.py), and so does `BEVStereo4DOCC.forward_train`
(depth loss + softmax cross entropy on the predicter's logits)."""
import os

import numpy as np
import torch
import torch.nn as nn

from . import builder, ops
from .modules import (ConvModule3d, Derived, DownScaleModule3DCustom, as_f32, precision, to_channels_last_3d)


# occ3d-nuScenes voxel counts per class (mmdet3d/models/detectors/preworld.py:19-21): class weights 1 / log(freq)
NUSC_CLASS_FREQUENCIES = np.array([1163161, 2309034, 188743, 2997643, 20317180, 852476, 243808, 2457947, 497017, 2731022,
                                   7224789, 214411435, 5565043, 63191967, 76098082, 128860031, 141625221, 2307405309],
                                  dtype=np.float64)


class BEVStereo4DOCC(nn.Module):
    """bevdet.py:20-58 (BEVDet), :273-288 (BEVDet4D), :565-571 (BEVStereo4D) and bevdet_occ.py:45-269 (BEVStereo4DOCC)
    restricted to what the camera -> occupancy forward pass uses."""

    def __init__(self, img_view_transformer, img_bev_encoder_backbone, img_bev_encoder_neck, img_backbone=None,
                 img_neck=None, pre_process=None, align_after_view_transfromation=False, num_adj=1, with_prev=True,
                 loss_occ=None, out_dim=32, num_classes=18, use_predicter=True, class_wise=False,
                 balance_cls_weight=False, use_depth_gt=False, use_mask=False, **kwargs):
        super().__init__()
        if align_after_view_transfromation:
            raise NotImplementedError('align_after_view_transfromation=True: BEVStereo4DOCC.__init__ forces it to False '
                                      '(bevdet_occ.py:80)')
        self.img_backbone = builder.build(img_backbone)
        self.img_neck = builder.build(img_neck)
        self.with_img_neck = self.img_neck is not None
        self.img_view_transformer = builder.build(img_view_transformer, 'LSSViewTransformer')
        self.img_bev_encoder_backbone = builder.build(img_bev_encoder_backbone, 'CustomResNet3D')
        self.img_bev_encoder_neck = builder.build(img_bev_encoder_neck, 'LSSFPN3D')
        self.pre_process = pre_process is not None
        if self.pre_process:
            self.pre_process_net = builder.build(pre_process, 'CustomResNet3D')
        self.align_after_view_transfromation = False
        self.num_adj, self.with_prev = num_adj, with_prev
        self.extra_ref_frames = 1                                   # bevdet.py:567-571
        self.temporal_frame = num_adj + 1
        self.num_frame = self.temporal_frame + self.extra_ref_frames
        self.out_dim, self.num_classes = out_dim, num_classes
        self.use_predicter, self.class_wise, self.use_depth_gt = use_predicter, class_wise, use_depth_gt
        C = self.img_view_transformer.out_channels
        self.final_conv = ConvModule3d(C, out_dim if use_predicter else num_classes, 3, stride=1, padding=1, bias=True,
                                       conv_cfg=dict(type='Conv3d'))
        if use_predicter:
            self.predicter = nn.Sequential(nn.Linear(out_dim, out_dim * 2), nn.Softplus(),
                                           nn.Linear(out_dim * 2, num_classes))
        self.loss_occ_cfg = loss_occ
        self._derived = Derived()

    # ---- bevdet_occ.py:88-139 (BEVStereo4DOCC.prepare_inputs): split the stacked inputs into
    # frames and express every sweep's sensor pose in the KEY frame's ego system (fp64 algebra)
    def prepare_inputs(self, inputs, stereo=False, num_frame=None, temporal_frame=None,
                       extra_ref_frames=None):
        """inputs = (imgs (B, N*T, C, H, W) camera-major/frame-minor, sensor2egos (B, T*N, 4, 4)
        frame-major, ego2globals, intrins (B,T*N,3,3), post_rots, post_trans (B,T*N,3), bda).
        Returns (imgs[T], sensor2keyegos[T], ego2globals[T], intrins[T], post_rots[T],
        post_trans[T], bda, curr2adjsensor) exactly like the reference."""
        extra_ref_frames = self.extra_ref_frames if extra_ref_frames is None else extra_ref_frames
        num_frame = num_frame or self.num_frame
        temporal_frame = temporal_frame or self.temporal_frame
        B, N, C, H, W = inputs[0].shape
        N = N // num_frame
        imgs = inputs[0].view(B, N, num_frame, C, H, W)
        imgs = [t.squeeze(2) for t in torch.split(imgs, 1, 2)]
        sensor2egos, ego2globals, intrins, post_rots, post_trans, bda = inputs[1:7]
        sensor2egos = sensor2egos.view(B, num_frame, N, 4, 4)
        ego2globals = ego2globals.view(B, num_frame, N, 4, 4)
        keyego2global = ego2globals[:, 0, 0, ...].unsqueeze(1).unsqueeze(1)
        global2keyego = torch.inverse(keyego2global.double())
        sensor2keyegos = (global2keyego @ ego2globals.double() @ sensor2egos.double()).float()
        curr2adjsensor = None
        if stereo:
            s_curr = sensor2egos[:, :temporal_frame, ...].double()
            e_curr = ego2globals[:, :temporal_frame, ...].double()
            s_adj = sensor2egos[:, 1:temporal_frame + 1, ...].double()
            e_adj = ego2globals[:, 1:temporal_frame + 1, ...].double()
            c2a = (torch.inverse(e_adj @ s_adj) @ e_curr @ s_curr).float()
            curr2adjsensor = [p.squeeze(1) for p in torch.split(c2a, 1, 1)]
            curr2adjsensor.extend([None for _ in range(extra_ref_frames)])
            assert len(curr2adjsensor) == num_frame
        extra = [sensor2keyegos, ego2globals, intrins.view(B, num_frame, N, 3, 3),
                 post_rots.view(B, num_frame, N, 3, 3), post_trans.view(B, num_frame, N, 3)]
        extra = [[p.squeeze(1) for p in torch.split(t, 1, 1)] for t in extra]
        sensor2keyegos, ego2globals, intrins, post_rots, post_trans = extra
        return imgs, sensor2keyegos, ego2globals, intrins, post_rots, post_trans, bda, curr2adjsensor

    # ---- bevdet.py:34-50 (PyTorch-ROCm image side)
    def image_encoder(self, img, stereo=False):
        if self.img_backbone is None:
            raise RuntimeError('this detector was built without img_backbone / img_neck: feed lifted inputs to '
                               'simple_test_from_lift() or pass the image-side configs')
        B, N, C, imH, imW = img.shape
        x = self.img_backbone(img.view(B * N, C, imH, imW))
        stereo_feat = None
        if stereo:
            stereo_feat, x = x[0], x[1:]
        if self.with_img_neck:
            x = self.img_neck(x)
            if type(x) in (list, tuple):
                x = x[0]
        return x.view(B, N, *x.shape[1:]), stereo_feat

    # ---- bevdet.py:573-603 (Swin branch)
    def extract_stereo_ref_feat(self, x):
        B, N, C, imH, imW = x.shape
        return self.img_backbone.stereo_ref_feat(x.view(B * N, C, imH, imW))

    # ---- bevdet_occ.py:141-165 + the frame loop of :167-241, up to the lifted inputs of every BEV frame
    @torch.no_grad()
    def lift_inputs_from_images(self, img_inputs):
        """img_inputs: prepare_inputs(...) output.  Runs backbone + neck + DepthNet per frame in the reference's order
        (extra stereo reference -> adjacent -> key, each cost volume against the previously processed frame's stereo
        feature, `mlp_input` always from the KEY frame's poses, bevdet_occ.py:197-199) and returns the list of per-frame
        dicts `simple_test_from_lift` consumes, key frame first."""
        imgs, sensor2keyegos, ego2globals, intrins, post_rots, post_trans, bda, curr2adjsensor = img_inputs
        vt = self.img_view_transformer
        frames, feat_prev_iv = [], None
        for fid in range(self.num_frame - 1, -1, -1):
            key_frame = fid == 0
            extra_ref_frame = fid == self.num_frame - self.extra_ref_frames
            if not (key_frame or self.with_prev):
                continue
            if extra_ref_frame:
                feat_prev_iv = self.extract_stereo_ref_feat(imgs[fid])
                continue
            mlp_input = vt.get_mlp_input(sensor2keyegos[0], ego2globals[0], intrins[fid], post_rots[fid], post_trans[fid], bda)
            x, stereo_feat = self.image_encoder(imgs[fid], stereo=True)
            B, N, C, H, W = x.shape
            metas = dict(k2s_sensor=curr2adjsensor[fid], intrins=intrins[fid], post_rots=post_rots[fid],
                         post_trans=post_trans[fid], frustum=vt.cv_frustum.to(x), cv_downsample=4,
                         downsample=vt.downsample, grid_config=vt.grid_config, cv_feat_list=[feat_prev_iv, stereo_feat])
            out = vt.depth_net(x.view(B * N, C, H, W), mlp_input, metas)
            depth, tran_feat = vt.depthnet_tail(out)                   # view_transformer.py:797-801 (HIP)
            frames.append(dict(depth=depth, tran_feat=tran_feat, sensor2keyego=sensor2keyegos[fid], intrin=intrins[fid],
                               post_rot=post_rots[fid], post_tran=post_trans[fid], bda=bda))
            feat_prev_iv = stereo_feat
        return frames[::-1]

    # ---- bevdet_occ.py:167-269: images -> encoder output.  Returns ([x (B,C,Z,Y,X) view], depth of the key frame).
    @torch.no_grad()
    def extract_img_feat(self, img_inputs, img_metas=None, **kwargs):
        frames = self.lift_inputs_from_images(img_inputs)
        x_cl = self._ranged(lambda: as_f32(self.extract_bev_feat_cl(frames)))
        return [x_cl.permute(0, 4, 1, 2, 3)], frames[0]['depth']

    # ---- bevdet.py:139-175: the test-time entry the runner calls (`model(return_loss=False, **data)`)
    def forward_test(self, points=None, img_metas=None, img_inputs=None, **kwargs):
        for var, name in [(img_inputs, 'img_inputs'), (img_metas, 'img_metas')]:
            if not isinstance(var, list):
                raise TypeError('{} must be a list, but got {}'.format(name, type(var)))
        if len(img_inputs) != len(img_metas):
            raise ValueError('num of augmentations ({}) != num of image meta ({})'.format(len(img_inputs), len(img_metas)))
        if not isinstance(img_inputs[0][0], list):
            points = [points] if points is None else points
            return self.simple_test(points[0], img_metas[0], img_inputs[0], **kwargs)
        raise NotImplementedError('aug_test is not implemented by the reference either (bevdet.py:177-179)')

    def forward(self, return_loss=True, **kwargs):
        """base.py:47-62"""
        if return_loss:
            return self.forward_train(**kwargs)
        return self.forward_test(**kwargs)

    # ---- the runner-facing API of mmdet 2.24.0 BaseDetector (mmdet/models/detectors/base.py; third-party, not in the tree, restated
    # from its published code): tools/train.py:244 calls model.init_weights() after build_model and mmcv's EpochBasedRunner calls
    # model.train_step(data, optimizer) / val_step on every iteration
    def init_weights(self):
        """mmcv BaseModule.init_weights applies `init_cfg`; the PreWorld configs give none for these modules, so the
        constructors' default initialisation stands (checkpoints are loaded afterwards by the runner / load_from)"""
        for m in self.children():
            if hasattr(m, 'init_weights') and m is not self:
                m.init_weights()

    @staticmethod
    def _parse_losses(losses):
        """dict of loss tensors / lists of tensors -> (total loss = sum of the entries whose key contains 'loss', log_vars of
        python floats averaged over the ranks of an initialised process group)"""
        from collections import OrderedDict
        import torch.distributed as dist
        log_vars = OrderedDict()
        for name, value in losses.items():
            if isinstance(value, torch.Tensor):
                log_vars[name] = value.mean()
            elif isinstance(value, list):
                log_vars[name] = sum(v.mean() for v in value)
            else:
                raise TypeError('%s is not a tensor or list of tensors' % name)
        loss = sum(v for k, v in log_vars.items() if 'loss' in k)
        log_vars['loss'] = loss
        for name, value in log_vars.items():
            if dist.is_available() and dist.is_initialized():
                value = value.data.clone()
                dist.all_reduce(value.div_(dist.get_world_size()))
            log_vars[name] = value.item()
        return loss, log_vars

    def train_step(self, data, optimizer=None):
        losses = self(**data)
        loss, log_vars = self._parse_losses(losses)
        return dict(loss=loss, log_vars=log_vars, num_samples=len(data['img_metas']))

    def val_step(self, data, optimizer=None):
        return self.train_step(data, optimizer)

    def forward_train(self, points=None, img_metas=None, img_inputs=None, **kwargs):
        """bevdet_occ.py:303-327 (module in .train()): depth loss + `loss_occ` on the predicter's logits.  `loss_occ` is built by
        mmdet's registry in the reference (third-party, not in the tree); the configs use
        dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0) = mean softmax cross entropy x loss_weight, which is what
        is implemented here (anything else raises)."""
        if not self.training:
            raise RuntimeError('forward_train expects the module in training mode (model.train())')
        cfg = dict(self.loss_occ_cfg or dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
        if cfg.get('type') != 'CrossEntropyLoss' or cfg.get('use_sigmoid', False) or cfg.get('class_weight') is not None:
            raise NotImplementedError('loss_occ=%r: only the plain softmax CrossEntropyLoss of the released configs is built' % (cfg,))
        prepared = self.prepare_inputs(img_inputs, stereo=True)
        feat_cl, depth = self._bev_feat_train(prepared)
        losses = {'loss_depth': self._lss_depth_loss(depth, prepared, points, kwargs)}
        v = as_f32(self.final_conv.forward_cl(feat_cl)).permute(0, 3, 2, 1, 4)      # (B,X,Y,Z,C) view (:318)
        occ_pred = self.predicter(v) if self.use_predicter else v
        sem = kwargs['voxel_semantics'].long().reshape(-1)
        losses['loss_occ'] = float(cfg.get('loss_weight', 1.0)) * nn.functional.cross_entropy(
            occ_pred.reshape(-1, self.num_classes), sem, reduction='mean')
        return losses

    def _lss_depth_loss(self, depth, prepared, points, kwargs):
        """The LSS depth term of the three forward_trains.  With only `gt_depth=` (the reference's dense maps): get_depth_loss, as
        before.  With `gt_depth_labels=` ((B*N,h,w) int32, e.g. from transforms.PointToMultiViewDepth(labels_downsample=...)), or
        with the sweep itself, `points=` and `lidar2img=` (B,N,4,4): labels and loss on the device (pw_depth_sup.hip) -- no dense
        map, no host synchronisation.  points: a list of B (P_b, >=3) tensors, or one tensor with `points_offsets=`."""
        vt = self.img_view_transformer
        labels = kwargs.get('gt_depth_labels')
        if labels is None and points is not None and kwargs.get('lidar2img') is not None:
            labels = vt.get_depth_labels(points=points, lidar2img=kwargs['lidar2img'], post_rots=prepared[4][0],
                                         post_trans=prepared[5][0], offsets=kwargs.get('points_offsets'))
        if labels is None:
            return vt.get_depth_loss(kwargs['gt_depth'], depth)
        return vt.get_depth_loss_from_labels(labels, depth)

    # ---- the frame loop of the training step (shared by the three detectors)
    def _bev_feat_train(self, img_inputs):
        """bevdet_occ.py:167-269 in training: the frame loop of extract_img_feat with the KEY frame under autograd and the
        adjacent / stereo-reference frames under no_grad (:229-238), each frame through image encoder -> DepthNet -> voxel
        pooling (ops.bev_pool_v2, backward = pw_bev_pool_v2_backward) -> pre_process_net; [adjacent, key] concat; encoder +
        neck.  Returns (channels-last (B,Z,Y,X,C) features, depth of the key frame)."""
        imgs, sensor2keyegos, ego2globals, intrins, post_rots, post_trans, bda, curr2adjsensor = img_inputs
        vt = self.img_view_transformer
        feats, depth_key, feat_prev_iv = [], None, None
        for fid in range(self.num_frame - 1, -1, -1):
            key_frame = fid == 0
            extra_ref_frame = fid == self.num_frame - self.extra_ref_frames
            if not (key_frame or self.with_prev):
                continue
            with torch.enable_grad() if key_frame else torch.no_grad():
                if extra_ref_frame:
                    feat_prev_iv = self.extract_stereo_ref_feat(imgs[fid])
                    continue
                mlp_input = vt.get_mlp_input(sensor2keyegos[0], ego2globals[0], intrins[fid], post_rots[fid], post_trans[fid], bda)
                x, stereo_feat = self.image_encoder(imgs[fid], stereo=True)
                metas = dict(k2s_sensor=curr2adjsensor[fid], intrins=intrins[fid], post_rots=post_rots[fid],
                             post_trans=post_trans[fid], frustum=vt.cv_frustum.to(x), cv_downsample=4, downsample=vt.downsample,
                             grid_config=vt.grid_config, cv_feat_list=[feat_prev_iv, stereo_feat])
                bev, depth = vt([x, sensor2keyegos[fid], ego2globals[fid], intrins[fid], post_rots[fid], post_trans[fid], bda,
                                 mlp_input], metas)
                bev_cl = to_channels_last_3d(bev)
                if self.pre_process:
                    bev_cl = as_f32(self.pre_process_net.forward_cl(bev_cl)[0])
                feats.append(bev_cl)
                if key_frame:
                    depth_key = depth
                feat_prev_iv = stereo_feat
        key = feats[-1]
        if not self.with_prev:
            feats = [key.new_zeros(key.shape[:-1] + (key.shape[-1] * self.num_adj,)), key]
        x = torch.cat(feats, dim=-1)                                  # [adjacent ..., key] (:266), channels-last
        return as_f32(self.bev_encoder_cl(x)), depth_key


    # ---- activation ranges of the split-fp16 path (ops.RangeCtx; include/preworld_hip.h "RANGE SLOTS")
    def _ranged(self, fn):
        """Run one inference pass fn() with its h2 tensors' exponents calibrated to the data: under this detector's own
        RangeCtx, repeated until the recorded maxima sit inside the window (one pass once the exponents fit; the check is
        one 2 KB D2H copy).  Inside an outer ops.use_range scope (pipeline.CapturedSample, the sharded harness) the owner of
        that scope calibrates and fn() simply runs."""
        if precision() != 'h2' or ops.current_range() is not None:
            return fn()
        dev = next(self.parameters()).device
        ctx = self.__dict__.get('_range_ctx')
        if ctx is None or ctx.device != dev:
            ctx = self.__dict__['_range_ctx'] = ops.RangeCtx(dev)
        return ops.ranged(fn, ctx)

    # ---- bevdet.py:52-58
    def bev_encoder_cl(self, x_cl, out_h2=False):
        h2 = precision() == 'h2'
        feats = self.img_bev_encoder_backbone.forward_cl(x_cl, keep_h2=h2)
        return self.img_bev_encoder_neck.forward_cl(feats, out_h2=out_h2)

    # ---- bevdet_occ.py:141-165 minus the image encoder / DepthNet
    def lift_frame_cl(self, depth, tran_feat, sensor2keyego, intrin, post_rot, post_tran, bda, out=None, out_h2=False):
        """one frame: voxel pooling + pre_process_net -> channels-last (B,Z,Y,X,C) fp32 (or ops.H2 with out_h2), written
        into `out` (a channel slice of the [adjacent, key] buffer) when given"""
        vt = self.img_view_transformer
        B, N = sensor2keyego.shape[:2]
        H, W = depth.shape[-2:]
        inp = [depth.new_empty(B, N, 1, H, W), sensor2keyego, None, intrin, post_rot, post_tran, bda]
        h2 = precision() == 'h2' and vt.out_channels % 32 == 0
        x = vt.pool_cl(inp, depth, tran_feat, out_h2=h2)
        if self.pre_process:
            return self.pre_process_net.forward_cl(x, out_last=out, keep_h2=out_h2)[0]
        if out is not None:
            if out_h2:                                      # into the destination's storage, under ITS range slot
                return ops.f32_to_h2(as_f32(x), out=out)
            dst = out.buf if isinstance(out, ops.H2) else out
            dst.copy_(as_f32(x))
            return dst
        return x if isinstance(x, ops.H2) == out_h2 else (ops.f32_to_h2(x) if out_h2 else as_f32(x))

    # ---- bevdet_occ.py:167-269 (frame loop, [adj, key] concat, with_prev=False -> zeros)
    def extract_bev_feat_cl(self, frames, out_h2=False, side_work=None):
        """frames: list ordered [key, adj, ...] of dicts(depth, tran_feat, sensor2keyego, intrin,
        post_rot, post_tran, bda).  Returns the bev_encoder output, channels-last (B,Z,Y,X,C).  side_work: an optional callable
        that depends on neither frame; it is run once behind the adjacent frame's lift (on the side stream when the lifts fork)."""
        # channel order [adjacent ..., key] (bevdet_occ.py:266): every frame's pre_process output is
        # written straight into its channel slice of ONE buffer (row stride n*C), no torch.cat copy.
        # In the 'h2' precision that buffer is in split-fp16 storage (an all-zero slice is zeros there too).
        f0 = frames[0]
        B = f0['sensor2keyego'].shape[0]
        _, _, size = self.img_view_transformer._grid()
        C = self.img_view_transformer.out_channels
        n = self.num_adj + 1
        h2 = precision() == 'h2' and C % 32 == 0
        x = torch.empty(B, size[2], size[1], size[0], n * C, device=f0['depth'].device, dtype=torch.float32)
        xslot = ops.new_slot(x.device) if h2 else None      # ONE range slot for the whole buffer: every frame is written under it

        def sl(lo, hi):
            return ops.H2(x[..., lo:hi], xslot) if h2 else x[..., lo:hi]
        # The frames' lift chains (voxel index, sort, pooling, pre_process_net) are independent until the encoder reads the
        # buffer: the adjacent frames run on a side stream (fork / join; captured into the hipGraph as two branches), so that
        # one frame's small latency-bound LSS kernels hide under the other's convolutions.  PW_LIFT_STREAMS=0: one stream.
        # (not on the first call: the packed / folded weights both branches share are built lazily by torch ops on whichever
        # stream reaches them first, and the other branch would read them without an event dependency -- ADVICE r02)
        fork = (x.is_cuda and not torch.is_grad_enabled() and self.with_prev and len(frames) > 1
                and os.environ.get('PW_LIFT_STREAMS', '1') != '0' and self.__dict__.get('_lift_warm', False))
        if fork:
            main = torch.cuda.current_stream(x.device)
            side = self.__dict__.get('_lift_stream')
            if side is None or side.device != x.device:
                side = self.__dict__['_lift_stream'] = torch.cuda.Stream(x.device)
            side.wait_stream(main)                        # x is allocated, the inputs are ready
        for j in range(self.num_adj):                      # adjacent frame j+1 sits left of frame j
            lo, hi = (n - 2 - j) * C, (n - 1 - j) * C
            if self.with_prev and len(frames) > 1 + j:
                if fork:
                    with torch.cuda.stream(side):
                        self.lift_frame_cl(out=sl(lo, hi), out_h2=h2, **frames[1 + j])
                else:
                    self.lift_frame_cl(out=sl(lo, hi), out_h2=h2, **frames[1 + j])
            else:
                x[..., lo:hi].zero_()
        # work that depends on neither frame (PreWorld4DTraj: the forecast's per-sample prologue, a one-block 20 us kernel that would
        # otherwise run alone in front of the forecast) rides on the side stream behind the adjacent frame's lift
        if side_work is not None:
            if fork:
                with torch.cuda.stream(side):
                    side_work()
            else:
                side_work()
        self.lift_frame_cl(out=sl((n - 1) * C, n * C), out_h2=h2, **f0)
        if fork:
            main.wait_stream(side)
        self.__dict__['_lift_warm'] = True
        return self.bev_encoder_cl(ops.H2(x, xslot) if h2 else x, out_h2=out_h2)

    def extract_voxel_feat_cl(self, frames, out_h2=False, side_work=None):
        """... followed by final_conv: conv + bias + ReLU (preworld.py:72-79), channels-last (B,Z,Y,X,out_dim); out_h2: keep
        the result in h2 storage (ops.H2) for the split-fp16 forecast / OccHead kernels."""
        return self.final_conv.forward_cl(self.extract_bev_feat_cl(frames, out_h2=precision() == 'h2', side_work=side_work),
                                          out_h2=out_h2 and precision() == 'h2')

    # ---- bevdet_occ.py:281-301: final_conv -> predicter MLP -> argmax(softmax) (softmax is monotone: argmax of logits)
    @torch.no_grad()
    def simple_test_from_lift(self, frames, **kwargs):
        return self._ranged(lambda: self._simple_test_from_lift(frames, **kwargs))

    def _predicter_packed(self):
        p = self.predicter
        return self._derived.get('pred', (p[0], p[2]), lambda: ops.pack_mlp_blocks([p]))

    def _simple_test_from_lift(self, frames, **kwargs):
        v = self.extract_voxel_feat_cl(frames)
        if self.use_predicter:
            v = ops.attr_mlp(v, self._predicter_packed(), final_softplus=False)[..., :self.num_classes]
        occ = v.argmax(-1).to(torch.uint8).permute(0, 3, 2, 1)         # (B,X,Y,Z)
        return [occ.squeeze(0)]

    def simple_test(self, points, img_metas, img=None, rescale=False, **kwargs):
        res = self.simple_test_from_lift(self.lift_inputs_from_images(self.prepare_inputs(img, stereo=True)))
        return [r.cpu().numpy().astype(np.uint8) for r in res]


def _zero_weight_of(mlp):
    """the zero-weight `loss_sup_*` term of an attribute MLP that nothing else consumes (fine-tune configs: if_render=False): the
    reference evaluates the MLP on all 640 000 voxels, a soft-target cross entropy, multiplies by 0. and back-propagates zeros through
    both; value and gradients are known without any of it (round 4: -3 ms of the voxel-side training step).  One behavioural
    difference, by design: a non-finite MLP output makes the reference's term NaN (0. * inf); this term stays 0."""
    ps = [p for p in mlp.parameters() if p.requires_grad]
    if not ps:                                     # a frozen MLP: the reference's `loss_sup * 0.` is a plain zero there too
        any_t = next(iter(mlp.parameters()), None)
        any_t = next(iter(mlp.buffers()), None) if any_t is None else any_t
        return torch.zeros((), device=any_t.device if any_t is not None else None)
    return _ZeroTerm.apply(*ps)


class _ZeroTerm(torch.autograd.Function):
    """0. * (anything finite computed from the parameters): value 0, zero-valued gradients for every parameter"""

    @staticmethod
    def forward(ctx, *ps):
        ctx.meta = [(p.shape, p.dtype, p.device) for p in ps]
        return torch.zeros((), device=ps[0].device)

    @staticmethod
    def backward(ctx, g):
        return tuple(torch.zeros(s, dtype=d, device=dev) for s, d, dev in ctx.meta)


def _zero_weight(pred):
    """`CrossEntropyLoss()(pred, ones) * 0.` of preworld.py:120-127 / :305-307 -- a zero-weight term whose only job is to keep the
    attribute MLPs in the autograd graph (their parameters get zero-valued gradients).  Its value is 0 and its gradient is 0 for any
    finite prediction, and so are this sum's: the soft-target cross entropy over 640 000 x {17, 3, 1} values (log-softmax and four
    reductions, forward and backward: 3 ms of the training step) is not evaluated."""
    return pred.sum() * 0.


class _PreWorldCommon(BEVStereo4DOCC):
    """What preworld.py:24-120 and preworld_temporal_traj.py:27-118 share: final_conv (out_dim), the three attribute
    MLPs, nerf_head, occupancy_head and the flags."""

    def __init__(self, out_dim=32, dataset_type='Nuscenes', num_classes=18, dense_nerf_head=None, nerf_head=None,
                 occupancy_head=None, test_threshold=8.5, use_lss_depth_loss=True, use_3d_loss=True, if_pretrain=False,
                 if_render=True, if_post_finetune=False, weight_voxel_ce=0.0, weight_voxel_sem_scal=0.0,
                 weight_voxel_geo_scal=0.0, weight_voxel_lovasz=0.0, empty_idx=17, use_focal_loss=True,
                 balance_cls_weight=True, final_softplus=True, **kwargs):
        kwargs.pop('use_predicter', None)
        super().__init__(use_predicter=False, out_dim=out_dim, num_classes=num_classes, **kwargs)
        if dataset_type != 'Nuscenes':
            raise NotImplementedError('dataset_type=%r: the released PreWorld configs are nuScenes only' % dataset_type)
        self.dataset_type, self.test_threshold = dataset_type, test_threshold
        self.use_lss_depth_loss, self.use_3d_loss = use_lss_depth_loss, use_3d_loss
        self.balance_cls_weight, self.final_softplus = balance_cls_weight, final_softplus
        self.if_pretrain, self.if_render, self.if_post_finetune = if_pretrain, if_render, if_post_finetune
        self.empty_idx = empty_idx
        C = self.img_view_transformer.out_channels
        self.final_conv = ConvModule3d(C, out_dim, 3, stride=1, padding=1, bias=True, conv_cfg=dict(type='Conv3d'))
        self.density_mlp = nn.Sequential(nn.Linear(out_dim, out_dim * 2), nn.Softplus(), nn.Linear(out_dim * 2, 2),
                                         *([nn.Softplus()] if final_softplus else []))
        self.semantic_mlp = nn.Sequential(nn.Linear(out_dim, out_dim * 2), nn.Softplus(),
                                          nn.Linear(out_dim * 2, num_classes - 1))
        self.color_mlp = nn.Sequential(nn.Linear(out_dim, out_dim * 2), nn.Softplus(), nn.Linear(out_dim * 2, 3))
        self.nerf_head = builder.build(nerf_head, 'NerfHead')
        # the hot-path benches build the detector without a head config: the OccHead of the released configs
        oh = occupancy_head or dict(in_channels=[out_dim], out_channel=num_classes, norm_cfg=dict(type='SyncBN'),
                                    soft_weights=True)
        self.occupancy_head = builder.build(oh, 'OccHead')
        self.weight_voxel_ce, self.weight_voxel_sem_scal = weight_voxel_ce, weight_voxel_sem_scal
        self.weight_voxel_geo_scal, self.weight_voxel_lovasz = weight_voxel_geo_scal, weight_voxel_lovasz
        self.use_focal_loss = use_focal_loss
        if use_focal_loss:
            self.focal_loss = builder.build(dict(type='CustomFocalLoss'))

    def _attr_packed(self):
        mods = (self.density_mlp, self.semantic_mlp, self.color_mlp)
        return self._derived.get('attr', [m[i] for m in mods for i in (0, 2)], lambda: ops.pack_attr_mlp(*mods))

    # ---- preworld_temporal_traj.py:231-236: density / semantic / color MLPs, fused
    def attributes_cl(self, v_cl):
        """v_cl (B,Z,Y,X,C) -> packed grid (B,Z,Y,X,24): [0:2] density_prob, [2:19] semantic,
        [19:22] color.  `grid[..., 0]` is the reference's `density`."""
        return ops.attr_mlp(v_cl, self._attr_packed(), final_softplus=len(self.density_mlp) == 4)

    # ---- preworld_temporal_traj.py:237-250: occupancy from density threshold + semantic argmax
    def attribute_decode(self, grid):
        dens = grid[..., 0]
        sem = grid[..., 2:19].argmax(-1)
        occ = torch.where(dens > self.test_threshold, sem, torch.full_like(sem, self.num_classes - 1))
        return occ.to(torch.uint8)

    def _voxel_losses_train(self, voxel_feats_cl, interval=None, voxel_semantics=None, rays=None, **kwargs):
        """preworld.py:237-303 / preworld_temporal_traj.py:392-434 from a state's features: OccHead per batch element, loss_voxel /
        the zero-weight `loss_sup_*` terms, optional render losses.  voxel_feats_cl: (B,Z,Y,X,C) channels-last.  interval: None
        for the single-time-step detector, else the state index (keys get the reference's `_{k}s` suffix)."""
        from . import losses as L, train
        sfx = '' if interval is None else '_%ds' % interval
        voxel_semantics = kwargs['voxel_semantics'] if voxel_semantics is None else voxel_semantics
        head = self.occupancy_head
        nb = voxel_feats_cl.shape[0]                 # (a batch slice of an autograd tensor costs a zero fill + copy of it backward)
        # pre-training (if_post_finetune=False): the head only feeds `loss_sup_voxel = CE x 0.` (preworld.py:130-135).  Its forward still
        # runs -- the BatchNorms see every batch and their running statistics move, as in the reference -- but outside autograd: the
        # backward through conv / BN / 1x1 layers would multiply zeros (round 6; value and zero-valued parameter gradients are restored
        # below, like the attribute MLPs' zero-weight terms of round 4)
        with torch.enable_grad() if self.if_post_finetune else torch.no_grad():
            parts = [train.occ_head_forward(head, voxel_feats_cl if nb == 1 else voxel_feats_cl[b:b + 1], transposed=True) for b in range(nb)]
        logits = parts[0] if len(parts) == 1 else torch.cat(parts, 0)               # (B,Z,Y,X,18); per batch element as :240-247
        occ_preds = logits.permute(0, 4, 3, 2, 1)                                   # (B,18,X,Y,Z) view, as :240-247 stacks them
        # the attribute MLPs act per voxel: applied to the (Z,Y,X) buffer as 1x1x1 convs on the MFMA kernels (train.mlp_cl), their
        # outputs viewed as the reference's (B,X,Y,Z,.) (:238)
        xyz = lambda t: t.permute(0, 3, 2, 1, 4)
        need_sem = self.if_render or (self.if_pretrain and interval is None)
        density = semantic = color = None
        if self.if_render:
            density_prob = xyz(train.mlp_cl(self.density_mlp, voxel_feats_cl))
            density, color = density_prob[..., 0], xyz(train.mlp_cl(self.color_mlp, voxel_feats_cl))
        if need_sem:
            semantic = xyz(train.mlp_cl(self.semantic_mlp, voxel_feats_cl))
        out = {}
        cw17 = getattr(self, '_cw17', None)                           # the 17 class weights, made once per device (no per-call H2D copy)
        if cw17 is None or cw17.device != occ_preds.device:
            cw17 = self._cw17 = torch.from_numpy(1.0 / np.log(NUSC_CLASS_FREQUENCIES[:17] + 0.001)).float().to(occ_preds.device)
        if self.if_post_finetune:
            lv = L.loss_voxel(occ_preds, voxel_semantics, cw17, camera_mask=None, empty_idx=self.empty_idx,
                              use_focal_loss=self.use_focal_loss, weight_voxel_ce=self.weight_voxel_ce,
                              weight_voxel_sem_scal=self.weight_voxel_sem_scal, weight_voxel_geo_scal=self.weight_voxel_geo_scal,
                              weight_voxel_lovasz=self.weight_voxel_lovasz, focal_loss=getattr(self, 'focal_loss', None))
            out.update({k + sfx: v for k, v in lv.items()})
        else:
            cw = torch.cat([cw17, torch.zeros(1, device=cw17.device)]).to(occ_preds)
            out['loss_sup_voxel' + sfx] = L.CE_ssc_loss(occ_preds, voxel_semantics, cw, 255) * 0. + _zero_weight_of(head)
        if self.if_render:
            extra = {} if interval is None else dict(if_temporal=True, interval=interval)
            out.update(self.nerf_head(density, semantic, color, if_pretrain=self.if_pretrain, dataset_type=self.dataset_type,
                                      rays=kwargs['rays'] if rays is None else rays, bda=kwargs.get('bda'), **extra))
        else:                                                         # loss_sup (:120-127): zero weight, keeps the MLPs in the graph
            for mlp, pred, tag in ((self.semantic_mlp, semantic, 'semantic'), (self.color_mlp, color, 'color'), (self.density_mlp, density, 'density')):
                out['loss_sup_%s%s' % (tag, sfx)] = _zero_weight(pred) if pred is not None else _zero_weight_of(mlp)
        if self.if_pretrain and interval is None:                      # preworld.py:305-307 (the temporal detector has no such term)
            n = self.num_classes - 1
            out['loss_sup_semantic'] = _zero_weight(semantic)
        return out

    def forward_train_from_feats(self, bev_feat_cl, **kwargs):
        """final_conv -> OccHead -> losses (preworld.py:237-309) from the neck output (B,Z,Y,X,C); what a test without the image
        side drives."""
        return self._voxel_losses_train(as_f32(self.final_conv.forward_cl(bev_feat_cl)), **kwargs)

    def simple_test_captured(self, frames, temporal_ego_states=None, n_steps=None, copy=True):
        """The reference-API result -- {'semantic_occ[_ks]' / 'geo_occ[_ks]': [numpy uint8 (X,Y,Z)]} -- through a hipGraph of the hot path
        that this module captures on first use for the inputs' shapes (pipeline.CapturedSample with the host payload inside the
        graph) and replays afterwards: no per-launch host work and no calibration pass per call.  Every call is range-checked on the
        host copy of the exponent table the replay delivers (run_checked: a sample outside the calibrated window is re-calibrated
        eagerly and replayed once).  Opt-in: `net.capture_replay = True` routes simple_test() here (round 6; the eager entry pays
        ~60 launches of host work and its per-call calibration sync -- bench.py `extra.dropin_simple_test`).  PreWorld4DTraj passes its
        ego states (B,1,21) and decodes n_steps (default 6) forecast states; PreWorld has neither.  copy=False returns views of the
        pinned buffer the next call overwrites."""
        from .pipeline import CapturedSample
        temporal = hasattr(self, 'forecast_cl')
        n_steps = (6 if n_steps is None else n_steps) if temporal else 0
        ego = temporal_ego_states if temporal else frames[0]['bda'].new_zeros(1)          # (CapturedSample keeps a static copy)
        key = tuple((k, tuple(v.shape), v.dtype, str(v.device), bool(getattr(v, '_pw_channels_last', False)))
                    for f in frames for k, v in sorted(f.items())) + (n_steps,)
        cache = self.__dict__.setdefault('_captured', {})
        cap = cache.get(key)
        if cap is None:
            if len(cache) >= 4:                                         # a handful of input shapes at most (static buffers are ~1.5 GB each)
                cache.pop(next(iter(cache)))
            cap = cache[key] = CapturedSample(self, frames, ego, n_steps=n_steps, d2h=True)
        cap.run_checked(frames, ego)
        host = cap.host.numpy()
        if copy:
            host = host.copy()
        return {k: [host[i]] for i, k in enumerate(cap.host_keys)}

    # ---- rendered camera views of the predicted state(s)
    def _render_head(self):
        """the NerfHead whose scene constants and sample table the views use: the model's own, or (a post-finetune config carries
        none) one with the released geometry of the view transformer's grid (configs/preworld/nuscenes/*-pretrain.py nerf_head)"""
        if self.nerf_head is not None:
            return self.nerf_head
        head = self.__dict__.get('_view_head')
        if head is None:
            from .modules import NerfHead
            gc = self.img_view_transformer.grid_config
            pcr = [gc['x'][0], gc['y'][0], gc['z'][0], gc['x'][1], gc['y'][1], gc['z'][1]]
            head = self.__dict__['_view_head'] = NerfHead(point_cloud_range=pcr, voxel_size=gc['x'][2], radius=39)
        return head

    @torch.no_grad()
    def _render_result(self, res, frames, intrins, sensor2keyegos, image_hw, stride=1, outputs=None, bda=None, **kw):
        """res: what simple_test_from_lift returned.  One view set per state, keyed '<output><suffix>' with the suffix of the state's
        `semantic_occ<suffix>` key.  Pre-train models (if_post_finetune=False): the state's features -> attr_mlp -> packed grid ->
        the soft renderer.  Post-finetune models: the state's uint8 grid from the OccHead, still on the device -> label mode."""
        head = self._render_head()
        if bda is None:
            bda = frames[0]['bda'].reshape(-1, 3, 3)[0]
        bda = bda.cpu()                      # ONE read-back per call (the scene constants are host arguments of the kernel), not one per state
        if outputs is None:
            outputs = ('depth', 'cls') if self.if_post_finetune else ('depth', 'cls', 'color')
        names = [k for k in res if k.startswith('semantic_occ')]
        out = {}
        for i, name in enumerate(names):
            sfx = name[len('semantic_occ'):]
            if self.if_post_finetune:
                views = head.render_label_views(res[name][0], intrins, sensor2keyegos, image_hw, bda=bda, stride=stride,
                                                empty_idx=self.empty_idx, outputs=outputs, **kw)
            else:
                f = res['voxel_feats'][i]
                grid = self.attributes_cl(ops.h2_to_f32(f) if isinstance(f, ops.H2) else f)[0]
                views = head.render_views(grid, intrins, sensor2keyegos, image_hw, bda=bda, stride=stride, outputs=outputs, **kw)
            out.update({k + sfx: v for k, v in views.items()})
        return out

    @staticmethod
    def _to_numpy(res):
        """the reference's payload: every grid a numpy uint8 (X,Y,Z) array (one D2H copy for all of them)"""
        keys = [k for k in res if k.startswith(('semantic_occ', 'geo_occ'))]
        stack = torch.stack([res[k][0] for k in keys]).cpu().numpy().astype(np.uint8)
        return {k: [stack[i]] for i, k in enumerate(keys)}


class PreWorld(_PreWorldCommon):
    """Drop-in for mmdet3d/models/detectors/preworld.py:23-226 (inference): `simple_test` returns
    {'semantic_occ': [uint8 (X,Y,Z)], 'geo_occ': [uint8 (X,Y,Z)]} for batch element 0, through either the density-threshold +
    semantic-MLP decode (:173-194) or the OccHead decode (:196-221, `if_post_finetune=True`)."""

    @torch.no_grad()
    def simple_test_from_lift(self, frames, want_logits=False, **kwargs):
        return self._ranged(lambda: self._simple_test_from_lift(frames, want_logits=want_logits, **kwargs))

    def _simple_test_from_lift(self, frames, want_logits=False, **kwargs):
        v0 = self.extract_voxel_feat_cl(frames, out_h2=self.if_post_finetune)   # (B,Z,Y,X,C); ops.H2 on the split-fp16 path
        res = {'voxel_feats': [v0]}
        if not self.if_post_finetune:
            occ = self.attribute_decode(self.attributes_cl(v0)).permute(0, 3, 2, 1)
            geo = torch.where(occ != self.num_classes - 1, torch.zeros_like(occ), torch.full_like(occ, self.num_classes - 1))
        else:
            out = self.occupancy_head.decode_cl(v0, want_logits=want_logits, transposed=True, want_geo=True)
            occ, geo = out[0].permute(0, 3, 2, 1), out[-1].permute(0, 3, 2, 1)
            if want_logits:
                res['logits'] = [out[1]]
        res['semantic_occ'] = [occ[0]]
        res['geo_occ'] = [geo[0]]
        return res

    def render_forecast(self, frames, intrins, sensor2keyegos, image_hw, stride=1, outputs=None, **kw):
        """The single predicted state as the cameras would see it: {'depth', 'cls', 'color', ...} -> (V,h,w[,3]) device tensors
        (_render_result; NerfHead.render_views / render_label_views).  intrins (V,3,3), sensor2keyegos (V,4,4), image_hw = (H, W) of
        the source images, every `stride`-th pixel.  simple_test is not involved and returns what it did."""
        return self._render_result(self.simple_test_from_lift(frames), frames, intrins, sensor2keyegos, image_hw, stride, outputs, **kw)

    def simple_test(self, points, img_metas, img=None, rescale=False, **kwargs):
        frames = self.lift_inputs_from_images(self.prepare_inputs(img, stereo=True))
        if getattr(self, 'capture_replay', False) and self.if_post_finetune:
            return self.simple_test_captured(frames)
        return self._to_numpy(self.simple_test_from_lift(frames))

    def forward_train(self, points=None, img_metas=None, img_inputs=None, **kwargs):
        """preworld.py:229-309 for the released nuScenes configs (module in .train()): image side in PyTorch under autograd, the
        voxel side -- pooling backward, pre_process / encoder / neck / final_conv / OccHead with batch-statistics BatchNorm, the
        voxel losses -- on the HIP training kernels (preworld_amd/train.py, losses.py).  Returns the reference's loss dict."""
        if not self.training:
            raise RuntimeError('forward_train expects the module in training mode (model.train())')
        prepared = self.prepare_inputs(img_inputs, stereo=True)
        feat_cl, depth = self._bev_feat_train(prepared)
        out = self.forward_train_from_feats(feat_cl, bda=prepared[6], **kwargs)
        if self.use_lss_depth_loss:
            out['loss_lss_depth'] = self._lss_depth_loss(depth, prepared, points, kwargs)
        return out


class PreWorld4DTraj(_PreWorldCommon):
    """Drop-in for mmdet3d/models/detectors/preworld_temporal_traj.py:26-370 (inference): 0 s state + 6 recursive
    state-conditioned forecasting steps -> `semantic_occ_{k}s` / `geo_occ_{k}s`, k = 0..6 (post-finetune branch) or
    0, 2..7 (density / semantic MLP branch, :294).

    simple_test_from_lift() consumes, per frame, the softmaxed depth (B*N,D,H,W) and context features that
    LSSViewTransformerBEVDepth.forward produces at view_transformer.py:798-801 plus the camera tensors, and returns the
    result dict with uint8 (X,Y,Z) torch tensors on the GPU; simple_test() (images in) returns exactly the
    reference's numpy payload with ONE D2H copy instead of the reference's 14 syncs per sample."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        out_dim = self.out_dim
        self.velocity_dim, self.past_frame = 3, 5
        self.plan_head = nn.Sequential(nn.Linear(self.velocity_dim * (self.past_frame + 2), 256),
                                       nn.ReLU(inplace=True), nn.Linear(256, 256),
                                       nn.ReLU(inplace=True), nn.Linear(256, out_dim))
        self.fusion_head = nn.Sequential(nn.Linear(out_dim * 2, out_dim * 4), nn.Softplus(),
                                         nn.Linear(out_dim * 4, out_dim))
        # A20 trajectory branch (train-time only, preworld_temporal_traj.py:134-150)
        self.downscale = DownScaleModule3DCustom(in_dim=out_dim)
        self.ego_fusion_head = nn.Sequential(nn.Linear(out_dim * 5, out_dim * 8), nn.Softplus(),
                                             nn.Linear(out_dim * 8, out_dim * 4), nn.Softplus(),
                                             nn.Linear(out_dim * 4, out_dim * 2), nn.Softplus(),
                                             nn.Linear(out_dim * 2, out_dim))
        self.traj_head = nn.Sequential(nn.Linear(out_dim, out_dim * 2), nn.Softplus(),
                                       nn.Linear(out_dim * 2, 2))

    def set_epoch(self, epoch):
        self.curr_epoch = epoch

    # ---- preworld_temporal_traj.py:457-470: ego-feature update + 2-D waypoint from one fused state
    def traj_branch_cl(self, fused_cl, ego_feat):
        """fused_cl (B,Z,Y,X,C) = v + fusion_head([v, e]); ego_feat (B,C) = plan_head(ego) ("identity").
        Returns (pred_traj (B,2), fused_ego_feats (B,C))."""
        down = self.downscale.forward_cl(fused_cl)                          # (B, 4C)
        h = torch.cat([ego_feat, down], dim=-1).contiguous()                # (B, 5C)
        efh, th = self.ego_fusion_head, self.traj_head
        for i in (0, 2, 4):
            h = ops.linear_act(h, efh[i].weight.contiguous(), efh[i].bias, 'softplus')
        res = ops.linear_act(h, efh[6].weight.contiguous(), efh[6].bias)
        fused_ego = ego_feat + res
        t = ops.linear_act(fused_ego.contiguous(), th[0].weight.contiguous(), th[0].bias, 'softplus')
        return ops.linear_act(t, th[2].weight.contiguous(), th[2].bias), fused_ego

    def _forecast_weights(self, kind):
        """the fusion head's two weight matrices packed for ops.forecast_steps ('fc') / ops.forecast_steps_h2 ('fc_h2'); its biases go
        to the kernels live"""
        w1, w2 = self.fusion_head[0].weight, self.fusion_head[2].weight
        if kind == 'fc_h2':
            return self._derived.get(kind, (w1, w2), lambda: ops.forecast_pack_h2(w1.float(), w2.float()))
        return self._derived.get(kind, (w1, w2), lambda: ops.forecast_pack(w1.float().contiguous(), w2.float().contiguous()))

    # ---- preworld_temporal_traj.py:329-368: all recursion steps in one kernel
    def forecast_cl(self, v_cl, ego_states, n_steps=6, out_h2=False, prologue=None):
        """v_cl (B,Z,Y,X,C), fp32 tensor or ops.H2; ego_states (B,1,21) (always temporal_ego_states[0], :331).
        Returns states (n_steps,B,Z,Y,X,C) (ops.H2 with out_h2 on the split-fp16 path) and the ego feature (B,32).
        prologue: (ego feature, c1p) of ops.forecast_prologue for THESE ego states if the caller launched it early (handed over
        explicitly -- ADVICE r05: it used to travel through attributes of the shared module and could go stale)."""
        ph, fh = self.plan_head, self.fusion_head
        B = v_cl.shape[0]
        ego = ego_states.reshape(B, -1).float().contiguous()
        plan = [(ph[0].weight.contiguous(), ph[0].bias), (ph[2].weight.contiguous(), ph[2].bias),
                (ph[4].weight.contiguous(), ph[4].bias)]
        if prologue is not None:                                  # launched early by _simple_test_from_lift, on the lift's side stream
            ef, c1p = prologue
            if ef.is_cuda and not torch.cuda.is_current_stream_capturing():     # allocated under the side stream, consumed on this one
                ef.record_stream(torch.cuda.current_stream(ef.device))
                c1p.record_stream(torch.cuda.current_stream(ef.device))
        else:
            ef, _, c1p = ops.forecast_prologue(ego, plan, fh[0].weight.contiguous(), fh[0].bias)
        if precision() == 'h2':
            return ops.forecast_steps_h2(v_cl, B, self._forecast_weights('fc_h2'), c1p, fh[2].bias, n_steps, out_h2=out_h2), ef
        if isinstance(v_cl, ops.H2):
            v_cl = ops.h2_to_f32(v_cl)
        w1p, w2p = self._forecast_weights('fc')
        states = ops.forecast_steps(v_cl, B, w1p, w2p, c1p, fh[2].bias, n_steps)
        return states, ef

    # ---- preworld_temporal_traj.py:212-370 (post-finetune branch) from lifted inputs
    @torch.no_grad()
    def simple_test_from_lift(self, frames, temporal_ego_states, n_steps=6, want_logits=False):
        return self._ranged(lambda: self._simple_test_from_lift(frames, temporal_ego_states, n_steps, want_logits))

    def _simple_test_from_lift(self, frames, temporal_ego_states, n_steps=6, want_logits=False):
        # post-finetune decode: final_conv -> forecast -> OccHead stay in h2 storage end to end on the split-fp16 path
        early, side_work = [], None
        if self.if_post_finetune and n_steps > 0:
            def side_work():                                          # plan_head + the hoisted ego term: depends on the ego state only
                ph, fh = self.plan_head, self.fusion_head
                ego = temporal_ego_states.reshape(temporal_ego_states.shape[0], -1).float().contiguous()
                plan = [(ph[0].weight.contiguous(), ph[0].bias), (ph[2].weight.contiguous(), ph[2].bias), (ph[4].weight.contiguous(), ph[4].bias)]
                ef, _, c1p = ops.forecast_prologue(ego, plan, fh[0].weight.contiguous(), fh[0].bias)
                early.append((ef, c1p))
        v0 = self.extract_voxel_feat_cl(frames, out_h2=self.if_post_finetune, side_work=side_work)      # (B,Z,Y,X,C)
        if not self.if_post_finetune:
            return self._simple_test_attributes(v0, temporal_ego_states, n_steps)
        res = {}
        feats = [v0]
        B = v0.shape[0]
        # OccHead on state 0, then on ALL forecast states in one launch (they are one contiguous (n_steps*B, Z, Y, X, C)
        # buffer): one persistent-kernel prologue and one partial last round of tiles instead of n_steps of each.
        # B == 1 (the reference's test-time batch) on the split-fp16 path: the kernel writes every state's semantic / geo grid
        # straight into a (n_states, 2, X, Y, Z) buffer -- the reference's (X,Y,Z)-contiguous arrays in payload order -- through
        # byte strides, so the host payload needs no transposing gather afterwards (it was a 46 us copy in every step)
        Zd, Yd, Xd = v0.shape[1:4]
        grids = None
        if B == 1 and isinstance(v0, ops.H2) and precision() == 'h2':
            grids = torch.empty(n_steps + 1, 2, Xd, Yd, Zd, device=v0.buf.device, dtype=torch.uint8)
            zyx = lambda t: t.permute(0, 3, 2, 1)                          # (n, X, Y, Z) storage as the kernel's (n, Z, Y, X)  # noqa: E731
            o0 = self.occupancy_head.decode_cl(v0, want_logits=want_logits, transposed=True, want_geo=True,
                                               occ_out=zyx(grids[0:1, 0]), geo_out=zyx(grids[0:1, 1]))
        else:
            o0 = self.occupancy_head.decode_cl(v0, want_logits=want_logits, transposed=True, want_geo=True)
        outs = [o0]
        if n_steps > 0:
            states, _ = self.forecast_cl(v0, temporal_ego_states, n_steps, out_h2=isinstance(v0, ops.H2),
                                         prologue=early[0] if early else None)
            feats += [states[k] for k in range(n_steps)]
            extra = dict(occ_out=zyx(grids[1:, 0]), geo_out=zyx(grids[1:, 1])) if grids is not None else {}
            o = self.occupancy_head.decode_cl(states.view((n_steps * B,) + tuple(v0.shape[1:])), want_logits=want_logits,
                                              transposed=True, want_geo=True, **extra)
            outs += [tuple(t[k * B:(k + 1) * B] for t in o) for k in range(n_steps)]
        logits_all = []
        for k, out in enumerate(outs):
            occ, geo = out[0], out[-1]                                 # geo_occ from the same kernel (:313-319)
            if want_logits:
                logits_all.append(out[1])
            occ_xyz = occ.permute(0, 3, 2, 1)                          # (B,X,Y,Z) view
            geo = geo.permute(0, 3, 2, 1)
            # the reference indexes batch element 0 (:306) and names states 0s..6s (:361)
            res['semantic_occ_%ds' % k] = [occ_xyz[0]]
            res['geo_occ_%ds' % k] = [geo[0]]
        if want_logits:
            res['logits'] = logits_all
        res['voxel_feats'] = feats
        if grids is not None:
            res['grids'] = grids                   # rows in the order of the semantic_occ_* / geo_occ_* keys above
        return res

    # ---- preworld_temporal_traj.py:224-301: density/semantic-MLP decode (if_post_finetune=False).
    # The reference names the future states 2s..7s in this branch (:294) and never emits 1s.
    def _simple_test_attributes(self, v0, temporal_ego_states, n_steps):
        feats = [v0]
        if n_steps > 0:
            states, _ = self.forecast_cl(v0, temporal_ego_states, n_steps)
            feats += [states[k] for k in range(n_steps)]
        res = {}
        for k, f in enumerate(feats):
            occ = self.attribute_decode(self.attributes_cl(f)).permute(0, 3, 2, 1)     # (B,X,Y,Z)
            geo = torch.where(occ != self.num_classes - 1, torch.zeros_like(occ),
                              torch.full_like(occ, self.num_classes - 1))
            name = 0 if k == 0 else k + 1
            res['semantic_occ_%ds' % name] = [occ[0]]
            res['geo_occ_%ds' % name] = [geo[0]]
        res['voxel_feats'] = feats
        return res

    def render_forecast(self, frames, ego, intrins, sensor2keyegos, image_hw, n_steps=6, stride=1, outputs=None, **kw):
        """Every predicted state as the cameras would see it: {'depth_{k}s', 'cls_{k}s', 'color_{k}s', ...}, one (V,h,w[,3]) device
        tensor per state and output, k numbered as simple_test numbers its keys (0..6 post-finetune, 0, 2..7 on the attribute-MLP
        branch).  frames / ego as simple_test_from_lift takes them; intrins (V,3,3), sensor2keyegos (V,4,4), image_hw = (H, W) of
        the source images, every `stride`-th pixel.  Pre-train models render depth / semantics / colour through the soft renderer,
        post-finetune models their uint8 grids through label mode (depth / cls), on the device, before any payload copy."""
        return self._render_result(self.simple_test_from_lift(frames, ego, n_steps), frames, intrins, sensor2keyegos, image_hw, stride,
                                   outputs, **kw)

    # ---- preworld_temporal_traj.py:212-370 with the reference's signature: images + kwargs['temporal_ego_states']
    def set_epoch(self, epoch):                                         # :150-151, called by the reference's epoch hook
        self.curr_epoch = epoch

    def future_intervals(self):
        """:436-446: how many forecast steps are supervised grows with the epoch"""
        ep = getattr(self, 'curr_epoch', 0)
        if self.if_render:
            return [0, 1] if ep <= 2 else list(range(0, min(ep - 1, 6)))
        return [0, 1] if ep <= 4 else list(range(0, min(int((ep - 3) // 2) + 1, 6)))

    def forward_train(self, points=None, img_metas=None, img_inputs=None, **kwargs):
        """preworld_temporal_traj.py:372-530 (module in .train()): the current state's losses, then for every supervised future
        interval one state-conditioned forecast step, the trajectory branch, OccHead + losses on the forecast state -- voxel side
        on the HIP training kernels (preworld_amd/train.py), per-voxel / per-sample MLPs as library GEMMs under torch autograd.
        Returns the reference's loss dict (keys `..._{k}s`)."""
        from . import train
        if not self.training:
            raise RuntimeError('forward_train expects the module in training mode (model.train())')
        prepared = self.prepare_inputs(img_inputs, stereo=True)
        feat_cl, depth = self._bev_feat_train(prepared)
        v = as_f32(self.final_conv.forward_cl(feat_cl))                 # (B,Z,Y,X,C)
        losses = {}
        if self.use_lss_depth_loss:
            losses['loss_lss_depth'] = self._lss_depth_loss(depth, prepared, points, kwargs)
        bda = prepared[6]
        losses.update(self._voxel_losses_train(v, interval=0, voxel_semantics=kwargs['voxel_semantics'],
                                               rays=kwargs.get('rays'), bda=bda))
        for ego_interval in self.future_intervals():
            ego = kwargs['temporal_ego_states'][0]
            ego = ego.reshape(ego.shape[0], ego.shape[-1]).float()
            identity = self.plan_head(ego)                              # (B, out_dim)
            fused = train.fusion_step(self.fusion_head, v, identity)
            down = train.downscale_forward(self.downscale, fused)       # (B, 4 out_dim)
            fused_ego = identity + self.ego_fusion_head(torch.cat([identity, down], dim=-1))
            pred_traj = self.traj_head(fused_ego)
            k = ego_interval + 1
            sem = kwargs['temporal_semantics'][k]['voxel_semantics'] if self.if_post_finetune else kwargs['voxel_semantics']
            rays = kwargs['temporal_rays'][k] if self.if_render else None
            losses.update(self._voxel_losses_train(fused, interval=k, voxel_semantics=sem, rays=rays, bda=bda))
            gt = kwargs['temporal_trajs'][:, k - 1, :]
            losses['loss_traj_%ds' % k] = torch.sum(torch.mean(torch.abs(pred_traj - gt) ** 2, dim=0))        # loss.py:125-131
            v = fused                                                   # recursive (:528)
        return losses

    def simple_test(self, points, img_metas, img=None, rescale=False, **kwargs):
        temporal_ego_states = kwargs['temporal_ego_states'][0]          # (:228,:304)
        frames = self.lift_inputs_from_images(self.prepare_inputs(img, stereo=True))
        if getattr(self, 'capture_replay', False) and self.if_post_finetune:
            return self.simple_test_captured(frames, temporal_ego_states[0])
        return self._to_numpy(self.simple_test_from_lift(frames, temporal_ego_states[0]))

