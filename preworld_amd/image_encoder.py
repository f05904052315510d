"""the image side of the detector in plain torch.nn (no mmcv / mmdet / mmseg), so that a true
image -> occupancy samples/s can be reported.  The reference keeps these modules on PyTorch and by default so does this
package (north_star: "the multi-camera backbone stays on PyTorch-ROCm").  Three things call the HIP library: the DepthNet's
stereo cost volume and its softmax tail (ops.stereo_cost_volume, ops.depthnet_tail -- rows 8f.1) and, only when asked for with
attn_impl='hip', the Swin blocks' shifted-window attention (ops.swin_window_attention, one launch per block between the qkv
and proj Linears -- DESIGN.md 17; forward only, the default 'torch' path is unchanged; attn_impl='hip_grad' adds the kernel's
HIP backward, ops.swin_window_attention_backward -- DESIGN.md 17b) and, with linear_impl='hip' on top of a fused attention, the
blocks' four Linears with both LayerNorms, the GELU and both residual additions fused in (ops.swin_linear, five calls per block
-- DESIGN.md 17c; forward only, the default 'torch' is unchanged; linear_impl='hip_grad' on top of attn_impl='hip_grad' adds their
HIP backward, ops.SwinLinear / ops.swin_linear_backward -- DESIGN.md 17d).  With conv_impl='hip' on FPN_LSS / DepthNet /
ImageBranch a fourth: their stride-1 convolutions with BatchNorm, bias, ReLU and residual fused in (ops.conv2d, one implicit GEMM per
layer over channels-last maps -- DESIGN.md 17e; float32, eval mode and forward only, the default 'torch' is unchanged).

State-dict keys, constructor arguments and forward contracts are the reference's, so released checkpoints load:

  SwinTransformer  mmdet3d/models/backbones/swin.py:680-976 (PatchEmbed :79-171, PatchMerging :174-241, WindowMSA :244-350,
                   ShiftWindowMSA :353-513, SwinBlock :516-592, SwinBlockSequence :595-677); the FFN is mmcv-full 1.6.0's
                   (third-party, not in the tree): layers = Sequential(Sequential(Linear, act, Dropout), Linear, Dropout)
  FPN_LSS          mmdet3d/models/necks/lss_fpn.py:12-101
  DepthNet         mmdet3d/models/necks/view_transformer.py:471-638 (ASPP :323-420, Mlp :423-445, SELayer :448-468);
                   BasicBlock is mmdet 2.24's ResNet block (third-party): conv1, bn1, conv2, bn2, downsample
  get_mlp_input    mmdet3d/models/necks/view_transformer.py:713-734
  ImageBranch      BEVDet.image_encoder (detectors/bevdet.py:34-50), extract_stereo_ref_feat (:573-603) and the per-frame
                   loop of BEVStereo4DOCC.extract_img_feat / prepare_bev_feat (detectors/bevdet_occ.py:142-241) up to the
                   (depth, context) pair the voxel-pooling path starts from.

Inference only (DropPath / Dropout are identities in eval mode; torch.utils.checkpoint is not used)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


# ----------------------------------------------------------------------------------------------- Swin
class PatchEmbed(nn.Module):
    def __init__(self, in_channels=3, embed_dims=128, kernel_size=4, stride=4, norm=True):
        super().__init__()
        self.patch_size = (kernel_size, kernel_size)
        self.projection = nn.Conv2d(in_channels, embed_dims, kernel_size=kernel_size, stride=stride)
        self.norm = nn.LayerNorm(embed_dims) if norm else None

    def forward(self, x):
        H, W = x.shape[2], x.shape[3]
        if H % self.patch_size[0] != 0:
            x = F.pad(x, (0, 0, 0, self.patch_size[0] - H % self.patch_size[0]))
        if W % self.patch_size[1] != 0:
            x = F.pad(x, (0, self.patch_size[1] - W % self.patch_size[1], 0, 0))
        x = self.projection(x)
        self.DH, self.DW = x.shape[2], x.shape[3]
        x = x.flatten(2).transpose(1, 2)
        return self.norm(x) if self.norm is not None else x


class PatchMerging(nn.Module):
    """nn.Unfold grouping (channel-major 2x2 samples), LayerNorm, Linear -- swin.py:174-241."""

    def __init__(self, in_channels, out_channels, stride=2, norm=True):
        super().__init__()
        self.stride, self.out_channels = stride, out_channels
        self.sampler = nn.Unfold(kernel_size=stride, dilation=1, padding=0, stride=stride)
        self.norm = nn.LayerNorm(stride ** 2 * in_channels) if norm else None
        self.reduction = nn.Linear(stride ** 2 * in_channels, out_channels, bias=False)

    def forward(self, x, hw_shape):
        B, L, C = x.shape
        H, W = hw_shape
        x = x.view(B, H, W, C).permute(0, 3, 1, 2)
        if (H % self.stride != 0) or (W % self.stride != 0):
            x = F.pad(x, (0, W % self.stride, 0, H % self.stride))
        x = self.sampler(x).transpose(1, 2)
        x = self.norm(x) if self.norm is not None else x
        return self.reduction(x), ((H + 1) // 2, (W + 1) // 2)


ATTN_IMPLS = ('torch', 'hip', 'hip_grad')


def _check_attn_impl(attn_impl, embed_dims, num_heads, ws):
    """'hip' and 'hip_grad' have no fallback: a config pw_swin_window_attention does not take is refused where the module is built"""
    if attn_impl not in ATTN_IMPLS:
        raise ValueError('attn_impl must be one of %s, got %r' % (ATTN_IMPLS, attn_impl))
    if attn_impl != 'torch':
        from . import ops
        why = ops.swin_attention_supported(embed_dims, num_heads, ws)
        if why is not None:
            raise ValueError("attn_impl=%r: the fused window attention does not support this block: %s" % (attn_impl, why))
    return attn_impl


LINEAR_IMPLS = ('torch', 'hip', 'hip_grad')


def _check_linear_impl(linear_impl, attn_impl, embed_dims, feedforward_channels):
    """'hip' and 'hip_grad' have no fallback: they need the fused attention (the block hands the kernel its qkv directly; 'hip_grad'
    needs attn_impl 'hip_grad', whose backward it is composed with) and Linears that pw_swin_linear takes, and are refused otherwise
    where the module is built"""
    if linear_impl not in LINEAR_IMPLS:
        raise ValueError('linear_impl must be one of %s, got %r' % (LINEAR_IMPLS, linear_impl))
    if linear_impl != 'torch':
        if attn_impl not in ('hip', 'hip_grad'):
            raise ValueError("linear_impl=%r needs attn_impl 'hip' or 'hip_grad', got %r" % (linear_impl, attn_impl))
        if linear_impl == 'hip_grad' and attn_impl != 'hip_grad':
            raise ValueError("linear_impl='hip_grad' needs attn_impl 'hip_grad', got %r" % (attn_impl,))
        from . import ops
        for K, N in ((embed_dims, 3 * embed_dims), (embed_dims, embed_dims), (embed_dims, feedforward_channels),
                     (feedforward_channels, embed_dims)):
            why = ops.swin_linear_supported(K, N)
            if why is not None:
                raise ValueError("linear_impl=%r: the fused Linears do not support this block: %s" % (linear_impl, why))
    return linear_impl


class WindowMSA(nn.Module):
    """attn_impl is recorded here for ShiftWindowMSA, which owns the fused path (it needs the un-partitioned map); forward() is the
    torch path whatever it says."""

    def __init__(self, embed_dims, num_heads, window_size, qkv_bias=True, qk_scale=None, attn_impl='torch'):
        super().__init__()
        self.attn_impl = _check_attn_impl(attn_impl, embed_dims, num_heads, max(window_size))
        self.embed_dims, self.window_size, self.num_heads = embed_dims, window_size, num_heads
        self.scale = qk_scale or (embed_dims // num_heads) ** -0.5
        Wh, Ww = window_size
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * Wh - 1) * (2 * Ww - 1), num_heads))
        seq1 = torch.arange(0, (2 * Ww - 1) * Wh, 2 * Ww - 1)
        seq2 = torch.arange(0, Ww, 1)
        coords = (seq1[:, None] + seq2[None, :]).reshape(1, -1)
        self.register_buffer('relative_position_index', (coords + coords.T).flip(1).contiguous())
        self.qkv = nn.Linear(embed_dims, embed_dims * 3, bias=qkv_bias)
        self.proj = nn.Linear(embed_dims, embed_dims)

    def forward(self, x, mask=None):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        bias = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(N, N, -1)
        bias = bias.permute(2, 0, 1).contiguous()                                 # nH, N, N
        # softmax(q k^T * scale + bias [+ mask]) v  ==  the reference's explicit attention (swin.py:322-344).  Measured
        # on MI355X (Swin-B, 512x1408, fp32): SDPA with the additive term expanded per window 137 ms per sample,
        # SDPA over (B/nW, nW, ...) with a broadcast mask 150 ms, explicit matmul + softmax 154 ms.
        if mask is not None:                                                      # (nW, N, N), 0 / -100
            nW = mask.shape[0]
            add = (bias.view(1, 1, self.num_heads, N, N) + mask.view(1, nW, 1, N, N)).expand(B // nW, nW, self.num_heads, N, N)
            x = F.scaled_dot_product_attention(q, k, v, attn_mask=add.reshape(B, self.num_heads, N, N), scale=self.scale)
        else:
            x = F.scaled_dot_product_attention(q, k, v, attn_mask=bias.unsqueeze(0), scale=self.scale)
        return self.proj(x.transpose(1, 2).reshape(B, N, C))


class ShiftWindowMSA(nn.Module):
    """attn_impl='torch' (default): pad, roll, window partition, WindowMSA, reverse, roll back, crop, as the reference.
    attn_impl='hip': qkv Linear on the (B, H*W, C) tokens, ops.swin_window_attention (one HIP launch that does pad, roll, partition,
    bias, shift mask, softmax and their inverses as index arithmetic), proj Linear; no mask cache, no window-ordered tensor.  The
    kernel is forward only: when autograd would need a backward (grad enabled and the input or a parameter of the attention requires
    grad) 'hip' runs the torch path, so training is unchanged; 'hip_grad' is the mode that trains through the kernel.
    attn_impl='hip_grad': without grad exactly 'hip'; with grad qkv Linear, ops.SwinWindowAttention (the same forward launch, its
    gradient is ops.swin_window_attention_backward: dqkv, and through the un-detached table and qkv.bias the gradients of both
    parameters), proj Linear.  The torch path never runs and no mask is cached; a host tensor is refused, never a fallback.
    Parameters, buffers and state-dict keys are the same for all three."""

    def __init__(self, embed_dims, num_heads, window_size, shift_size=0, qkv_bias=True, qk_scale=None, attn_impl='torch'):
        super().__init__()
        self.window_size, self.shift_size = window_size, shift_size
        self.w_msa = WindowMSA(embed_dims, num_heads, (window_size, window_size), qkv_bias, qk_scale, attn_impl)
        self.attn_impl = self.w_msa.attn_impl
        self._mask_cache = {}

    def set_attn_impl(self, attn_impl):
        m = self.w_msa
        self.attn_impl = m.attn_impl = _check_attn_impl(attn_impl, m.embed_dims, m.num_heads, self.window_size)

    def _needs_backward(self, query):
        return torch.is_grad_enabled() and (query.requires_grad or any(p.requires_grad for p in self.w_msa.parameters()))

    def _forward_hip(self, query, hw_shape):
        from . import ops
        m = self.w_msa
        qkv = m.qkv(query)                                                        # (B, H*W, 3C): Linears act per token
        if not qkv.is_contiguous():
            qkv = qkv.contiguous()
        pad = None if m.qkv.bias is None else m.qkv.bias.detach().to(qkv.dtype)   # qkv of a zero (padded) token
        x = ops.swin_window_attention(qkv, pad, m.relative_position_bias_table.detach().float(), hw_shape[0], hw_shape[1],
                                      m.num_heads, self.window_size, self.shift_size, m.scale)
        return m.proj(x)

    def _forward_hip_grad(self, query, hw_shape):
        from . import ops
        m = self.w_msa
        qkv = m.qkv(query)
        if not qkv.is_contiguous():
            qkv = qkv.contiguous()
        pad = None if m.qkv.bias is None else m.qkv.bias.to(qkv.dtype)            # not detached: it receives dpad_qkv
        x = ops.SwinWindowAttention.apply(qkv, pad, m.relative_position_bias_table.float(), hw_shape[0], hw_shape[1],
                                          m.num_heads, self.window_size, self.shift_size, m.scale)
        return m.proj(x)

    def _partition(self, x):
        B, H, W, C = x.shape
        ws = self.window_size
        x = x.view(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).contiguous()
        return x.view(-1, ws, ws, C)

    def _reverse(self, windows, H, W):
        ws = self.window_size
        B = int(windows.shape[0] / (H * W / ws / ws))
        x = windows.view(B, H // ws, W // ws, ws, ws, -1)
        return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)

    def _shift_mask(self, Hp, Wp, device):
        """Additive attention mask of the shifted configuration (swin.py:422-444): after the cyclic shift the last
        window row / column mixes three source regions per axis (|..unshifted..|ws - ss|ss|); tokens of different
        regions must not attend to each other (-100).  Region ids come from index arithmetic and the (nW, N, N) mask
        is cached per padded size."""
        key = (Hp, Wp, str(device))
        m = self._mask_cache.get(key)
        if m is None:
            ws, ss = self.window_size, self.shift_size
            ih, iw = torch.arange(Hp, device=device), torch.arange(Wp, device=device)
            rh = (ih >= Hp - ws).long() + (ih >= Hp - ss).long()
            rw = (iw >= Wp - ws).long() + (iw >= Wp - ss).long()
            region = (3 * rh[:, None] + rw[None, :]).float().view(1, Hp, Wp, 1)
            mw = self._partition(region).view(-1, ws * ws)
            diff = mw.unsqueeze(1) - mw.unsqueeze(2)
            m = torch.where(diff != 0, torch.full_like(diff, -100.0), torch.zeros_like(diff))
            self._mask_cache[key] = m
        return m

    def forward(self, query, hw_shape):
        if self.attn_impl != 'torch':
            if not self._needs_backward(query):
                return self._forward_hip(query, hw_shape)
            if self.attn_impl == 'hip_grad':
                return self._forward_hip_grad(query, hw_shape)
        B, L, C = query.shape
        H, W = hw_shape
        ws, ss = self.window_size, self.shift_size
        x = query.view(B, H, W, C)
        pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
        if pad_r or pad_b:
            x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b))
        Hp, Wp = H + pad_b, W + pad_r
        mask = None
        if ss > 0:
            x = torch.roll(x, shifts=(-ss, -ss), dims=(1, 2))
            mask = self._shift_mask(Hp, Wp, x.device)
        win = self.w_msa(self._partition(x).view(-1, ws * ws, C), mask=mask)
        x = self._reverse(win.view(-1, ws, ws, C), Hp, Wp)
        if ss > 0:
            x = torch.roll(x, shifts=(ss, ss), dims=(1, 2))
        if pad_r or pad_b:
            x = x[:, :H, :W, :].contiguous()
        return x.view(B, H * W, C)


class FFN(nn.Module):
    """mmcv.cnn.bricks.transformer.FFN (num_fcs=2, add_identity=True): keys layers.0.0.*, layers.1.*"""

    def __init__(self, embed_dims, feedforward_channels):
        super().__init__()
        self.layers = nn.Sequential(nn.Sequential(nn.Linear(embed_dims, feedforward_channels), nn.GELU(), nn.Dropout(0.)),
                                    nn.Linear(feedforward_channels, embed_dims), nn.Dropout(0.))

    def forward(self, x, identity=None):
        return (x if identity is None else identity) + self.layers(x)


class SwinBlock(nn.Module):
    """linear_impl='torch' (default): norm1, attention, residual, norm2, FFN as the reference.
    linear_impl='hip' (needs attn_impl 'hip' or 'hip_grad'): five calls and no token-sized temporary but qkv, the attention output
    and the hidden tensor -- qkv = Linear(LN1(x)); ops.swin_window_attention on that qkv; x1 = x + proj(attn);
    h = GELU(fc1(LN2(x1))); x2 = x1 + fc2(h) (ops.swin_linear, include/preworld_hip_swin_linear.h: the GEMM, and in front of it a
    small launch for the (M, 2) row statistics where the mode has any).  Forward only: when autograd
    would need a backward the block runs exactly what linear_impl='torch' runs.  An fp32 block runs the split-fp16 mode, under
    torch.autocast(bfloat16) the bf16 mode; a block whose residual stream is not float32 (.bfloat16(), .half()) is refused.  The
    packed operands live in a modules.Derived cache keyed on the Linears' and LayerNorms' parameters; parameters, buffers and
    state-dict keys do not depend on linear_impl.
    linear_impl='hip_grad' (needs attn_impl 'hip_grad'): without grad exactly 'hip'.  With grad in float32 the same five calls run as
    autograd Functions (ops.SwinLinear around ops.swin_linear, ops.SwinWindowAttention): the forward gives the same bits, the backward
    is include/preworld_hip_swin_linear_bwd.h, and the torch Linears, LayerNorms and GELU never run.  Saved per token are x, qkv, the
    attention output, x1 and the hidden tensor (10 C; neither LayerNorm output nor the pre-GELU tensor).  Under bf16 autocast with
    grad it does what 'hip' does (the torch path): the gradient kernels are float32 only.  There is no DropPath in this block (as
    with attn_impl='hip_grad'), so none is fused."""

    def __init__(self, embed_dims, num_heads, feedforward_channels, window_size, shift, qkv_bias=True, qk_scale=None,
                 attn_impl='torch', linear_impl='torch'):
        super().__init__()
        self.embed_dims, self.feedforward_channels = embed_dims, feedforward_channels
        self.norm1 = nn.LayerNorm(embed_dims)
        self.attn = ShiftWindowMSA(embed_dims, num_heads, window_size, window_size // 2 if shift else 0, qkv_bias, qk_scale,
                                   attn_impl)
        self.norm2 = nn.LayerNorm(embed_dims)
        self.ffn = FFN(embed_dims, feedforward_channels)
        self.linear_impl = _check_linear_impl(linear_impl, attn_impl, embed_dims, feedforward_channels)
        self._derived = None

    def check_linear_impl(self, linear_impl):
        return _check_linear_impl(linear_impl, self.attn.attn_impl, self.embed_dims, self.feedforward_channels)

    def set_linear_impl(self, linear_impl):
        self.linear_impl = self.check_linear_impl(linear_impl)

    def _needs_backward(self, x):
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _packed(self, dtype):
        """(qkv, proj, fc1, fc2) packed for the mode `dtype`, rebuilt when a Linear's or LayerNorm's parameter changes"""
        from . import ops
        from .modules import Derived
        if self._derived is None:
            self._derived = Derived()
        m, fc1, fc2 = self.attn.w_msa, self.ffn.layers[0][0], self.ffn.layers[1]

        def build():
            return (ops.swin_linear_pack(m.qkv.weight, m.qkv.bias, self.norm1.weight, self.norm1.bias, dtype=dtype),
                    ops.swin_linear_pack(m.proj.weight, m.proj.bias, dtype=dtype),
                    ops.swin_linear_pack(fc1.weight, fc1.bias, self.norm2.weight, self.norm2.bias, dtype=dtype),
                    ops.swin_linear_pack(fc2.weight, fc2.bias, dtype=dtype))
        return self._derived.get('swin_linear_%s' % dtype, (self.norm1, m.qkv, m.proj, self.norm2, fc1, fc2), build)

    def _forward_fused(self, x, hw_shape):
        from . import _lib, ops
        m = self.attn.w_msa
        params = [p for mod in (self.norm1, m.qkv, m.proj, self.norm2, self.ffn) for p in mod.parameters()]
        dtype = torch.float32
        if torch.is_autocast_enabled('cuda'):
            dtype = torch.get_autocast_dtype('cuda')
            if dtype != torch.bfloat16:
                raise _lib.PreworldHipError("SwinBlock(linear_impl='hip'): autocast to %s is not supported, only torch.bfloat16" % dtype)
            if x.dtype == torch.bfloat16:          # under autocast PatchMerging's Linear hands the next stage a bf16 map: the first block
                x = x.float()                      # lifts it (exact) and the stage's residual stream is float32 from there on
        if x.dtype != torch.float32 or any(p.dtype != torch.float32 for p in params):
            raise _lib.PreworldHipError("SwinBlock(linear_impl='hip'): the residual stream and the parameters must be float32 (got x %s); "
                                        "for bf16 run the float32 module under torch.autocast('cuda', torch.bfloat16)" % x.dtype)
        qkv_p, proj_p, fc1_p, fc2_p = self._packed(dtype)
        if not x.is_contiguous():
            x = x.contiguous()
        qkv = ops.swin_linear(x, qkv_p, ln=True, eps=self.norm1.eps)
        # what qkv gives for a zero (padded) token is the Linear's own bias: the LayerNorm's beta is applied in the prologue, not folded
        pad = None if m.qkv.bias is None else m.qkv.bias.detach().to(qkv.dtype)
        a = ops.swin_window_attention(qkv, pad, m.relative_position_bias_table.detach(), hw_shape[0], hw_shape[1], m.num_heads,
                                      self.attn.window_size, self.attn.shift_size, m.scale)
        x = ops.swin_linear(a, proj_p, residual=x)
        h = ops.swin_linear(x, fc1_p, ln=True, eps=self.norm2.eps, act='gelu')
        return ops.swin_linear(h, fc2_p, residual=x)

    def _packed_t(self):
        """(qkv, proj, fc1, fc2) transposed packs for the data gradient: same sources as _packed, so an in-place optimizer step
        rebuilds them with the forward packs"""
        from . import ops
        from .modules import Derived
        if self._derived is None:
            self._derived = Derived()
        m, fc1, fc2 = self.attn.w_msa, self.ffn.layers[0][0], self.ffn.layers[1]
        return self._derived.get('swin_linear_t_%s' % torch.float32, (self.norm1, m.qkv, m.proj, self.norm2, fc1, fc2),
                                 lambda: tuple(ops.swin_linear_pack_transposed(l.weight) for l in (m.qkv, m.proj, fc1, fc2)))

    def _forward_fused_grad(self, x, hw_shape):
        """float32 with grad: the five calls of _forward_fused as autograd Functions (ops.SwinLinear, ops.SwinWindowAttention).  The
        residual additions go through SwinLinear's pass-through output, so every gradient of the residual stream is folded into a
        kernel and autograd adds only the two small contributions to qkv.bias (dpad and the column sums of dqkv)."""
        from . import _lib, ops
        m, fc1, fc2 = self.attn.w_msa, self.ffn.layers[0][0], self.ffn.layers[1]
        params = [p for mod in (self.norm1, m.qkv, m.proj, self.norm2, self.ffn) for p in mod.parameters()]
        if x.dtype != torch.float32 or any(p.dtype != torch.float32 for p in params):
            raise _lib.PreworldHipError("SwinBlock(linear_impl='hip_grad'): the residual stream and the parameters must be float32 (got x %s)"
                                        % x.dtype)
        qkv_p, proj_p, fc1_p, fc2_p = self._packed(torch.float32)
        qkv_t, proj_t, fc1_t, fc2_t = self._packed_t()
        if not x.is_contiguous():
            x = x.contiguous()
        L = ops.SwinLinear.apply
        qkv, x = L(x, m.qkv.weight, m.qkv.bias, self.norm1.weight, self.norm1.bias, None, qkv_p, qkv_t, 'ln', self.norm1.eps)
        a = ops.SwinWindowAttention.apply(qkv, m.qkv.bias, m.relative_position_bias_table, hw_shape[0], hw_shape[1], m.num_heads,
                                          self.attn.window_size, self.attn.shift_size, m.scale)
        x = L(a, m.proj.weight, m.proj.bias, None, None, x, proj_p, proj_t, 'res', 0.0)
        h, x = L(x, fc1.weight, fc1.bias, self.norm2.weight, self.norm2.bias, None, fc1_p, fc1_t, 'ln_gelu', self.norm2.eps)
        return L(h, fc2.weight, fc2.bias, None, None, x, fc2_p, fc2_t, 'res', 0.0)

    def forward(self, x, hw_shape):
        if self.linear_impl != 'torch':
            if not self._needs_backward(x):
                return self._forward_fused(x, hw_shape)
            if self.linear_impl == 'hip_grad' and not torch.is_autocast_enabled('cuda'):
                return self._forward_fused_grad(x, hw_shape)
        x = self.attn(self.norm1(x), hw_shape) + x
        return self.ffn(self.norm2(x), identity=x)


class SwinBlockSequence(nn.Module):
    def __init__(self, embed_dims, num_heads, feedforward_channels, depth, window_size, downsample, qkv_bias=True,
                 qk_scale=None, attn_impl='torch', linear_impl='torch'):
        super().__init__()
        self.blocks = nn.ModuleList([SwinBlock(embed_dims, num_heads, feedforward_channels, window_size, i % 2 == 1,
                                               qkv_bias, qk_scale, attn_impl, linear_impl) for i in range(depth)])
        self.downsample = downsample

    def forward(self, x, hw_shape):
        for block in self.blocks:
            x = block(x, hw_shape)
        if self.downsample is not None:
            x_down, down_hw = self.downsample(x, hw_shape)
            return x_down, down_hw, x, hw_shape
        return x, hw_shape, x, hw_shape


class SwinTransformer(nn.Module):
    """Same constructor arguments as the reference (those that only matter for training / checkpoint loading are
    accepted and ignored), plus attn_impl: 'torch' (default), 'hip', the fused window attention of ShiftWindowMSA (forward only), or
    'hip_grad', the same with its HIP backward; a config selects one with dict(type='SwinTransformer', ..., attn_impl='hip'); and
    linear_impl: 'torch' (default), 'hip', the blocks' Linears with LayerNorm, GELU and residual fused in (SwinBlock; needs a fused
    attn_impl; forward only), or 'hip_grad', the same with their HIP backward (needs attn_impl='hip_grad').  forward(x (BN,3,H,W)) -> list: [stage-0 feature un-normed if return_stereo_feat] +
    [norm_i(stage i) for i in out_indices], each (BN, C_i, H_i, W_i) -- swin.py:946-971."""

    def __init__(self, pretrain_img_size=224, in_channels=3, embed_dims=96, patch_size=4, window_size=7, mlp_ratio=4,
                 depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), strides=(4, 2, 2, 2), out_indices=(0, 1, 2, 3),
                 qkv_bias=True, qk_scale=None, patch_norm=True, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1,
                 use_abs_pos_embed=False, act_cfg=None, norm_cfg=None, pretrain_style='official', pretrained=None,
                 init_cfg=None, with_cp=True, return_stereo_feat=False, output_missing_index_as_none=False,
                 frozen_stages=-1, attn_impl='torch', linear_impl='torch'):
        super().__init__()
        assert strides[0] == patch_size, 'Use non-overlapping patch embed.'
        if use_abs_pos_embed:
            raise NotImplementedError('use_abs_pos_embed=True is not used by the PreWorld configs')
        self.out_indices, self.return_stereo_feat = tuple(out_indices), return_stereo_feat
        self.output_missing_index_as_none = output_missing_index_as_none
        self.use_abs_pos_embed = False
        self.attn_impl = attn_impl
        self.linear_impl = linear_impl
        self.patch_embed = PatchEmbed(in_channels, embed_dims, patch_size, strides[0], norm=patch_norm)
        self.drop_after_pos = nn.Dropout(p=drop_rate)
        self.stages = nn.ModuleList()
        c = embed_dims
        for i in range(len(depths)):
            down = PatchMerging(c, 2 * c, strides[i + 1], norm=patch_norm) if i < len(depths) - 1 else None
            self.stages.append(SwinBlockSequence(c, num_heads[i], mlp_ratio * c, depths[i], window_size, down, qkv_bias,
                                                 qk_scale, attn_impl, linear_impl))
            if down is not None:
                c = down.out_channels
        self.num_features = [int(embed_dims * 2 ** i) for i in range(len(depths))]
        for i in self.out_indices:
            self.add_module('norm%d' % i, nn.LayerNorm(self.num_features[i]))

    def set_attn_impl(self, attn_impl):
        """switch every block of a built model between 'torch', 'hip' and 'hip_grad' (the fused window attention); an unsupported block raises
        before any block is switched"""
        blocks = [m for m in self.modules() if isinstance(m, ShiftWindowMSA)]
        for m in blocks:
            _check_attn_impl(attn_impl, m.w_msa.embed_dims, m.w_msa.num_heads, m.window_size)
        for m in blocks:
            m.set_attn_impl(attn_impl)
        self.attn_impl = attn_impl

    def set_linear_impl(self, linear_impl):
        """switch every block of a built model between 'torch', 'hip' and 'hip_grad' (the fused Linears); a block that cannot take it -- its
        attention is not fused, or a Linear's width is not supported -- raises before any block is switched"""
        blocks = [m for m in self.modules() if isinstance(m, SwinBlock)]
        for m in blocks:
            m.check_linear_impl(linear_impl)
        for m in blocks:
            m.set_linear_impl(linear_impl)
        self.linear_impl = linear_impl

    def _to_map(self, out, hw, i, channels_last=False):
        m = out.view(-1, *hw, self.num_features[i]).permute(0, 3, 1, 2)
        # the stereo feature only feeds the cost volume kernel, whose fast path reads channels-last storage: the
        # token layout (B, H*W, C) already is that, so the NCHW-shaped view is handed out without the 138 MB copy
        return m if channels_last else m.contiguous()

    def forward(self, x):
        x = self.drop_after_pos(self.patch_embed(x))
        hw_shape = (self.patch_embed.DH, self.patch_embed.DW)
        outs = []
        for i, stage in enumerate(self.stages):
            x, hw_shape, out, out_hw = stage(x, hw_shape)
            if i == 0 and self.return_stereo_feat:
                outs.append(self._to_map(out, out_hw, i, channels_last=True))
            if i in self.out_indices:
                outs.append(self._to_map(getattr(self, 'norm%d' % i)(out), out_hw, i))
            elif self.output_missing_index_as_none:
                outs.append(None)
        return outs

    def stereo_ref_feat(self, x):
        """extract_stereo_ref_feat's Swin branch (bevdet.py:589-603): patch embedding + stage 0 only."""
        x = self.drop_after_pos(self.patch_embed(x))
        hw_shape = (self.patch_embed.DH, self.patch_embed.DW)
        _, _, out, out_hw = self.stages[0](x, hw_shape)
        return self._to_map(out, out_hw, 0, channels_last=True)


# ----------------------------------------------------------------------------------------------- fused convolutions
CONV_IMPLS = ('torch', 'hip')


def _conv_reason(conv):
    """None if ops.conv2d takes this layer, else the reason it does not"""
    from . import ops
    if not isinstance(conv, nn.Conv2d):
        return 'a %s is not an nn.Conv2d' % type(conv).__name__
    if conv.padding_mode != 'zeros':
        return 'padding_mode %r' % conv.padding_mode
    return ops.conv2d_supported(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.dilation, conv.padding,
                                conv.groups)


def _check_conv_impl(conv_impl, convs):
    """'hip' has no fallback: a layer pw_conv2d does not take is refused where the module is built or switched"""
    if conv_impl not in CONV_IMPLS:
        raise ValueError('conv_impl must be one of %s, got %r' % (CONV_IMPLS, conv_impl))
    if conv_impl != 'torch':
        for name, conv in convs:
            why = _conv_reason(conv)
            if why is not None:
                raise ValueError("conv_impl=%r: the fused convolution does not support %s: %s" % (conv_impl, name, why))
    return conv_impl


def _channels_last(x):
    """x in torch.channels_last storage: itself if it already is, else one copy"""
    return x if x.permute(0, 2, 3, 1).is_contiguous() else x.contiguous(memory_format=torch.channels_last)


class _FusedConvs:
    """What FPN_LSS, DepthNet, BasicBlock2d, ASPP and _ASPPModule share for conv_impl='hip': every stride-1 convolution listed by
    _own_convs() runs ops.conv2d (include/preworld_hip_conv2d.h) with its eval-mode BatchNorm, bias, ReLU and residual folded in, on
    channels-last maps.  The fused path is taken in eval mode, when autograd needs no backward, outside autocast; in training mode
    (BatchNorm batch statistics), with grad, or under autocast (bf16) the module runs exactly its 'torch' path -- those are out of
    scope of the kernel.  Packed operands live in a modules.Derived cache keyed on the convolution's parameters and the BatchNorm's
    parameters and running statistics, so load_state_dict or an optimizer step rebuilds them.  Parameters, buffers and state-dict
    keys do not depend on conv_impl."""
    conv_impl = 'torch'
    _derived = None

    def _own_convs(self):
        raise NotImplementedError

    def _fused_convs(self):
        """(name, layer) of every convolution the fused path of this module and of the modules below it runs"""
        return [((prefix + '.' if prefix else '') + n, c) for prefix, m in self.named_modules() if isinstance(m, _FusedConvs)
                for n, c in m._own_convs()]

    def check_conv_impl(self, conv_impl):
        return _check_conv_impl(conv_impl, self._fused_convs())

    def set_conv_impl(self, conv_impl):
        """switch this module and every module below it between 'torch' and 'hip'; a layer the kernel does not take raises before any
        module is switched"""
        self.check_conv_impl(conv_impl)
        for m in self.modules():
            if isinstance(m, _FusedConvs):
                m.conv_impl = conv_impl

    def _fused(self, *xs):
        if self.conv_impl != 'hip' or self.training or torch.is_autocast_enabled(xs[0].device.type):
            return False
        return not (torch.is_grad_enabled() and (any(x.requires_grad for x in xs) or any(p.requires_grad for p in self.parameters())))

    def _conv(self, x, name, conv, bn=None, relu=False, residual=None):
        from . import ops
        from .modules import Derived
        if self._derived is None:
            self._derived = Derived()
        pk = self._derived.get('conv2d_' + name, (conv, bn), lambda: ops.conv2d_pack(conv, bn))
        return ops.conv2d(x, pk, dilation=conv.dilation[0], relu=relu, residual=residual)


# ----------------------------------------------------------------------------------------------- FPN_LSS
class FPN_LSS(_FusedConvs, nn.Module):
    """lss_fpn.py:12-101.  conv_impl='torch' (default) or 'hip' (_FusedConvs): with 'hip' the inputs are made channels-last, the
    bilinear upsample and the concat stay on torch, and the convolutions run ops.conv2d with BatchNorm and ReLU fused; the output keeps
    its NCHW shape and values, in channels-last storage.  A config selects it with dict(type='FPN_LSS', ..., conv_impl='hip')."""

    def __init__(self, in_channels, out_channels, scale_factor=4, input_feature_index=(0, 2), norm_cfg=None,
                 extra_upsample=2, lateral=None, use_input_conv=False, conv_impl='torch'):
        super().__init__()
        if lateral is not None or use_input_conv:
            raise NotImplementedError('lateral / use_input_conv are not used by the PreWorld configs')
        self.input_feature_index = input_feature_index
        self.extra_upsample = extra_upsample is not None
        self.up = nn.Upsample(scale_factor=scale_factor, mode='bilinear', align_corners=True)
        cf = 2 if self.extra_upsample else 1
        self.conv = nn.Sequential(
            nn.Conv2d(in_channels, out_channels * cf, 3, padding=1, bias=False), nn.BatchNorm2d(out_channels * cf),
            nn.ReLU(inplace=True),
            nn.Conv2d(out_channels * cf, out_channels * cf, 3, padding=1, bias=False), nn.BatchNorm2d(out_channels * cf),
            nn.ReLU(inplace=True))
        if self.extra_upsample:
            self.up2 = nn.Sequential(
                nn.Upsample(scale_factor=extra_upsample, mode='bilinear', align_corners=True),
                nn.Conv2d(out_channels * cf, out_channels, 3, padding=1, bias=False), nn.BatchNorm2d(out_channels),
                nn.ReLU(inplace=True), nn.Conv2d(out_channels, out_channels, 1, padding=0))
        self.conv_impl = self.check_conv_impl(conv_impl)

    def _own_convs(self):
        convs = [('conv.0', self.conv[0]), ('conv.3', self.conv[3])]
        if self.extra_upsample:
            convs += [('up2.1', self.up2[1]), ('up2.4', self.up2[4])]
        return convs

    def _forward_hip(self, x2, x1):
        x = _channels_last(torch.cat([_channels_last(x2), self.up(_channels_last(x1))], dim=1))      # both channels-last: so is the concat
        x = self._conv(x, 'conv.0', self.conv[0], self.conv[1], relu=True)
        x = self._conv(x, 'conv.3', self.conv[3], self.conv[4], relu=True)
        if self.extra_upsample:
            x = _channels_last(self.up2[0](x))
            x = self._conv(x, 'up2.1', self.up2[1], self.up2[2], relu=True)
            x = self._conv(x, 'up2.4', self.up2[4])
        return x

    def forward(self, feats):
        x2, x1 = feats[self.input_feature_index[0]], feats[self.input_feature_index[1]]
        if self._fused(x2, x1):
            return self._forward_hip(x2, x1)
        x = self.conv(torch.cat([x2, self.up(x1)], dim=1))
        return self.up2(x) if self.extra_upsample else x


# ----------------------------------------------------------------------------------------------- DepthNet
class BasicBlock2d(_FusedConvs, nn.Module):
    """mmdet.models.backbones.resnet.BasicBlock (2.24, third-party): 3x3 conv-BN-ReLU, 3x3 conv-BN, + downsample(x), ReLU.
    conv_impl='hip' (_FusedConvs): three ops.conv2d calls -- conv1 with bn1 and ReLU, the downsample convolution if there is one, conv2
    with bn2, the residual addition and ReLU.  A strided or grouped layer is refused where the block is built."""

    def __init__(self, inplanes, planes, stride=1, downsample=None, conv_impl='torch'):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.conv_impl = self.check_conv_impl(conv_impl)

    def _own_convs(self):
        return [('conv1', self.conv1), ('conv2', self.conv2)] + ([] if self.downsample is None else [('downsample', self.downsample)])

    def _forward_hip(self, x):
        x = _channels_last(x)
        out = self._conv(x, 'conv1', self.conv1, self.bn1, relu=True)
        identity = x if self.downsample is None else self._conv(x, 'downsample', self.downsample)
        return self._conv(out, 'conv2', self.conv2, self.bn2, relu=True, residual=identity)

    def forward(self, x):
        if self._fused(x):
            return self._forward_hip(x)
        out = self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x)))))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class _ASPPModule(_FusedConvs, nn.Module):
    def __init__(self, inplanes, planes, kernel_size, padding, dilation, conv_impl='torch'):
        super().__init__()
        self.atrous_conv = nn.Conv2d(inplanes, planes, kernel_size, stride=1, padding=padding, dilation=dilation, bias=False)
        self.bn = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU()
        self.conv_impl = self.check_conv_impl(conv_impl)

    def _own_convs(self):
        return [('atrous_conv', self.atrous_conv)]

    def forward(self, x):
        if self._fused(x):
            return self._conv(_channels_last(x), 'atrous_conv', self.atrous_conv, self.bn, relu=True)
        return self.relu(self.bn(self.atrous_conv(x)))


class ASPP(_FusedConvs, nn.Module):
    """view_transformer.py:323-420.  conv_impl='hip' (_FusedConvs): the four branches and conv1 + bn1 + ReLU run ops.conv2d; the pooled
    branch, its upsample and the concat stay on torch; the Dropout is an identity in eval mode, the only mode the fused path runs in."""

    def __init__(self, inplanes, mid_channels=256, conv_impl='torch'):
        super().__init__()
        self.aspp1 = _ASPPModule(inplanes, mid_channels, 1, 0, 1, conv_impl)
        self.aspp2 = _ASPPModule(inplanes, mid_channels, 3, 6, 6, conv_impl)
        self.aspp3 = _ASPPModule(inplanes, mid_channels, 3, 12, 12, conv_impl)
        self.aspp4 = _ASPPModule(inplanes, mid_channels, 3, 18, 18, conv_impl)
        self.global_avg_pool = nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)), nn.Conv2d(inplanes, mid_channels, 1, bias=False),
                                             nn.BatchNorm2d(mid_channels), nn.ReLU())
        self.conv1 = nn.Conv2d(int(mid_channels * 5), inplanes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(inplanes)
        self.relu = nn.ReLU()
        self.dropout = nn.Dropout(0.5)
        self.conv_impl = self.check_conv_impl(conv_impl)

    def _own_convs(self):
        return [('conv1', self.conv1)]

    def _forward_hip(self, x):
        x = _channels_last(x)
        x5 = F.interpolate(self.global_avg_pool(x), size=x.shape[2:], mode='bilinear', align_corners=True)
        x = torch.cat((self.aspp1(x), self.aspp2(x), self.aspp3(x), self.aspp4(x), _channels_last(x5)), dim=1)
        return self._conv(_channels_last(x), 'conv1', self.conv1, self.bn1, relu=True)

    def forward(self, x):
        if self._fused(x):
            return self._forward_hip(x)
        x5 = F.interpolate(self.global_avg_pool(x), size=x.shape[2:], mode='bilinear', align_corners=True)
        x = torch.cat((self.aspp1(x), self.aspp2(x), self.aspp3(x), self.aspp4(x), x5), dim=1)
        return self.dropout(self.relu(self.bn1(self.conv1(x))))


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = nn.ReLU()
        self.drop1 = nn.Dropout(0.0)
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)
        self.drop2 = nn.Dropout(0.0)

    def forward(self, x):
        return self.drop2(self.fc2(self.drop1(self.act(self.fc1(x)))))


class SELayer(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv_reduce = nn.Conv2d(channels, channels, 1, bias=True)
        self.act1 = nn.ReLU()
        self.conv_expand = nn.Conv2d(channels, channels, 1, bias=True)
        self.gate = nn.Sigmoid()

    def forward(self, x, x_se):
        return x * self.gate(self.conv_expand(self.act1(self.conv_reduce(x_se))))


class DepthNet(_FusedConvs, nn.Module):
    """view_transformer.py:471-638 with use_dcn=False (the PreWorld configs).  With `stereo_metas` holding a previous
    stereo feature the cost volume comes from ops.stereo_cost_volume (HIP, one kernel instead of the reference's 32
    grid_sample rounds); without one it is zeros, as in the reference (:621-628).
    conv_impl='hip' (_FusedConvs; depthnet_cfg=dict(..., conv_impl='hip') in a config): reduce_conv, context_conv, the BasicBlocks, the
    ASPP and the last depth_conv layer run ops.conv2d on channels-last maps; the BatchNorm1d, the Mlps, the SE gates and their
    (B, C, 1, 1) convolutions, the concats and cost_volumn_net (stride 2) stay on torch.  The output keeps its NCHW shape and values,
    in channels-last storage."""

    def __init__(self, in_channels, mid_channels, context_channels, depth_channels, use_dcn=True, use_aspp=True,
                 with_cp=False, stereo=False, bias=0.0, aspp_mid_channels=-1, D=100, conv_impl='torch'):
        super().__init__()
        if use_dcn:
            raise NotImplementedError('use_dcn=True (mmcv deformable conv) is not used by the PreWorld configs')
        self.reduce_conv = nn.Sequential(nn.Conv2d(in_channels, mid_channels, 3, stride=1, padding=1),
                                         nn.BatchNorm2d(mid_channels), nn.ReLU(inplace=True))
        self.context_conv = nn.Conv2d(mid_channels, context_channels, 1)
        self.bn = nn.BatchNorm1d(27)
        self.depth_mlp = Mlp(27, mid_channels, mid_channels)
        self.depth_se = SELayer(mid_channels)
        self.context_mlp = Mlp(27, mid_channels, mid_channels)
        self.context_se = SELayer(mid_channels)
        cin, downsample = mid_channels, None
        self.stereo = stereo
        if stereo:
            cin += depth_channels
            downsample = nn.Conv2d(cin, mid_channels, 1, 1, 0)
            net = []
            for _ in range(2):
                net += [nn.Conv2d(depth_channels, depth_channels, 3, stride=2, padding=1), nn.BatchNorm2d(depth_channels)]
            self.cost_volumn_net = nn.Sequential(*net)
            self.bias = bias
        if conv_impl not in CONV_IMPLS:
            raise ValueError('conv_impl must be one of %s, got %r' % (CONV_IMPLS, conv_impl))
        layers = [BasicBlock2d(cin, mid_channels, downsample=downsample, conv_impl=conv_impl),
                  BasicBlock2d(mid_channels, mid_channels, conv_impl=conv_impl), BasicBlock2d(mid_channels, mid_channels, conv_impl=conv_impl)]
        if use_aspp:
            layers.append(ASPP(mid_channels, mid_channels if aspp_mid_channels < 0 else aspp_mid_channels, conv_impl))
        layers.append(nn.Conv2d(mid_channels, depth_channels, 1))
        self.depth_conv = nn.Sequential(*layers)
        self.depth_channels = depth_channels
        self.conv_impl = self.check_conv_impl(conv_impl)

    def _own_convs(self):
        return [('reduce_conv.0', self.reduce_conv[0]), ('context_conv', self.context_conv),
                ('depth_conv.%d' % (len(self.depth_conv) - 1), self.depth_conv[-1])]

    def _forward_hip(self, x, mlp_input, stereo_metas):
        x = self._conv(_channels_last(x), 'reduce_conv.0', self.reduce_conv[0], self.reduce_conv[1], relu=True)
        context = self.context_se(x, self.context_mlp(mlp_input)[..., None, None])
        context = self._conv(_channels_last(context), 'context_conv', self.context_conv)
        depth = self.depth_se(x, self.depth_mlp(mlp_input)[..., None, None])
        if stereo_metas is not None:
            depth = torch.cat([_channels_last(depth), _channels_last(self.cost_volumn_net(self._cost_volume(x, stereo_metas)))], dim=1)
        depth = _channels_last(depth)
        for layer in self.depth_conv[:-1]:
            depth = layer(depth)                          # BasicBlock2d / ASPP: their own fused path
        depth = self._conv(depth, 'depth_conv.%d' % (len(self.depth_conv) - 1), self.depth_conv[-1])
        return torch.cat([depth, context], dim=1)

    def calculate_cost_volumn(self, metas):
        from . import ops
        prev, curr = metas['cv_feat_list']
        return ops.stereo_cost_volume(prev, curr, metas['frustum'], metas['k2s_sensor'], metas['intrins'],
                                      metas['post_rots'], metas['post_trans'], bias=self.bias)

    def _cost_volume(self, x, stereo_metas):
        if stereo_metas['cv_feat_list'][0] is None:
            BN, _, H, W = x.shape
            s = float(stereo_metas['downsample']) / stereo_metas['cv_downsample']
            return torch.zeros((BN, self.depth_channels, int(H * s), int(W * s))).to(x)
        with torch.no_grad():
            return self.calculate_cost_volumn(stereo_metas)

    def forward(self, x, mlp_input, stereo_metas=None):
        mlp_input = self.bn(mlp_input.reshape(-1, mlp_input.shape[-1]))
        if self._fused(x, mlp_input):
            return self._forward_hip(x, mlp_input, stereo_metas)
        x = self.reduce_conv(x)
        context = self.context_conv(self.context_se(x, self.context_mlp(mlp_input)[..., None, None]))
        depth = self.depth_se(x, self.depth_mlp(mlp_input)[..., None, None])
        if stereo_metas is not None:
            depth = torch.cat([depth, self.cost_volumn_net(self._cost_volume(x, stereo_metas))], dim=1)
        return torch.cat([self.depth_conv(depth), context], dim=1)


def get_mlp_input(sensor2ego, ego2global, intrin, post_rot, post_tran, bda):
    """LSSViewTransformerBEVDepth.get_mlp_input (view_transformer.py:713-734): 15 scalars + sensor2ego[:3,:] = 27."""
    B, N, _, _ = sensor2ego.shape
    bda = bda.view(B, 1, 3, 3).repeat(1, N, 1, 1)
    v = torch.stack([intrin[:, :, 0, 0], intrin[:, :, 1, 1], intrin[:, :, 0, 2], intrin[:, :, 1, 2],
                     post_rot[:, :, 0, 0], post_rot[:, :, 0, 1], post_tran[:, :, 0],
                     post_rot[:, :, 1, 0], post_rot[:, :, 1, 1], post_tran[:, :, 1],
                     bda[:, :, 0, 0], bda[:, :, 0, 1], bda[:, :, 1, 0], bda[:, :, 1, 1], bda[:, :, 2, 2]], dim=-1)
    return torch.cat([v, sensor2ego[:, :, :3, :].reshape(B, N, -1)], dim=-1)


def create_frustum(depth_cfg, input_size, downsample):
    """LSSViewTransformer.create_frustum (view_transformer.py:84-112): (D, H/ds, W/ds, 3) of (u, v, d)."""
    H_in, W_in = input_size
    Hf, Wf = H_in // downsample, W_in // downsample
    d = torch.arange(*depth_cfg, dtype=torch.float).view(-1, 1, 1).expand(-1, Hf, Wf)
    D = d.shape[0]
    x = torch.linspace(0, W_in - 1, Wf, dtype=torch.float).view(1, 1, Wf).expand(D, Hf, Wf)
    y = torch.linspace(0, H_in - 1, Hf, dtype=torch.float).view(1, Hf, 1).expand(D, Hf, Wf)
    return torch.stack((x, y, d), -1)


# ----------------------------------------------------------------------------------------------- image -> (depth, context)
class ImageBranch(nn.Module):
    """img_backbone + img_neck + DepthNet with the reference's attribute names (`img_backbone`, `img_neck`,
    `img_view_transformer.depth_net`) so that a detector checkpoint's keys map one to one.

    frames_from_images(...) runs BEVStereo4DOCC.extract_img_feat's frame loop (bevdet_occ.py:188-241) up to the lifting
    inputs: for fid = num_frame-1 .. 0: the extra reference frame gives only its stage-0 stereo feature; every other
    frame goes through backbone, neck and DepthNet (cost volume against the previously processed, i.e. older, frame's
    stereo feature) and yields dict(depth softmax (B*N, D, H, W), tran_feat channels-last (B*N, H, W, C), sensor2keyego,
    intrin, post_rot, post_tran, bda) -- exactly what modules.PreWorld4DTraj.simple_test_from_lift consumes (key first)."""

    def __init__(self, backbone_cfg, neck_cfg, depthnet_cfg, grid_depth, input_size, downsample=16, out_channels=32,
                 in_channels=512, conv_impl=None):
        super().__init__()
        if conv_impl is not None:                         # over what the two configs say; None leaves them as they are
            if conv_impl not in CONV_IMPLS:
                raise ValueError('conv_impl must be one of %s, got %r' % (CONV_IMPLS, conv_impl))
            neck_cfg, depthnet_cfg = dict(neck_cfg, conv_impl=conv_impl), dict(depthnet_cfg, conv_impl=conv_impl)
        self.img_backbone = SwinTransformer(**backbone_cfg)
        self.img_neck = FPN_LSS(**neck_cfg)
        self.img_view_transformer = nn.Module()
        self.D = len(torch.arange(*grid_depth))
        self.img_view_transformer.depth_net = DepthNet(in_channels, in_channels, out_channels, self.D, **depthnet_cfg)
        self.out_channels, self.downsample = out_channels, downsample
        self.register_buffer('cv_frustum', create_frustum(grid_depth, input_size, 4), persistent=False)

    @property
    def conv_impl(self):
        """'torch' or 'hip' (FPN_LSS and DepthNet, see _FusedConvs), or 'mixed' if the two were configured differently"""
        a, b = self.img_neck.conv_impl, self.img_view_transformer.depth_net.conv_impl
        return a if a == b else 'mixed'

    def set_conv_impl(self, conv_impl):
        """switch the neck and the DepthNet between 'torch' and 'hip' (the fused convolutions); a layer the kernel does not take raises
        before either is switched"""
        parts = (self.img_neck, self.img_view_transformer.depth_net)
        for m in parts:
            m.check_conv_impl(conv_impl)
        for m in parts:
            m.set_conv_impl(conv_impl)

    def image_encoder(self, img):
        B, N, C, H, W = img.shape
        x = self.img_backbone(img.view(B * N, C, H, W))
        stereo_feat, x = x[0], self.img_neck(x[1:])
        return x.view(B, N, *x.shape[1:]), stereo_feat

    @torch.no_grad()
    def frames_from_images(self, imgs, sensor2keyegos, ego2globals, intrins, post_rots, post_trans, bda, curr2adjsensor,
                           extra_ref_frames=1, with_prev=True):
        from . import ops
        num_frame = len(imgs)
        frames, feat_prev = [], None
        for fid in range(num_frame - 1, -1, -1):
            img = imgs[fid]
            if fid == num_frame - extra_ref_frames:
                B, N, C, H, W = img.shape
                feat_prev = self.img_backbone.stereo_ref_feat(img.view(B * N, C, H, W))
                continue
            if not (fid == 0 or with_prev):
                continue
            mlp_input = get_mlp_input(sensor2keyegos[0], ego2globals[0], intrins[fid], post_rots[fid], post_trans[fid], bda)
            x, stereo_feat = self.image_encoder(img)
            B, N, C, H, W = x.shape
            metas = dict(k2s_sensor=curr2adjsensor[fid], intrins=intrins[fid], post_rots=post_rots[fid],
                         post_trans=post_trans[fid], frustum=self.cv_frustum.to(x), cv_downsample=4,
                         downsample=self.downsample, cv_feat_list=[feat_prev, stereo_feat])
            out = self.img_view_transformer.depth_net(x.view(B * N, C, H, W), mlp_input, metas)
            depth, feat = ops.depthnet_tail(out.float().contiguous(), self.D, self.out_channels)
            feat._pw_channels_last = True       # (B*N, H, W, C): view_transform_core skips its permute copy
            frames.append(dict(depth=depth, tran_feat=feat, sensor2keyego=sensor2keyegos[fid], intrin=intrins[fid],
                               post_rot=post_rots[fid], post_tran=post_trans[fid], bda=bda))
            feat_prev = stereo_feat
        return frames[::-1]                     # key frame first


def preworld_image_cfg():
    """configs/preworld/nuscenes/bevstereo-occ.py:45-88: Swin-B, FPN_LSS, DepthNet of the PreWorld detectors."""
    return dict(
        backbone_cfg=dict(pretrain_img_size=224, patch_size=4, window_size=12, mlp_ratio=4, embed_dims=128,
                          depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], strides=(4, 2, 2, 2), out_indices=(2, 3),
                          qkv_bias=True, qk_scale=None, patch_norm=True, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1,
                          use_abs_pos_embed=False, return_stereo_feat=True, pretrain_style='official',
                          output_missing_index_as_none=False),
        neck_cfg=dict(in_channels=512 + 1024, out_channels=512, extra_upsample=None, input_feature_index=(0, 1),
                      scale_factor=2),
        depthnet_cfg=dict(use_dcn=False, aspp_mid_channels=96, stereo=True, bias=5.),
        grid_depth=[1.0, 45.0, 0.5], input_size=(512, 1408), downsample=16, out_channels=32, in_channels=512)
