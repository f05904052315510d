"""The voxel losses of the fine-tune step restated in float64 torch under autograd -- the yardstick the loss kernels
(csrc/pw_loss.hip, csrc/pw_loss2.hip) answer to.  Written from the formulas oracle/oracle.py cites, not from the reference's
program text:
  * CE_ssc_loss, sem_scal_loss, geo_scal_loss (mmdet3d/models/detectors/loss.py:20-113) as losses.voxel_losses combines them:
    class-weighted cross entropy over the voxels whose label is not `ignore_index`; the per-class precision / recall / specificity
    terms over the voxels that are not ignored (and in the camera mask); the geometry terms of the `empty_idx` class.  Every
    BCE(x, 1) goes through F.binary_cross_entropy, so both its log clamp at -100 and its backward,
    (x - 1) / max(x (1 - x), 1e-12), are the reference's.
  * CustomFocalLoss (mmdet3d/models/loss_utils/focal_loss.py:163-262): per valid voxel the sigmoid focal loss of its C logits,
    weighted by class_weights[c] * oracle.focal_radial_map(X, Y)[x, y], summed over classes, averaged over the valid voxels,
    times loss_weight.
  * lovasz_softmax(classes='present', per_image=False) (mmdet3d/models/detectors/lovasz_softmax.py:20-33, 157-232): for every
    class present among the valid voxels, the errors |fg - p_c| sorted descending dotted with lovasz_grad(fg_sorted), which is a
    constant (no gradient flows through it); the mean over those classes.
Every function takes float64 tensors (B, C, X, Y, Z) on any device and returns float64 scalars."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle as O


def _bce1(x):
    return F.binary_cross_entropy(x, torch.ones_like(x))


def voxel_losses(pred, target, class_weights=None, ignore_index=255, empty_idx=17, camera_mask=None):
    """-> (ce, sem, geo); pred (B,C,X,Y,Z) float64 logits, target (B,X,Y,Z) integers, camera_mask (B,X,Y,Z) bool or None"""
    B, C = pred.shape[:2]
    t = target.long()
    cam = torch.ones_like(t, dtype=torch.bool) if camera_mask is None else camera_mask.bool()
    w = torch.ones(C, dtype=pred.dtype, device=pred.device) if class_weights is None else class_weights.to(pred)
    logp = torch.log_softmax(pred, dim=1)
    p = torch.softmax(pred, dim=1)
    # cross entropy: sum_v w[t] (-log p_t) / sum_v w[t] over the voxels that are not ignored
    valid = t != ignore_index
    tv = t[valid]
    lp_t = logp.movedim(1, -1)[valid].gather(1, tv[:, None])[:, 0]
    ce = (w[tv] * -lp_t).sum() / w[tv].sum()
    # sem_scal: over the voxels that are not ignored and in the camera mask
    M = valid & cam
    pm = p.movedim(1, -1)[M]                                       # (n, C)
    tm = t[M]
    sem, count = pred.new_zeros(()), 0
    for i in range(C):
        ct = (tm == i).to(pred.dtype)
        if ct.sum() > 0:
            count += 1
            pi = pm[:, i]
            nom = (pi * ct).sum()
            lc = pred.new_zeros(())
            if pi.sum() > 0:
                lc = lc + _bce1(nom / pi.sum())
            lc = lc + _bce1(nom / ct.sum())
            if (1 - ct).sum() > 0:
                lc = lc + _bce1(((1 - pi) * (1 - ct)).sum() / (1 - ct).sum())
            sem = sem + lc
    sem = sem / count
    # geo_scal: over every voxel; target "non-empty" = label != empty_idx and in the camera mask
    pe = p[:, empty_idx].reshape(-1)
    nt = ((t != empty_idx) & cam).to(pred.dtype).reshape(-1)
    inter = (nt * (1 - pe)).sum()
    geo = _bce1(inter / (1 - pe).sum()) + _bce1(inter / nt.sum()) + _bce1(((1 - nt) * pe).sum() / (1 - nt).sum())
    return ce, sem, geo


def focal_loss(pred, target, class_weights, ignore_index=255, camera_mask=None, gamma=2.0, alpha=0.25, loss_weight=100.0):
    """CustomFocalLoss()(pred, target, class_weights, None, ignore_index, camera_mask=camera_mask)"""
    B, C, X, Y, Z = pred.shape
    t = target.long()
    valid = t != ignore_index
    if camera_mask is not None:
        valid = valid & camera_mask.bool()
    cmap = torch.from_numpy(O.focal_radial_map(X, Y).astype(np.float64)).to(pred.device)
    z = pred.movedim(1, -1)[valid]                                  # (n, C)
    onehot = (t[valid][:, None] == torch.arange(C, device=pred.device)[None, :]).to(pred.dtype)
    # binary cross entropy with logits, times the focal factor alpha_t (1 - p_t)^gamma
    bce = F.softplus(z) - z * onehot
    s = torch.sigmoid(z)
    pt = (1 - s) * onehot + s * (1 - onehot)
    el = bce * (alpha * onehot + (1 - alpha) * (1 - onehot)) * pt.pow(gamma)
    rad = cmap[:, :, None].expand(X, Y, Z)[None].expand(B, X, Y, Z)[valid]
    wm = class_weights.to(pred)[None, :] * rad[:, None]
    return loss_weight * (el * wm).sum(-1).mean()


def lovasz_classes(probas, labels, ignore=None, camera_mask=None):
    """The valid voxels as lovasz_softmax flattens them: (valid (B*X*Y*Z,) bool, their probabilities (n, C), their labels (n,))"""
    B, C = probas.shape[:2]
    pr = probas.reshape(B, C, -1).movedim(1, 2).reshape(-1, C)
    lab = labels.reshape(-1).long()
    valid = torch.ones_like(lab, dtype=torch.bool) if ignore is None else lab != ignore
    if camera_mask is not None:
        valid = valid & camera_mask.reshape(-1).bool()
    return valid, pr[valid], lab[valid]


def lovasz_grad(fg_sorted):
    """the Jaccard loss gradient w.r.t. the sorted errors (Alg. 1 of the Lovasz-Softmax paper), float64"""
    fg = fg_sorted.to(torch.float64)
    gts = fg.sum()
    jac = 1.0 - (gts - fg.cumsum(0)) / (gts + (1 - fg).cumsum(0))
    if fg.numel() > 1:
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
    return jac


def lovasz_softmax(probas, labels, ignore=None, camera_mask=None):
    """probas (B,C,X,Y,Z) float64 probabilities, labels (B,X,Y,Z)"""
    _, vp, vl = lovasz_classes(probas, labels, ignore, camera_mask)
    losses = []
    for c in range(probas.shape[1]):
        fg = (vl == c).to(probas.dtype)
        if fg.sum() == 0:
            continue
        err = (fg - vp[:, c]).abs()
        es, perm = torch.sort(err, descending=True)
        losses.append(torch.dot(es, lovasz_grad(fg[perm]).detach()))
    if not losses:
        return (probas * 0).sum()
    return torch.stack(losses).mean()
