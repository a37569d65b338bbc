"""Training-side pieces of the reference that sit next to the hot path: losses, match costs, 3-D IoU,
the dynamic-k OTA label assignment and the frozen-LiDAR-branch helper.  The losses and match costs are plain torch.  The label assignment
on the GPU is HIP: all decoder stages and samples of a step in one call (`ops.ota_assign`, csrc/ota.hip; SRF_OTA=0 switches it off), with
the torch restatement kept as the route of everything that call does not take; so is the rotated BEV IoU under `bbox_overlaps_3d`.
With SRF_SET_LOSS=1 the focal and L1 losses of all decoder stages are one call as well (`SetLoss` around `ops.set_loss`, csrc/setloss.hip;
`set_loss_route` says when).

Mirrors: OTAssignerSRFDet  mmdet3d_plugin/core/bbox/assigners/ota_srfdet.py:18-327
         BBox3DL1Cost / IoU3DCost  mmdet3d_plugin/core/bbox/match_costs/match_cost.py:5-36
         FocalLoss / L1Loss / FocalLossCost / BboxOverlaps3D: mmdet 2.28 / mmdet3d 1.0rc6 semantics (not in the reference
         tree, "parity unpinned"); freeze_lidar_components  tools/train.py:221-276.
"""
import torch
import torch.distributed as dist
import torch.nn.functional as F
from torch import nn

from .. import ops
from ..compat.registry import BBOX_ASSIGNERS, LOSSES, MATCH_COST
from .bbox_util import boxes3d_to_corners3d, denormalize_bbox, normalize_bbox


def reduce_mean(t):
    """mmdet.core.utils.reduce_mean: mean over ranks (collective C4 of SURVEY.md 2.3)."""
    if not (dist.is_available() and dist.is_initialized()):
        return t
    t = t.clone()
    dist.all_reduce(t.div_(dist.get_world_size()), op=dist.ReduceOp.SUM)
    return t


@LOSSES.register_module()
class FocalLoss(nn.Module):
    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="mean", loss_weight=1.0, activated=False):
        super().__init__()
        assert use_sigmoid and not activated
        self.use_sigmoid, self.gamma, self.alpha, self.reduction, self.loss_weight = use_sigmoid, gamma, alpha, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        """pred (N, C) logits; target (N,) labels with C = background."""
        C = pred.size(1)
        t = F.one_hot(target, num_classes=C + 1)[:, :C].type_as(pred)
        p = pred.sigmoid()
        pt = (1 - p) * t + p * (1 - t)
        fw = (self.alpha * t + (1 - self.alpha) * (1 - t)) * pt.pow(self.gamma)
        loss = F.binary_cross_entropy_with_logits(pred, t, reduction="none") * fw
        if weight is not None:
            loss = loss * weight.view(-1, 1)
        if self.reduction == "sum":
            loss = loss.sum()
        elif self.reduction == "mean":
            loss = loss.sum() / avg_factor if avg_factor is not None else loss.mean()
        return self.loss_weight * loss


@LOSSES.register_module()
class L1Loss(nn.Module):
    def __init__(self, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        loss = (pred - target).abs()
        if weight is not None:
            loss = loss * weight
        if self.reduction == "sum":
            loss = loss.sum()
        elif self.reduction == "mean":
            loss = loss.sum() / avg_factor if avg_factor is not None else loss.mean()
        return self.loss_weight * loss


@MATCH_COST.register_module()
class FocalLossCost:
    def __init__(self, weight=1.0, alpha=0.25, gamma=2, eps=1e-12, binary_input=False):
        self.weight, self.alpha, self.gamma, self.eps = weight, alpha, gamma, eps

    def __call__(self, cls_pred, gt_labels):
        p = cls_pred.sigmoid()
        neg = -(1 - p + self.eps).log() * (1 - self.alpha) * p.pow(self.gamma)
        pos = -(p + self.eps).log() * self.alpha * (1 - p).pow(self.gamma)
        return (pos[:, gt_labels] - neg[:, gt_labels]) * self.weight


@MATCH_COST.register_module()
class BBox3DL1Cost:
    def __init__(self, weight=1.0):
        self.weight = weight

    def __call__(self, bbox_pred, gt_bboxes):
        return torch.cdist(bbox_pred, gt_bboxes, p=1) * self.weight


@MATCH_COST.register_module()
class IoU3DCost:
    def __init__(self, weight):
        self.weight = weight

    def __call__(self, iou):
        return -iou * self.weight


def bbox_overlaps_3d(boxes1, boxes2):
    """mmdet3d BboxOverlaps3D(coordinate='lidar'), mode 'iou': boxes (n, >=7) [x, y, z, dx, dy, dz, yaw] with z taken
    as the bottom face (the reference hands gravity centres to it on both sides, ota_srfdet.py:148-150) -> (n, m)."""
    n, m = boxes1.shape[0], boxes2.shape[0]
    if n * m == 0:
        return boxes1.new_zeros((n, m))
    top1, top2 = boxes1[:, 2] + boxes1[:, 5], boxes2[:, 2] + boxes2[:, 5]
    h = (torch.min(top1.view(-1, 1), top2.view(1, -1)) - torch.max(boxes1[:, 2].view(-1, 1), boxes2[:, 2].view(1, -1))).clamp(min=0)
    bev1 = boxes1[:, [0, 1, 3, 4, 6]].clone()
    bev2 = boxes2[:, [0, 1, 3, 4, 6]].clone()
    bev1[:, 2:4] = bev1[:, 2:4].clamp(min=1e-4)
    bev2[:, 2:4] = bev2[:, 2:4].clamp(min=1e-4)
    iou2d = ops.box_iou_rotated(bev1.contiguous(), bev2.contiguous())
    a1 = (bev1[:, 2] * bev1[:, 3]).view(-1, 1)
    a2 = (bev2[:, 2] * bev2[:, 3]).view(1, -1)
    inter3d = iou2d * (a1 + a2) / (1 + iou2d) * h
    v1 = (boxes1[:, 3] * boxes1[:, 4] * boxes1[:, 5]).view(-1, 1)
    v2 = (boxes2[:, 3] * boxes2[:, 4] * boxes2[:, 5]).view(1, -1)
    return inter3d / (v1 + v2 - inter3d).clamp(min=1e-8)


@MATCH_COST.register_module()
class ClassificationCost:
    """mmdet's softmax classification cost (the default `cls_cost` of HungarianAssignerSRFDet)."""

    def __init__(self, weight=1.0):
        self.weight = weight

    def __call__(self, cls_pred, gt_labels):
        return -cls_pred.softmax(-1)[:, gt_labels] * self.weight


@MATCH_COST.register_module()
class BBoxL1Cost(BBox3DL1Cost):
    """mmdet's name for the plain L1 cost (default `reg_cost` of HungarianAssignerSRFDet); the box format conversions of
    the 2-D original do not apply to the normalised 3-D boxes it is given here."""

    def __init__(self, weight=1.0, box_format="xyxy"):
        super().__init__(weight)


class AssignResult:
    """The four fields of mmdet's AssignResult that callers of the assigner read."""

    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


@BBOX_ASSIGNERS.register_module()
class HungarianAssignerSRFDet:
    """One-to-one matching of predictions to ground truth on cost = classification + L1 over the first 8 normalised box
    parameters, solved on the host with scipy (hungarian_assigner_srfdet.py:14-129).  No config of the reference enables
    it (the lines are commented out in favour of OTAssignerSRFDet); it is here so that those lines resolve."""

    def __init__(self, cls_cost=None, reg_cost=None, pc_range=None):
        self.cls_cost = MATCH_COST.build(cls_cost if cls_cost is not None else dict(type="ClassificationCost", weight=1.0))
        self.reg_cost = MATCH_COST.build(reg_cost if reg_cost is not None else dict(type="BBoxL1Cost", weight=1.0))
        self.pc_range = pc_range

    @torch.no_grad()
    def assign(self, bbox_pred, cls_pred, gt_bboxes, gt_labels, gt_bboxes_ignore=None, eps=1e-7, kdistillation=False):
        """-> AssignResult: gt_inds[i] = 0 for background or 1 + index of the matched ground truth; labels[i] = its class
        or -1."""
        from scipy.optimize import linear_sum_assignment
        from .bbox_util import normalize_bbox
        assert gt_bboxes_ignore is None, "gt_bboxes_ignore is not supported (as in the reference)"
        n_gt, n_q = gt_bboxes.size(0), bbox_pred.size(0)
        gt_inds = bbox_pred.new_full((n_q,), 0 if n_gt == 0 else -1, dtype=torch.long)
        labels = bbox_pred.new_full((n_q,), -1, dtype=torch.long)
        if n_gt == 0 or n_q == 0:
            return AssignResult(n_gt, gt_inds, None, labels=labels)
        target = gt_bboxes if kdistillation else normalize_bbox(gt_bboxes, self.pc_range)
        cost = self.cls_cost(cls_pred, gt_labels) + self.reg_cost(bbox_pred[:, :8], target[:, :8])
        rows, cols = linear_sum_assignment(cost.detach().cpu().numpy())
        rows = torch.from_numpy(rows).to(bbox_pred.device)
        cols = torch.from_numpy(cols).to(bbox_pred.device)
        gt_inds[:] = 0
        gt_inds[rows] = cols + 1
        labels[rows] = gt_labels[cols]
        return AssignResult(n_gt, gt_inds, None, labels=labels)


class Assigned(tuple):
    """What OTAssignerSRFDet returns for one sample: the pair (fg, j) -- fg (n_p,) bool, the foreground predictions; j (fg.sum(),) long, the
    ground-truth index of each in ascending prediction order -- and, on the kernel route, `rows` = the foreground indices themselves
    (fg.nonzero() without its host synchronisation), so that the losses select rows by index.  `rows` is None on the torch route."""

    def __new__(cls, fg, j, rows=None):
        self = super().__new__(cls, (fg, j))
        self.rows = rows
        return self


class AssignedLayers(list):
    """What `OTAssignerSRFDet.assign_layers` returns: the per-stage lists of per-sample `Assigned`, and on the kernel route `raw` = the
    tensors of the one `ops.ota_assign` call as they came back -- count (S, B), pred_idx / gt_idx (S, B, P) int32 -- with the padded ground
    truth beside them: gt_boxes (B, Gpad, 7 | 9), gt_labels (B, Gpad) int32.  `raw` is None on the torch route."""
    raw = None


@BBOX_ASSIGNERS.register_module()
class OTAssignerSRFDet(nn.Module):
    """1-to-k dynamic matching of predictions to ground truth (ota_srfdet.py:18-327).  On the GPU the whole assignment of a step -- every
    decoder stage, every sample -- is one call of `ops.ota_assign` (csrc/ota.hip: a cost and a match kernel, no read-back inside); the torch
    ops below are the same assignment for everything that call does not take (`kernel_route`)."""

    def __init__(self, cls_cost, reg_cost, iou_cost, center_radius=1.5, candidate_topk=5, pc_range=None, iou_calculator=None,
                 num_heads=6):
        super().__init__()
        self.center_radius, self.candidate_topk, self.pc_range, self.num_heads = center_radius, candidate_topk, pc_range, num_heads
        self.cls_cost, self.reg_cost, self.iou_cost = MATCH_COST.build(cls_cost), MATCH_COST.build(reg_cost), MATCH_COST.build(iou_cost)

    def forward(self, outputs, gt_boxes_list, gt_labels_list, head_idx):
        return self.assign_layers([(outputs, head_idx)], gt_boxes_list, gt_labels_list)[0]

    def single_assigner(self, pred_boxes, pred_logits, gt_boxes, gt_labels, head_idx):
        out = dict(pred_boxes=pred_boxes[None], pred_logits=pred_logits[None])
        return self.assign_layers([(out, head_idx)], [gt_boxes], [gt_labels])[0][0]

    def kernel_params(self):
        """The scalar arguments of `ops.ota_assign`, or None when a match cost is not one of the three classes csrc/ota.hip restates."""
        if type(self.cls_cost) is not FocalLossCost or type(self.reg_cost) is not BBox3DL1Cost or type(self.iou_cost) is not IoU3DCost:
            return None
        c = self.cls_cost
        return dict(cost_weights=(float(c.weight), float(self.reg_cost.weight), float(self.iou_cost.weight)), alpha=float(c.alpha),
                    gamma=float(c.gamma), eps=float(c.eps), center_radius=float(self.center_radius), candidate_topk=int(self.candidate_topk),
                    num_heads=int(self.num_heads))

    def kernel_route(self, layers, gts, labels):
        """Whether `assign_layers` makes the one call of `ops.ota_assign`: SRF_OTA is not 0, the three match costs are the configs', every
        tensor is a float32 (labels: integer) GPU tensor and the stacked shape is inside `ops.ota_assign_ok`."""
        if not ops.ota_enabled() or self.kernel_params() is None or not layers or not gts:
            return False
        boxes, logits = layers[0][0]["pred_boxes"], layers[0][0]["pred_logits"]
        for out, head_idx in layers:
            b, l = out["pred_boxes"], out["pred_logits"]
            if not (b.is_cuda and l.is_cuda and b.dtype == l.dtype == torch.float32 and b.dim() == 3 and b.shape == boxes.shape
                    and l.shape == logits.shape and l.shape[:2] == b.shape[:2]) or not isinstance(head_idx, int):
                return False
        if len(gts) != boxes.shape[0] or len(labels) != len(gts):
            return False
        for g, l in zip(gts, labels):
            if not (g.is_cuda and l.is_cuda and g.dtype == torch.float32 and g.dim() == 2 and g.shape[1] >= 7 and l.dim() == 1
                    and l.shape[0] == g.shape[0] and not l.dtype.is_floating_point and l.dtype != torch.bool):
                return False
        gpad = self._gpad(gts)
        return ops.ota_assign_ok(len(layers), boxes.shape[0], boxes.shape[1], boxes.shape[2], logits.shape[2], gpad, self.candidate_topk)

    @staticmethod
    def _gpad(gts):
        return (max(max(int(g.shape[0]) for g in gts), 1) + 7) // 8 * 8

    @torch.no_grad()
    def assign_layers(self, layers, gts, labels):
        """All decoder stages of a step at once.  layers: [(outputs of a stage, its head_idx)], every stage with pred_boxes (B, P, D) and
        pred_logits (B, P, C); gts / labels: the B samples' (n, >= 7) gravity-centre boxes and (n,) classes.  -> per stage, per sample an
        `Assigned`: (fg, j) as `single_assigner` has always returned them, with `.rows` = the foreground indices ascending.
        On the kernel route (`kernel_route`) this is ONE call of `ops.ota_assign` and ONE device-to-host copy (the matched counts and the
        status words); a (stage, sample) pair whose repair loop hit the kernel's cap is assigned again by the torch route."""
        if not self.kernel_route(layers, gts, labels):
            return AssignedLayers([self._single_torch(out["pred_boxes"][i], out["pred_logits"][i], gts[i], labels[i], head_idx)
                                   for i in range(len(gts))] for out, head_idx in layers)
        dev = gts[0].device
        S, B, P, G = len(layers), len(gts), layers[0][0]["pred_boxes"].shape[1], self._gpad(gts)
        boxes = torch.stack([out["pred_boxes"].detach() for out, _ in layers])
        logits = torch.stack([out["pred_logits"].detach() for out, _ in layers])
        ns = [int(g.shape[0]) for g in gts]                                  # host-known: no synchronisation
        gt_pad, lab_pad = torch.zeros((B, G, 7), dtype=torch.float32, device=dev), torch.zeros((B, G), dtype=torch.int32, device=dev)
        # the ground truth with all its columns (velocities) for `ops.set_loss`, only where that route is on and the boxes have more than 7
        Dg = int(gts[0].shape[1])
        wide = ops.set_loss_enabled() and Dg > 7 and all(int(g.shape[1]) == Dg for g in gts)
        gt_wide = torch.zeros((B, G, Dg), dtype=torch.float32, device=dev) if wide else None
        for b, (g, l) in enumerate(zip(gts, labels)):
            if ns[b]:
                gt_pad[b, :ns[b]] = g[:, :7]
                lab_pad[b, :ns[b]] = l
                if wide:
                    gt_wide[b, :ns[b]] = g
        # the box counts and head indices go up in one copy from pinned memory: a copy from pageable memory waits for the stream
        meta = torch.tensor(ns + [h for _, h in layers], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        n_gt, heads = meta[:B], meta[B:]
        count, pred_idx, gt_idx, status = ops.ota_assign(boxes, logits, gt_pad, lab_pad, n_gt, heads, **self.kernel_params())
        host = count._base.cpu().tolist()                                    # the one read-back: [counts, status words]
        # fg of every pair in one go: slot t of pair q is foreground row pred_idx[q, t] when t < count[q]; the other slots go to a spare cell
        slot = torch.arange(P, device=dev)
        live = slot[None, None, :] < count[:, :, None]
        flat = (torch.arange(S * B, device=dev).view(S, B, 1) * P + pred_idx).masked_fill_(~live, S * B * P)
        fg_all = torch.zeros(S * B * P + 1, dtype=torch.bool, device=dev)
        fg_all.index_fill_(0, flat.view(-1), True)
        fg_all = fg_all[:S * B * P].view(S, B, P)
        rows_all, j_all = pred_idx.long(), gt_idx.long()
        res = AssignedLayers()
        res.raw = dict(count=count, pred_idx=pred_idx, gt_idx=gt_idx, gt_boxes=gt_wide if wide else gt_pad, gt_labels=lab_pad)
        for s, (out, head_idx) in enumerate(layers):
            stage = []
            for b in range(B):
                n = host[0][s][b]
                if host[1][s][b] != 0:
                    stage.append(self._single_torch(out["pred_boxes"][b], out["pred_logits"][b], gts[b], labels[b], head_idx))
                else:
                    stage.append(Assigned(fg_all[s, b], j_all[s, b, :n], rows_all[s, b, :n]))
            res.append(stage)
        return res

    @torch.no_grad()
    def _single_torch(self, pred_boxes, pred_logits, gt_boxes, gt_labels, head_idx):
        """One stage of one sample in torch ops: the route of CPU tensors, other dtypes, shapes past the kernel's limits, other match costs,
        SRF_OTA=0 and of a pair the kernel gave up on."""
        n_gt = gt_boxes.size(0)
        if n_gt == 0:
            return Assigned(pred_boxes.new_zeros((pred_boxes.shape[0],), dtype=torch.bool), pred_boxes.new_zeros((0,), dtype=torch.long))
        cost, ious = self.cost_matrices(pred_boxes, pred_logits, gt_boxes, gt_labels)
        return Assigned(*self._dynamic_k(cost, ious, n_gt, head_idx))

    def cost_matrices(self, pred_boxes, pred_logits, gt_boxes, gt_labels):
        """cost and 3-D IoU (n_p, n_gt) of one sample, n_gt > 0, in torch ops."""
        valid, in_both = self._in_gt_and_center(pred_boxes, gt_boxes)
        cls = self.cls_cost(pred_logits, gt_labels)
        reg = self.reg_cost(pred_boxes[:, :8], normalize_bbox(gt_boxes[:, :7], self.pc_range))
        ious = bbox_overlaps_3d(denormalize_bbox(pred_boxes, self.pc_range), gt_boxes)
        cost = cls + reg + self.iou_cost(ious) + (~in_both) * 100.0
        cost[~valid] = cost[~valid] + 10000.0
        return cost, ious

    def _in_gt_and_center(self, pred, gt):
        c = pred[:, None, :3]                                                  # (n_p, 1, 3)
        corners = boxes3d_to_corners3d(gt[None, :, :7], bottom_center=False, ry=True)[0]   # (n_gt, 8, 3)
        lo, hi = corners.min(dim=1).values[None], corners.max(dim=1).values[None]
        in_box = ((c > lo) & (c < hi)).all(-1)                                  # (n_p, n_gt)
        r = self.center_radius * gt[None, :, 3:6]
        in_ctr = ((c > gt[None, :, :3] - r) & (c < gt[None, :, :3] + r)).all(-1)
        return in_box.any(1) | in_ctr.any(1), in_box & in_ctr

    def _dynamic_k(self, cost, ious, n_gt, head_idx):
        topk = torch.topk(ious, min(self.candidate_topk, ious.size(0)), dim=0).values
        ks = torch.clamp((topk.sum(0) - 0.5 * (self.num_heads - head_idx)).int(), min=1)
        # the reference walks the ground-truth boxes: `topk(cost[:, g], k = ks[g].item(), largest=False)` per box (ota_srfdet.py:296-300) --
        # one read-back of ks and, per box, a top-k and an index_put launch (200 + 200 launches per step at 20 boxes x 10 assignments).
        # The same set in one pass: a prediction matches box g when its rank in the ascending order of cost[:, g] is below ks[g].
        # Ties go to the lower index (the stable sort here, the first minimum of argmin below): tests/ota_ref.py states the rule,
        # tests/test_ota_ref.py holds this function to it, and csrc/ota.hip follows it on the GPU.
        order = torch.argsort(cost, dim=0, stable=True)
        rank = torch.empty_like(order)
        rank.scatter_(0, order, torch.arange(cost.shape[0], device=cost.device)[:, None].expand_as(order))
        match = (rank < ks[None, :]).to(cost.dtype)
        multi = match.sum(1) > 1
        if multi.any():
            best = cost[multi].argmin(dim=1)
            match[multi] = 0
            match[multi, best] = 1.0
        while (match.sum(0) == 0).any():
            cost[match.sum(1) > 0] += 100000.0
            for g in torch.nonzero(match.sum(0) == 0, as_tuple=False).squeeze(1).tolist():
                match[cost[:, g].argmin(), g] = 1.0
            if (match.sum(1) > 1).any():  # the reference re-uses the FIRST multi-match mask here (ota_srfdet.py:309-313)
                best = cost[multi].argmin(dim=1)
                match[multi] = match[multi] * 0
                match[multi, best] = 1.0
        fg = match.sum(1) > 0
        return fg, match[fg].argmax(1)


def set_loss_route(head, outs, assigned, gts):
    """Whether `SRFDetHead.loss_ota` computes the losses of the whole step in the one call of `ops.set_loss` (csrc/setloss.hip):
    SRF_SET_LOSS is 1; the assignment came from `ops.ota_assign` (`assigned.raw`) and every (stage, sample) pair carries `rows`, so none
    fell back on a status word; the losses are exactly FocalLoss and L1Loss with reduction "sum"; every prediction is a float32 GPU tensor
    of one shape; and the shape is inside `ops.set_loss_ok`.  outs: the stages' output dicts; gts: the samples' (n, 7 | 9) boxes."""
    raw = getattr(assigned, "raw", None)
    if not ops.set_loss_enabled() or raw is None or not outs or len(assigned) != len(outs):
        return False
    if not all(getattr(a, "rows", None) is not None for stage in assigned for a in stage):
        return False
    lc, lb = getattr(head, "loss_cls", None), getattr(head, "loss_bbox", None)
    if type(lc) is not FocalLoss or type(lb) is not L1Loss or lc.reduction != "sum" or lb.reduction != "sum":
        return False
    logits, boxes = outs[0]["pred_logits"], outs[0]["pred_boxes"]
    for out in outs:
        l, b = out["pred_logits"], out["pred_boxes"]
        if not (l.is_cuda and b.is_cuda and l.dtype == b.dtype == torch.float32 and l.dim() == 3 and l.shape == logits.shape
                and b.shape == boxes.shape and b.shape[:2] == l.shape[:2]):
            return False
    cw, gt = head.code_weights, raw["gt_boxes"]
    if not (cw.is_cuda and cw.dtype == torch.float32 and cw.dim() == 1) or len(gts) != logits.shape[0]:
        return False
    if any(int(g.shape[1]) != int(gt.shape[2]) for g in gts):          # the losses read every column the head's `gts` have
        return False
    return ops.set_loss_ok(len(outs), logits.shape[0], logits.shape[1], logits.shape[2], boxes.shape[2], cw.numel(), gt.shape[1], gt.shape[2],
                           float(lc.gamma), float(lc.alpha))


class SetLoss(torch.autograd.Function):
    """The focal and L1 losses of S decoder stages as one autograd node around `ops.set_loss`: forward(raw, num, scalars, code_weights,
    S logits..., S boxes...) stacks the stages, makes the one call and keeps the two gradient tensors; -> loss (S, 2).  backward scales the
    kept gradients by the incoming (S, 2) gradient -- two element-wise launches -- and hands every stage its view."""

    @staticmethod
    def forward(ctx, raw, num, scalars, code_weights, *preds):
        S = len(preds) // 2
        logits, boxes = torch.stack([p.detach() for p in preds[:S]]), torch.stack([p.detach() for p in preds[S:]])
        loss, ctx.grad_logits, ctx.grad_boxes = ops.set_loss(logits, boxes, raw["count"], raw["pred_idx"], raw["gt_idx"], raw["gt_boxes"],
                                                             raw["gt_labels"], code_weights, num, **scalars)
        return loss

    @staticmethod
    def backward(ctx, grad):
        S = grad.shape[0]
        gl = ctx.grad_logits * grad[:, 0].view(S, 1, 1, 1)
        gb = ctx.grad_boxes * grad[:, 1].view(S, 1, 1, 1)
        return (None, None, None, None) + gl.unbind(0) + gb.unbind(0)


def freeze_lidar_components(model):
    """tools/train.py:221-276: stop gradients in every pts_* sub-module and keep their BatchNorm in eval."""
    for name in ("pts_voxel_encoder", "pts_middle_encoder", "pts_backbone", "pts_neck"):
        mod = getattr(model, name, None)
        if mod is None:
            continue
        mod.eval()
        for p in mod.parameters():
            p.requires_grad = False
        mod.train = lambda mode=True, _m=mod: nn.Module.train(_m, False)  # stays in eval under model.train()
    return model
