"""The steps either side of the RoI-head boundary ("next" rows f1 / f2 of SURVEY.md §8(f)).

* ``process_2d_detections`` — MV2D.process_2d_detections (mmdet3d_plugin/models/detectors/mv2d.py:60-86): per-class arrays of the 2-D
  detector -> one [n,6] (x1,y1,x2,y2,score,label) tensor per view + the min_bbox_size filter.  Host-side data plumbing.
* ``pack_results`` — the 3-D "NMS" + result packing after the head (mv2d.py:265-293).  With the shipped ``nms_thr=1.0`` mmdet3d's
  box3d_multiclass_nms suppresses nothing (a rotated IoU never exceeds 1): it only drops scores <= score_thr, orders the boxes
  class-major / score-descending and caps them at max_per_scene.  Runs as one tiny HIP kernel (mv2d_result_pack).
  mmdet3d is third-party and absent from the reference tree: this row is parity-unpinned (restated from mmdet3d 1.0.0).
"""
import numpy as np
import torch

from . import ops
from .engine import native_map


def process_2d_detections(results, device, min_bbox_size=0):
    dets = []
    for res in results:
        rows = [torch.cat([torch.as_tensor(np.asarray(b), dtype=torch.float32).reshape(-1, 5),
                           torch.full((len(b), 1), float(label_id), dtype=torch.float32)], 1) for label_id, b in enumerate(res)]
        det = torch.cat(rows, 0) if rows else torch.zeros((0, 6))
        if min_bbox_size > 0:
            wh = det[:, 2:4] - det[:, 0:2]
            det = det[(wh >= min_bbox_size).all(1)]
        dets.append(det.to(device))
    return dets


_NMS_WARNED = [False]


def _warn_unpinned_nms():
    # mmcv 1.6.1's nms_bev is absent from the reference tree: the rotated-IoU suppression is pinned against this repo's oracle only
    # (LOG.md section 7.1 f1).  Every shipped config uses nms_thr = 1.0 and never gets here.
    if not _NMS_WARNED[0]:
        import warnings
        warnings.warn('mv2d_amd: nms_thr < 1 runs mv2d_nms_bev, whose parity with mmcv 1.6.1 nms_bev is not pinned by a reference-side golden '
                      '(no shipped MV2D config sets nms_thr < 1)', RuntimeWarning)
        _NMS_WARNED[0] = True


def pack_results(boxes, scores, labels, count, score_thr=0.0, max_per_scene=300, nms_thr=1.0):
    """boxes [n,9], scores [n], labels [n] (device, first *count valid) -> dict(boxes_3d, scores_3d, labels_3d) on the host
    (mmdet3d bbox3d2result), ordered like box3d_multiclass_nms.  nms_thr < 1: rotated BEV suppression per class first (mv2d_nms_bev)."""
    dev = boxes.device
    if float(nms_thr) < 1.0:
        _warn_unpinned_nms()
        scores = ops.nms_bev(boxes, scores, labels, count, nms_thr)
    ob = torch.zeros((max_per_scene, 9), device=dev)
    os_ = torch.zeros(max_per_scene, device=dev)
    ol = torch.zeros(max_per_scene, dtype=torch.int64, device=dev)
    oc = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.result_pack(boxes.contiguous(), scores.contiguous(), labels.contiguous(), count, score_thr, max_per_scene, ob, os_, ol, oc)
    n = int(oc.item())
    return dict(boxes_3d=ob[:n].cpu(), scores_3d=os_[:n].cpu(), labels_3d=ol[:n].cpu())


def pack_results_batch(boxes, scores, labels, count, score_thr=0.0, max_per_scene=300, nms_thr=1.0):
    """run_batch outputs (boxes [B,n,9], scores [B,n], labels [B,n], count [B]) -> B dicts like pack_results, one launch and one host
    synchronisation for the whole batch."""
    dev, B = boxes.device, count.numel()
    if float(nms_thr) < 1.0:
        _warn_unpinned_nms()
        scores = ops.nms_bev(boxes, scores, labels, count, nms_thr, n_samples=B)
    ob = torch.zeros((B, max_per_scene, 9), device=dev)
    os_ = torch.zeros((B, max_per_scene), device=dev)
    ol = torch.zeros((B, max_per_scene), dtype=torch.int64, device=dev)
    oc = torch.zeros(B, dtype=torch.int32, device=dev)
    ops.result_pack(boxes.contiguous(), scores.contiguous(), labels.contiguous(), count, score_thr, max_per_scene, ob, os_, ol, oc,
                    n_samples=B, in_stride=scores.shape[-1])
    ns = oc.tolist()
    ob, os_, ol = ob.cpu(), os_.cpu(), ol.cpu()
    return [dict(boxes_3d=ob[b, :n], scores_3d=os_[b, :n], labels_3d=ol[b, :n]) for b, n in enumerate(ns)]


def simple_test_batch_from_detections(roi_head, feat_maps, det_results_list, img_metas_list, rcnn_test_cfg, min_bbox_size=0, wrap_pts_bbox=False):
    """simple_test_from_detections for a batch of samples: feat_maps[lvl] = the stacked [B*V,256,h,w] map, det_results_list / img_metas_list
    = one entry per sample.  One sequence of launches, one host synchronisation."""
    nms_thr = float(rcnn_test_cfg.get('nms', rcnn_test_cfg).get('nms_thr', 1.0))
    feat = feat_maps[roi_head.feat_lvl]
    proposals = [process_2d_detections(d, feat.device, min_bbox_size) for d in det_results_list]
    eng = roi_head.engine(feat.device, img_metas_list[0])
    out = eng.run_batch(native_map(feat), proposals, img_metas_list)
    res = pack_results_batch(out['boxes'], out['scores'], out['labels'], out['count'], rcnn_test_cfg.get('score_thr', 0.0),
                             rcnn_test_cfg.get('max_per_scene', 300), nms_thr)
    if int(out['ws']['nnz'][1].item()) != 0:
        raise RuntimeError('mv2d engine: CSR capacity exceeded (raise col_cap_per_query)')
    for b, r in enumerate(res):
        box_type = img_metas_list[b][0].get('box_type_3d')
        if box_type is not None:
            r['boxes_3d'] = box_type(r['boxes_3d'], r['boxes_3d'].size(-1))
    return [dict(pts_bbox=r) for r in res] if wrap_pts_bbox else res


def simple_test_from_detections(roi_head, feat_maps, det_results, img_metas, rcnn_test_cfg, min_bbox_size=0, wrap_pts_bbox=False):
    """The part of MV2D.simple_test (mv2d.py:225-295, batch 1) that surrounds the RoI head: 2-D detector results ->
    proposals -> head (HIP engine) -> result packing, with one host synchronisation at the very end.
    rcnn_test_cfg: dict(score_thr, max_per_scene, nms=dict(nms_thr)) (CFG-T:154-158).  wrap_pts_bbox=True returns the reference's
    ``[{'pts_bbox': {...}}]`` (mv2d.py:283-292) instead of the bare dict."""
    nms_thr = float(rcnn_test_cfg.get('nms', rcnn_test_cfg).get('nms_thr', 1.0))
    feat = feat_maps[roi_head.feat_lvl]
    proposals = process_2d_detections(det_results, feat.device, min_bbox_size)
    eng = roi_head.engine(feat.device, img_metas)
    out = eng.run(native_map(feat), proposals, img_metas)
    res = pack_results(out['boxes'], out['scores'], out['labels'], out['count'], rcnn_test_cfg.get('score_thr', 0.0),
                       rcnn_test_cfg.get('max_per_scene', 300), nms_thr)
    if int(out['ws']['nnz'][1].item()) != 0:
        raise RuntimeError('mv2d engine: CSR capacity exceeded (raise col_cap_per_query)')
    box_type = img_metas[0].get('box_type_3d')
    if box_type is not None:
        res['boxes_3d'] = box_type(res['boxes_3d'], res['boxes_3d'].size(-1))
    return [dict(pts_bbox=res)] if wrap_pts_bbox else [res]
