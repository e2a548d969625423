"""Reference training goldens for two query-generator shapes (build container only: needs the reference tree; never run on the GPU machine).

    python -B tools/gen_golden_qg_shape_train.py      # writes tests/golden/qg_shape_train.npz (described in tests/golden/README_qg_shape.md)

The forward_train record of oracle/gen_golden_train.py (its last section; that script has only a main(), so its steps are repeated here) for
one S and one T entry of ``synthetic.FWD_TRAIN_CASES``, with the UNMODIFIED reference heads built with the ``query_generator`` keys of the
inference cases micro_s_c2 and cfg1_t_c0_f2 (tools/gen_golden_qg_shape.py) on ``synthetic.with_qg_shape_state(make_head_state(seed=0), 0, keys)``.  Same fields as tests/golden/train_loss.npz: the losses, the match of every layer, gradient norms
and probe projections of every parameter, and the feature-map gradient's norm, projection and per-view norms.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mv2d_amd import configs, synthetic  # noqa: E402
from oracle import _stubs_train  # noqa: E402
from tools import gen_golden_qg_shape as gen  # noqa: E402

REFERENCE = '/root/reference'
# (entry of synthetic.FWD_TRAIN_CASES, inference case whose query_generator keys the head is built with)
CASES = [('train_micro_s', 'micro_s_c2'), ('train_cfg1_t', 'cfg1_t_c0_f2')]
OUT = os.path.join(ROOT, 'tests', 'golden', 'qg_shape_train.npz')


def build_head(kind, S_cls, T_cls, num_views, case):
    _, _, roi_size, keys = next(c for c in gen.CASES if c[0] == case)
    head = gen.build_head(kind, S_cls, T_cls, gen.case_state(keys, roi_size), num_views, keys, roi_size, train=True)
    assert {k: tuple(v.shape) for k, v in head.query_generator.state_dict().items()} == gen.qg_shape.parse(keys).param_shapes(roi_size)
    return head


def main():
    (S_cls, T_cls), Assigner = _stubs_train.install(REFERENCE)
    rec = {}
    for name, case in CASES:
        prob_name, kind, G, seed = synthetic.FWD_TRAIN_CASES[name]
        prob = synthetic.make_problem(prob_name, seed=0)
        with_dn = kind.endswith('+DN')
        kind = kind[0]
        h = build_head(kind, S_cls, T_cls, prob['views_per_frame'], case)
        if with_dn:
            h.use_denoise = True
        cfgk = (configs.roi_head_cfg_s() if kind == 'S' else configs.roi_head_cfg_t())['bbox_head']
        _stubs_train.arm_bbox_head(h.bbox_head, Assigner, configs.TRAIN_CFG_RCNN, cfgk['loss_cls'], cfgk['loss_bbox'])
        h.train()
        for m in h.modules():
            if isinstance(m, nn.Dropout):
                m.p = 0.0
            if isinstance(m, nn.MultiheadAttention):
                m.dropout = 0.0
        gtc = synthetic.make_train_gt(G, seed)
        gt = _stubs_train.GtBoxes(torch.from_numpy(gtc['gt_bottom']))
        labels = torch.from_numpy(gtc['gt_labels'])
        rnd = torch.from_numpy(synthetic.make_dn_noise(G * 10, seed))
        metas = [dict(m, box_type_3d=(lambda b, d: b)) for m in prob['img_metas']]
        props = [torch.from_numpy(p) for p in prob['proposals']]
        captured = {}
        orig = h._bbox_forward_train

        def wrapped(*a, **k):
            r = orig(*a, **k)
            captured['res'] = r
            return r
        h._bbox_forward_train = wrapped
        cuda, rand_like = torch.Tensor.cuda, torch.rand_like
        torch.Tensor.cuda = lambda self, *a, **k: self
        torch.rand_like = lambda t, *a, **k: rnd.to(t.dtype)
        try:
            xg = torch.from_numpy(prob['feat']).clone().requires_grad_(True)
            losses = h.forward_train([xg], metas, props, None, None, None, None, [gt], [labels], None)
        finally:
            torch.Tensor.cuda, torch.rand_like = cuda, rand_like
        for k, v in losses.items():
            rec[f'{name}.loss.{k}'] = np.float32(float(v))
        sum(losses.values()).backward()
        names, norms, projs = [], [], []
        for pn, q in h.named_parameters():
            if q.grad is not None:
                names.append(pn)
                norms.append(float(q.grad.double().norm()))
                projs.append(float((q.grad.double().flatten() * torch.from_numpy(synthetic.grad_probe(pn, q.numel())).double()).sum()))
        rec[f'{name}.dfeat_norm'] = np.float64(float(xg.grad.double().norm()))
        rec[f'{name}.dfeat_proj'] = np.float64(float((xg.grad.double().flatten() * torch.from_numpy(synthetic.grad_probe('feat', xg.numel())).double()).sum()))
        rec[f'{name}.dfeat_view_norms'] = xg.grad.double().flatten(1).norm(dim=1).numpy()
        assert all('query_generator.' + k in names for k in h.query_generator.state_dict())   # (every parameter of the shape has a gradient)
        rec[f'{name}.grad_names'] = np.array(names)
        rec[f'{name}.grad_norm'] = np.array(norms)
        rec[f'{name}.grad_proj'] = np.array(projs)
        res = captured['res']
        rec[f'{name}.cls'] = torch.stack(res['pred']['cls_scores']).detach().numpy()
        rec[f'{name}.reg'] = torch.stack(res['pred']['bbox_preds']).detach().numpy()
        gtc9 = torch.cat((gt.gravity_center, gt.tensor[:, 3:]), 1)
        rec[f'{name}.match'] = np.stack([(h.bbox_head.assigner.assign(b.detach(), c.detach(), gtc9, labels).gt_inds - 1).numpy()
                                         for c, b in zip(res['pred']['cls_scores'], res['pred']['bbox_preds'])]).astype(np.int32)
        md = res.get('dn_mask_dict')
        if md:
            rec[f'{name}.dn_cls'] = md['output_known_lbs_bboxes'][0][:, 0].detach().numpy()
            rec[f'{name}.dn_reg'] = md['output_known_lbs_bboxes'][1][:, 0].detach().numpy()
        print(name, {k: round(float(v), 5) for k, v in list(losses.items())[-4:]}, 'grads', len(names), 'rows', rec[f'{name}.cls'].shape, flush=True)
    np.savez_compressed(OUT, **rec)


if __name__ == '__main__':
    main()
