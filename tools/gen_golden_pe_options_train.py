"""Reference training golden for the PE's switches (build container only: needs the reference tree; never run on the GPU machine).

    python -B tools/gen_golden_pe_options_train.py      # writes tests/golden/pe_options_train.npz (described in tests/golden/README_pe_options.md)

The forward_train record of tools/gen_golden_pe_depth_train.py (the fields of tests/golden/pe_depth_train_d32.npz / train_loss.npz) for
``train_micro_t`` with ``pe.with_fpe = False`` and ``train_micro_s`` with ``pe.no_sin_enc = True, pe.LID = False``, with the UNMODIFIED reference heads
(configs.roi_head_cfg_s / _t with those keys) on ``synthetic.with_pe_options_state(make_head_state(seed=0), ...)``: the losses, the match of every
layer, gradient norms and probe projections of every parameter, and the feature-map gradient's norm, projection and per-view norms.
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
from tools.gen_golden_pe_options import build_head, case_state  # noqa: E402

REFERENCE = '/root/reference'
CASES = [('train_micro_t', dict(with_fpe=False)), ('train_micro_s', dict(no_sin_enc=True, LID=False))]
OUT = os.path.join(ROOT, 'tests', 'golden', 'pe_options_train.npz')


def main():
    (S_cls, T_cls), Assigner = _stubs_train.install(REFERENCE)
    rec = {}
    for name, pe_keys in CASES:
        prob_name, kind, G, seed = synthetic.FWD_TRAIN_CASES[name]
        prob = synthetic.make_problem(prob_name, seed=0)
        with_dn = kind.endswith('+DN')
        kind = kind[0]
        h = build_head(kind, S_cls, T_cls, case_state(pe_keys), prob['views_per_frame'], pe_keys, train_cfg=configs.TRAIN_CFG_RCNN)
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
        assert 'position_encoding.position_encoder.0.weight' in names
        assert not any('.fpe.' in n for n in names) or pe_keys.get('with_fpe', True)
        assert not any('.adapt_pos3d.' in n for n in names) or not pe_keys.get('no_sin_enc', False)
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
    assert os.path.getsize(OUT) < 200 * 1024, os.path.getsize(OUT)


if __name__ == '__main__':
    main()
