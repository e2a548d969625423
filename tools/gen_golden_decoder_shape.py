"""Reference goldens for the decoder's shape keys (build container only: needs the reference tree; never run on the GPU machine).

    python -B tools/gen_golden_decoder_shape.py [case ...|train]     # writes tests/golden/decoder_shape_<case>.npz, decoder_shape_refnoise.npz,
                                                                     # decoder_shape_state_keys.json and decoder_shape_train.npz
                                                                     # (described in tests/golden/README_decoder_shape.md)

Builds the UNMODIFIED reference MV2DSHead / MV2DTHead with ``configs.roi_head_cfg_s / _t(num_layers=, feedforward_channels=)``, loads
``synthetic.with_decoder_shape_state(make_head_state(seed=0), 0, num_layers, feedforward_channels)`` and records through
``oracle.gen_golden.run_case`` under every execution variant of ``oracle.gen_golden_refnoise.VARIANTS``: the 't8' run is the golden (only the keys
tests/test_gpu_decoder_shape.py reads are kept), the others give the reference's own rank noise for that case.  The training record is the
forward_train record of oracle/gen_golden_train.py (its last section; that script has only a main(), so its steps are repeated here as in
tools/gen_golden_qg_shape_train.py) for ``train_micro_s`` at 3 layers and 448 channels under ``stage_loss_weights=[0.1] * 3``.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mv2d_amd import configs, synthetic  # noqa: E402
from oracle import _stubs, _stubs_train  # noqa: E402
from oracle.gen_golden import OUT, run_case  # noqa: E402
from oracle.gen_golden_refnoise import VARIANTS, ranked_diff  # noqa: E402

REFERENCE = '/root/reference'
NOISE_MAX = 4
SEED = 0              # of with_decoder_shape_state (README_decoder_shape.md says so if a case had to take the next one)
# (case name, problem, num_layers, feedforward_channels)
CASES = [('micro_s_l3', 'micro_s', 3, 2048),
         ('micro_t_l2_f448', 'micro_t', 2, 448),
         ('cfg1_t_l8_f576', 'cfg1_t', 8, 576),
         ('cfg1_s_l1_f4096', 'cfg1_s', 1, 4096),
         ('cfg1_s_f1024', 'cfg1_s', 6, 1024)]
KEEP = ('intr', 'center_pred', 'xyz', 'feat_for_rois', 'feat_for_rois_shape', 'key_padding', 'corr', 'corr_mask', 'ref', 'cls', 'reg', 'boxes', 'scores',
        'labels', 'topk_index', 'topk_scores')
TRAIN = ('train_micro_s', 3, 448)            # (entry of synthetic.FWD_TRAIN_CASES, num_layers, feedforward_channels)
TRAIN_OUT = os.path.join(OUT, 'decoder_shape_train.npz')
DEC = 'bbox_head.transformer.decoder.'


def case_state(num_layers, ffn, seed=SEED):
    return synthetic.with_decoder_shape_state(synthetic.make_head_state(seed=0), seed, num_layers, ffn)


def build_head(kind, S_cls, T_cls, sd_np, num_views, num_layers, ffn, train_cfg=None):
    cfg = (configs.roi_head_cfg_s if kind == 'S' else configs.roi_head_cfg_t)(num_layers=num_layers, feedforward_channels=ffn)
    cfg.pop('type')
    cfg['test_cfg'] = configs.TEST_CFG_RCNN
    if train_cfg is not None:
        cfg['train_cfg'] = train_cfg
    if kind == 'T':
        cfg['num_views'] = num_views
    head = (S_cls if kind == 'S' else T_cls)(**cfg).eval()
    missing, unexpected = head.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=False)
    assert not unexpected, unexpected
    assert all('loss' in m for m in missing), missing
    return head


def decoder_params(head):
    """The reference module's own decoder and per-layer branch parameter names and shapes."""
    return {k: list(v.shape) for k, v in head.state_dict().items()
            if k.startswith((DEC, 'bbox_head.cls_branches.', 'bbox_head.reg_branches.'))}


def inference(only):
    S_cls, T_cls = _stubs.install(REFERENCE)
    path = os.path.join(OUT, 'decoder_shape_refnoise.npz')
    store = dict(np.load(path)) if os.path.exists(path) else {}
    kpath = os.path.join(OUT, 'decoder_shape_state_keys.json')
    keys_json = json.load(open(kpath)) if os.path.exists(kpath) else {}
    for name, problem, num_layers, ffn in CASES:
        if only and name not in only:
            continue
        sd_np = case_state(num_layers, ffn)
        prob = synthetic.make_problem(problem, seed=0)
        recs = {}
        for vname, v in VARIANTS:
            torch.set_num_threads(v['threads'])
            torch.backends.mkldnn.enabled = v['mkldnn']
            head = build_head(prob['kind'], S_cls, T_cls, sd_np, prob['views_per_frame'], num_layers, ffn)
            recs[vname] = run_case(head, prob['kind'], prob['feat'], prob['proposals'], prob['img_metas'], False)
        torch.backends.mkldnn.enabled = True
        params = decoder_params(head)
        assert params == {k: list(v.shape) for k, v in sd_np.items() if k in params} and len(head.bbox_head.transformer.decoder.layers) == num_layers
        keys_json[name] = dict(kind=prob['kind'], problem=problem, num_layers=num_layers, feedforward_channels=ffn, seed=SEED, params=params)
        base = recs['t8']
        assert base['cls'].shape[0] == num_layers and base['reg'].shape[0] == num_layers
        rec = {k: base[k] for k in KEEP if k in base}
        out = os.path.join(OUT, f'decoder_shape_{name}.npz')
        np.savez_compressed(out, num_layers=np.int32(num_layers), feedforward_channels=np.int32(ffn), **rec)
        assert os.path.getsize(out) < 200 * 1024, (out, os.path.getsize(out))
        key = f'{name}_s0'
        store[key + '_variants'] = np.array([v for v, _ in VARIANTS])
        store[key + '_topk_index'] = np.stack([recs[v]['topk_index'] for v, _ in VARIANTS])
        store[key + '_topk_scores'] = np.stack([recs[v]['topk_scores'] for v, _ in VARIANTS])
        pair = np.array([[ranked_diff(recs[a]['topk_index'], recs[b]['topk_index']) for b, _ in VARIANTS] for a, _ in VARIANTS], np.int32)
        store[key + '_pairwise_ranked_diff'] = pair
        assert int(pair.max()) <= NOISE_MAX, (name, int(pair.max()), 'take the next seed and say so in README_decoder_shape.md')
        gaps = [0.0]
        pos_ = {int(x): j for j, x in enumerate(base['topk_index'])}
        for v, _ in VARIANTS[1:]:
            for i, x in enumerate(recs[v]['topk_index']):
                j = pos_.get(int(x))
                if j is not None and j != i:
                    gaps.append(abs(float(base['topk_scores'][i]) - float(base['topk_scores'][j])))
        store[key + '_max_tie_gap'] = np.float64(max(gaps))
        store[key + '_cls_dev'] = np.float64(max(float(np.abs(recs[v]['cls'] - base['cls']).max()) for v, _ in VARIANTS[1:]) /
                                             float(np.abs(base['cls']).max()))
        np.savez_compressed(path, **store)
        json.dump(keys_json, open(kpath, 'w'), indent=1, sort_keys=True)
        print(key, {k: v.shape for k, v in rec.items()}, os.path.getsize(out), 'bytes; max ranked diff', int(pair.max()), 'gap %.2e' % max(gaps), flush=True)


def train():
    (S_cls, T_cls), Assigner = _stubs_train.install(REFERENCE)
    name, num_layers, ffn = TRAIN
    train_cfg = dict(configs.TRAIN_CFG_RCNN, stage_loss_weights=[0.1] * num_layers)
    prob_name, kind, G, seed = synthetic.FWD_TRAIN_CASES[name]
    prob = synthetic.make_problem(prob_name, seed=0)
    with_dn = kind.endswith('+DN')
    kind = kind[0]
    # one thread: the CPU backward accumulates gradients across threads in an order that varies from run to run (1e-10 relative in the stored
    # norms); single-threaded, the record regenerates byte for byte
    torch.set_num_threads(1)
    h = build_head(kind, S_cls, T_cls, case_state(num_layers, ffn), prob['views_per_frame'], num_layers, ffn, train_cfg=train_cfg)
    if with_dn:
        h.use_denoise = True
    cfgk = (configs.roi_head_cfg_s() if kind == 'S' else configs.roi_head_cfg_t())['bbox_head']
    _stubs_train.arm_bbox_head(h.bbox_head, Assigner, train_cfg, cfgk['loss_cls'], cfgk['loss_bbox'])
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
    rec = {}
    for k, v in losses.items():
        rec[f'{name}.loss.{k}'] = np.float32(float(v))
    assert {k for k in losses if k.startswith('l')} >= {f'l{i}.loss_cls' for i in range(num_layers)} and f'l{num_layers}.loss_cls' not in losses
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
    rec[f'{name}.grad_names'] = np.array(names)
    rec[f'{name}.grad_norm'] = np.array(norms)
    rec[f'{name}.grad_proj'] = np.array(projs)
    res = captured['res']
    rec[f'{name}.cls'] = torch.stack(res['pred']['cls_scores']).detach().numpy()
    rec[f'{name}.reg'] = torch.stack(res['pred']['bbox_preds']).detach().numpy()
    gtc9 = torch.cat((gt.gravity_center, gt.tensor[:, 3:]), 1)
    rec[f'{name}.match'] = np.stack([(h.bbox_head.assigner.assign(b.detach(), c.detach(), gtc9, labels).gt_inds - 1).numpy()
                                     for c, b in zip(res['pred']['cls_scores'], res['pred']['bbox_preds'])]).astype(np.int32)
    assert rec[f'{name}.cls'].shape[0] == num_layers
    np.savez_compressed(TRAIN_OUT, num_layers=np.int32(num_layers), feedforward_channels=np.int32(ffn), **rec)
    assert os.path.getsize(TRAIN_OUT) < 200 * 1024
    print(name, {k: round(float(v), 5) for k, v in list(losses.items())[-4:]}, 'grads', len(names), 'rows', rec[f'{name}.cls'].shape, flush=True)


def main():
    only = [a for a in sys.argv[1:] if not a.startswith('-')]
    if not only or any(a != 'train' for a in only):
        inference([a for a in only if a != 'train'])
    if not only or 'train' in only:
        train()


if __name__ == '__main__':
    main()
