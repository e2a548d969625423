"""Fused MI355X inference engine for the MV2D RoI head hot path.

One ``HeadEngine`` owns the packed weights (fp16 hi / lo pairs, fragment-major, for the split-precision kernels of the key and the query side;
single fp16 copies for the query generator's conv), a shape-keyed workspace (every buffer pre-allocated, kernels never allocate) and enqueues the whole
frame on the current HIP stream through the C-ABI (mv2d_amd.ops) without a single device->host synchronisation:

  T path (MV2DTHead, RH/mv2d_t_head.py:26-142)        S path (MV2DSHead eval branch, RH/mv2d_s_head.py:122-211)
  rois -> per-RoI camera -> RoIAlign(feat) -> QueryGenerator -> ref points -> query_pos
  box correlation -> match lists                        box correlation (k=1) -> CSR over RoI-feature rows
  masks -> key list S + CSR (device-side counts)        RoI tap positions -> PE there -> RoIAlign(feat, pe)
  PE only at the S key positions -> key rows (feat + pe) / value rows (feat), key16, shared by all layers and heads
  6 x [self-attn, LN, cross-attn in the raw key space (K / V in_proj folded into the query side), LN, FFN, LN] -> heads -> top-k decode

The reference evaluates PE on the whole map and runs dense [8,R,S] attention with a boolean mask.  The engine's route is the INDEX-EXACT one
(round 5: the default): every operand an fp16 hi + lo pair, three MFMAs per product -- the ranked box indices equal the reference's (DESIGN.md
section 2).  ``exact=False`` selects the opt-in key16 mode (one fp16 rounding of the key side: faster, a few ranked indices move).
"""
import math
import os

import numpy as np
import torch

from . import calib, ops, pe_cache, qg_shape, route

BF16 = torch.bfloat16
F32 = torch.float32
C = 256
L_DEFAULT = 6


def _t(x, device, dtype=None):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    x = x.detach()
    if dtype is not None:
        x = x.to(dtype)
    return x.to(device).contiguous()


def native_map(feat):
    """The stride-16 map as the engine takes it: fp32, fp16 and bf16 maps are handed on as they are (a mixed-precision backbone's 16-bit map is
    read natively, no fp32 copy); any other dtype is cast to fp32 as before."""
    return feat if feat.dtype in ops.MAP_FMT else feat.float()


class HeadEngine:
    def __init__(self, state_dict, kind, device, num_views=6, topk=None, expand_stride=None, num_layers=L_DEFAULT,
                 max_num=300, pc_range=(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0),
                 post_range=(-61.2, -61.2, -10.0, 61.2, 61.2, 10.0), depth_num=64, stride=16, col_cap_per_query=2048,
                 iou_thr=0.0, ratio=0.0, masked_row='nan', exact=None, num_classes=10, roi_size=7, use_reg_layer=False,
                 group_reg_dims=(2, 2, 1, 1, 2, 2), depth_start=1, position_range=None, query_generator=None, num_reg_fcs=2,
                 with_fpe=True, no_sin_enc=False, adapt_pos3d=True, LID=True, feedforward_channels=2048, sample_size=4, num_depth=8,
                 corr_depth_start=0.5, corr_depth_end=70, corr_LID=True, intrins_feat_scale=0.1):
        assert kind in ('S', 'T')
        self.kind = kind
        self.dev = torch.device(device)
        # the decoder's shape (ops.check_decoder_shape: 1 to 8 layers, an FFN width that is a multiple of 64 in [64, 4096]).  Fixed per engine: the
        # state dict has to agree (load_state).  The FFN always accumulates ops.FFN_GROUPS = 8 hidden slices per block, so a width gives
        # ceil(F / 512) slabs -- exactly what the workspaces allocate and the FFN tail sums; a width that is no multiple of 512 launches the ragged
        # instance of the FFN kernel (csrc/ffn_x3.hip), the shipped 2048 allocates, packs and launches what it always did.
        self.L, self.ffn_dim = ops.check_decoder_shape(num_layers, feedforward_channels, 'HeadEngine')
        self.ffn_slabs = ops.ffn_slabs(self.ffn_dim)
        self.num_views = num_views
        self.topk = topk if topk is not None else (1 if kind == 'S' else 20)
        self.expand = float(expand_stride if expand_stride is not None else (0 if kind == 'S' else 2))
        self.max_num = max_num
        self.num_classes = int(num_classes)
        if not 1 <= self.num_classes <= 64:       # the class output layer of the branch kernels: up to 4 column tiles of 16
            raise ValueError(f'HeadEngine: num_classes must be in [1, 64], got {num_classes}')
        # RoIAlign output size s (square): s x s bins per RoI -> s * s RoI cells (query-generator conv input; the S path's keys per RoI)
        self.roi_size = int(roi_size)
        if self.roi_size != roi_size or not 1 <= self.roi_size <= 14:
            raise ValueError(f'HeadEngine: roi_size must be an int in [1, 14], got {roi_size}')
        self.cells = self.roi_size * self.roi_size
        # the query generator's shape: a dict of the reference QueryGenerator's own config keys (mv2d_amd/qg_shape.py lists what is accepted; None =
        # the shipped shape, which allocates and launches exactly what it always did).  Fixed per engine: the state dict has to agree (load_state).
        self.qg = qg_shape.parse(query_generator, 'HeadEngine')
        # the regression branches as the reference's RegLayer (CrossAttentionBoxHead(use_reg_layer=True): two shared linears, one task head per
        # entry of group_reg_dims) -- mv2d_reg_layer_depth_x3 next to the class-only launch of the fused branches.  Fixed per engine: the state dict's
        # key layout has to agree (load_state), and it is part of the graph key.
        self.use_reg_layer = bool(use_reg_layer)
        self.group_reg_dims = ops.check_group_reg_dims(group_reg_dims) if self.use_reg_layer else tuple(group_reg_dims)
        # hidden layers per prediction branch (the head's num_reg_fcs; RegLayer's shared layers): every depth launches the depth entries with [L][n]
        # tables (csrc/branches_x3.hip picks the kernel instance from n).  Fixed per engine: the state dict's branches have to have that depth.
        self.num_reg_fcs = ops.check_num_reg_fcs(num_reg_fcs, 'HeadEngine')
        # the PE's depth_num / depth_start / position_range (MU/pe.py:52-63).  Every consumer of the frustum rows takes them with Kp = pe_kp(depth_num)
        # columns (3 * depth_num zero-padded to a multiple of 32) and position_encoder.0.weight zero-padded to [1024, Kp]: one instance of the fused PE
        # kernel per Kp / 32 (csrc/pe_x3_kernel.h).  position_range=None: the coder's post_range, as in the shipped configs; the decode's centre filter
        # always uses post_range.
        self.depth_num = ops.check_pe_depth(depth_num, 'HeadEngine')
        self.pe_kp = ops.pe_kp(self.depth_num)
        self.depth_start, pe_range = ops.check_pe_range(depth_start, post_range if position_range is None else position_range, 'HeadEngine')
        self.pe_range_h64 = torch.tensor(pe_range, dtype=torch.float64)
        # the PE's four switches (MU/pe.py:51-82; ops.check_pe_options).  Fixed per engine: the state dict's key layout has to agree (load_state).  The
        # shipped values allocate, pack and launch what they always did; with_fpe=False runs the gate-less instance of the fused PE kernel
        # (mv2d_pe_fused_x3_ng: no fpe weights), no_sin_enc=True feeds either instance one all-zero table row (no adapt_pos3d weights, no sine rows),
        # LID=False only changes the depth table.  Anything but the shipped values runs on the index-exact route only (route.resolve).
        self.with_fpe, self.no_sin_enc, self.adapt_pos3d, self.LID = ops.check_pe_options(with_fpe, no_sin_enc, adapt_pos3d, LID, 'HeadEngine')
        self.stride = stride
        self.iou_thr, self.ratio = iou_thr, ratio
        self.col_cap_per_query = col_cap_per_query
        # a query whose every key is masked: 'nan' = the reference's behaviour (nn.MultiheadAttention yields NaN, the next self
        # attention spreads it to every query, the frame returns no boxes), 'zero' = zero attention output for that query only
        assert masked_row in ('nan', 'zero')
        self.empty_nan = masked_row == 'nan'
        self.pc_range_h = torch.tensor(pc_range, dtype=F32)
        self.post_range_h = torch.tensor(post_range, dtype=F32)
        self.post_range_h64 = torch.tensor(post_range, dtype=torch.float64)
        # box_correlation's sampling keys (RH/utils/box_correlation.py:12-21; ops.check_box_correlation: the accepted values) and the head's
        # intrins_feat_scale.  Fixed per engine, like depth_num: self.const holds their sample grid and depth table, the frame launch gets them with
        # every frame.  The shipped values build and launch what they always did; more than 128 samples per (RoI, view), or a depth_start that is no
        # fp32 number, launch the second instance of the correlation block (csrc/geometry.hip).
        self.sample_size, self.num_depth, self.corr_depth_start, self.corr_depth_end, self.corr_LID = ops.check_box_correlation(
            sample_size, num_depth, corr_depth_start, corr_depth_end, corr_LID, 'HeadEngine')
        self.intrins_feat_scale = ops.check_intrins_feat_scale(intrins_feat_scale, 'HeadEngine')
        self.const = {k: v.to(self.dev) for k, v in calib.constant_tables(self.sample_size, self.num_depth, self.corr_depth_start, self.corr_depth_end,
                                                                          lid=self.corr_LID).items()}
        self._ws = {}
        self._ws_base = {}
        self._shape_cache = {}
        # ---- route options: plain attributes, settable on a live engine (the next call follows them: its workspace and its graph are keyed by
        # the route they resolve to).  Names, defaults and what each one does: mv2d_amd/route.py.  The only other environment variable the engine
        # reads is MV2D_EXACT (route.Route.exact).
        self.__dict__.update(route.default_options())
        if not self.qg.is_default:
            # other query-generator shapes chain their convs cell to cell: on the index-exact route they run in split precision (the shipped shape
            # keeps its key16 conv there by default: exact_skip = {'conv'}); with 'conv' put back into exact_skip the engine refuses the frame
            self.exact_skip = self.exact_skip - {'conv'}
        # adapt_pos3d(sine) (MU/pe.py:164-166) depends only on the weights and on the padding geometry of the rig, not on features, boxes
        # or calibration: it is constant-folded into a per-(weights version, geometry) table that the fused PE kernel adds in its epilogue
        self._weights_version = 0     # bumped by every load_state(): invalidates whatever was folded from the weights
        self.pe_cache_builds = 0      # tables of the cached frustum MLP this engine built (route options pe_cache / pe_cache_views: _build_pe_q / _build_pe_q_views, once per frame that builds)
        self.exact = (os.environ.get('MV2D_EXACT', '1') != '0') if exact is None else bool(exact)
        self.K16 = ops.key16_dtype()  # dtype of the key side's 16-bit buffers (csrc/common.h "key16": fp16 since round 4)
        self.load_state(state_dict)

    # ------------------------------------------------------------------------------------------ weights
    def load_state(self, sd):
        d, L, nf = self.dev, self.L, self.num_reg_fcs
        self.check_decoder_shape(sd, L, self.ffn_dim)
        self.check_reg_layout(sd, self.use_reg_layer, self.group_reg_dims)
        self.check_branch_depth(sd, nf, self.use_reg_layer)
        self.check_pe_layout(sd, self.with_fpe, self.no_sin_enc)
        nc = int(tuple(sd[f'bbox_head.cls_branches.0.{3 * nf}.weight'].shape)[0])
        if nc != self.num_classes:
            raise ValueError(f'HeadEngine: the state dict has {nc} classes (cls_branches.*.{3 * nf}.weight), num_classes={self.num_classes}')
        k1 = int(tuple(sd['position_encoding.position_encoder.0.weight'].shape)[1])
        if k1 != 3 * self.depth_num:
            raise ValueError(f'HeadEngine: the state dict has {k1} frustum channels (position_encoder.0.weight), 3 * depth_num = {3 * self.depth_num}')
        self._weights_version = getattr(self, '_weights_version', 0) + 1
        g = lambda k: _t(sd[k], d, F32)
        k16 = ops.pack_key16                                                             # fp32 [N,K] -> key16, fragment-major (key-side kernels)
        w = {}
        dec = 'bbox_head.transformer.decoder.'
        for i in range(L):
            p = f'{dec}layers.{i}.'
            w[f'sa_in_b{i}'] = g(p + 'attentions.0.attn.in_proj_bias')
            w[f'sa_out_b{i}'] = g(p + 'attentions.0.attn.out_proj.bias')
            inw, inb = g(p + 'attentions.1.attn.in_proj_weight'), g(p + 'attentions.1.attn.in_proj_bias')
            w[f'ca_q_b{i}'] = inb[:C].contiguous()
            # packed operands of xattn_qmap / xattn_ctxmap: the K / V in_proj ride on the query side (bf16x3)
            w[f'ca_mapA{i}'], w[f'ca_mapB{i}'] = ops.pack_xattn_maps(inw[C:2 * C].contiguous(), inw[2 * C:].contiguous())
            w[f'ca_v_b{i}'] = inb[2 * C:].contiguous()
            w[f'ca_out_b{i}'] = g(p + 'attentions.1.attn.out_proj.bias')
            w[f'ffn_b1{i}'] = g(p + 'ffns.0.layers.0.0.bias')
            w[f'ffn_b2{i}'] = g(p + 'ffns.0.layers.1.bias')
            # bf16x3 + fragment-major copies (row-fused kernels, fused FFN)
            w[f'sa_in_wx{i}'] = ops.pack_x3(g(p + 'attentions.0.attn.in_proj_weight'))
            w[f'sa_out_wx{i}'] = ops.pack_x3(g(p + 'attentions.0.attn.out_proj.weight'))
            w[f'ca_q_wx{i}'] = ops.pack_x3(inw[:C].contiguous())
            w[f'ca_out_wx{i}'] = ops.pack_x3(g(p + 'attentions.1.attn.out_proj.weight'))
            w[f'ffn_w1x{i}'] = ops.pack_x3(g(p + 'ffns.0.layers.0.0.weight'))
            w[f'ffn_w2x{i}'] = ops.pack_x3(g(p + 'ffns.0.layers.1.weight'))
            for n in range(3):
                w[f'ln{n}_w{i}'] = g(p + f'norms.{n}.weight')
                w[f'ln{n}_b{i}'] = g(p + f'norms.{n}.bias')
        w['post_w'], w['post_b'] = g(dec + 'post_norm.weight'), g(dec + 'post_norm.bias')
        w['qe_b0'], w['qe_b2'] = g('bbox_head.query_embedding.0.bias'), g('bbox_head.query_embedding.2.bias')
        w['qe_w0x'], w['qe_w2x'] = ops.pack_x3(g('bbox_head.query_embedding.0.weight')), ops.pack_x3(g('bbox_head.query_embedding.2.weight'))
        # the box head's weight tables, one layout for every depth (csrc/branches_x3.hip STACKED): the nf hidden layers of a branch in one [L][nf]
        # array, every tensor layer-major.  Class block i at cls_branches.{l}.{3i, 3i+1}, output at {3nf}; Sequential regression block i at {2i},
        # output at {2nf}; RegLayer shared block i at reg_branch.{3i}, then one task head per entry of group_reg_dims
        st = lambda fmt: torch.stack([g(fmt.format(l)) for l in range(L)]).contiguous()
        stn = lambda fmt, idx: torch.stack([torch.stack([g(fmt.format(l, i)) for i in idx]) for l in range(L)]).contiguous()
        cb, rb = 'bbox_head.cls_branches.{}.', 'bbox_head.reg_branches.{}.'
        lin_i, ln_i, seq_i = [3 * i for i in range(nf)], [3 * i + 1 for i in range(nf)], [2 * i for i in range(nf)]
        cls_src = (stn(cb + '{}.weight', lin_i), stn(cb + '{}.bias', lin_i), stn(cb + '{}.weight', ln_i), stn(cb + '{}.bias', ln_i),
                   st(cb + f'{3 * nf}.weight'), st(cb + f'{3 * nf}.bias'))
        if self.use_reg_layer:
            G = len(self.group_reg_dims)
            stg = lambda fmt, cat: torch.stack([cat([g(rb.format(l) + fmt.format(g_)) for g_ in range(G)]) for l in range(L)]).contiguous()
            cls_t, _ = ops.pack_heads_depth(*cls_src)
            reg_t = ops.pack_reg_layer_depth(stn(rb + 'reg_branch.{}.weight', lin_i), stn(rb + 'reg_branch.{}.bias', lin_i),
                                             stg('task_heads.{}.0.weight', torch.stack), stg('task_heads.{}.0.bias', torch.stack),
                                             stg('task_heads.{}.2.weight', torch.cat), stg('task_heads.{}.2.bias', torch.cat))
        else:
            cls_t, reg_t = ops.pack_heads_depth(*cls_src, stn(rb + '{}.weight', seq_i), stn(rb + '{}.bias', seq_i),
                                                st(rb + f'{2 * nf}.weight'), st(rb + f'{2 * nf}.bias'))
        w['head_tables'] = cls_t, reg_t = tuple(cls_t), tuple(reg_t)
        self.cls_ptrs_x3, self.reg_ptrs_x3 = ops.make_ptr_array(list(cls_t)), ops.make_ptr_array(list(reg_t))
        # the same tensors from the last decoder layer on: the launch of the last_stage_heads option
        self._last_cls, self._last_reg = [t[L - 1:] for t in cls_t], [t[L - 1:] for t in reg_t]
        self.cls_ptrs_x3_last, self.reg_ptrs_x3_last = ops.make_ptr_array(self._last_cls), ops.make_ptr_array(self._last_reg)
        q = 'query_generator.'
        self.qg.check_state(sd, self.roi_size, 'HeadEngine')
        if not self.qg.is_default:
            self._qg_tail_dims = False
            self._load_qg_shape(g, w)
        else:
            conv = g(q + 'shared_convs.0.conv.weight').permute(0, 2, 3, 1).reshape(C, 9 * C).contiguous()       # [256,256,3,3] -> [out][tap][cin]
            w['qg_conv_wp'] = k16(conv)                                                   # key16, fragment-major: the fused conv kernel
            w['qg_conv_b'] = g(q + 'shared_convs.0.conv.bias')
            w['qg_fc_b'] = g(q + 'shared_fcs.0.bias')
            e0 = g(q + 'extra_enc.0.weight')                                              # [512,1040] -> K padded to 1056
            e0p = torch.zeros((e0.shape[0], 1056), device=d, dtype=F32)
            e0p[:, :e0.shape[1]] = e0
            w['qg_e0_b'], w['qg_e2_b'] = g(q + 'extra_enc.0.bias'), g(q + 'extra_enc.2.bias')
            w['qg_c_w'], w['qg_c_b'] = g(q + 'fc_center.weight'), g(q + 'fc_center.bias')
            # LDS-tiled bf16x3 linears (mv2d_linear_x3)
            w['qg_fc_wx'], w['qg_e0_wx'], w['qg_e2_wx'] = ops.pack_x3(g(q + 'shared_fcs.0.weight')), ops.pack_x3(e0p), ops.pack_x3(g(q + 'extra_enc.2.weight'))
            # the one-launch tail (mv2d_qg_tail_x3) is built for the shipped dimensions: 256 -> 1024, + 16 intrinsics columns (32 with the pad) -> 512 -> 256,
            # query_embedding 384 -> 256 -> 256; anything else keeps the four launches
            shp = lambda k: tuple(sd[k].shape)
            self._qg_tail_dims = (shp(q + 'shared_fcs.0.weight') == (1024, C) and shp(q + 'extra_enc.0.weight') == (512, 1040)
                                  and shp(q + 'extra_enc.2.weight') == (C, 512) and shp(q + 'fc_center.weight') == (3, C)
                                  and shp('bbox_head.query_embedding.0.weight') == (C, 384) and shp('bbox_head.query_embedding.2.weight') == (C, C))
        pe = 'position_encoding.'
        # (position_encoder.0.weight with its K zero-padded to Kp: the padded frustum rows meet zero columns)
        c1 = lambda k: ops.pad_pe_w1a(g(pe + k)) if k == 'position_encoder.0.weight' else g(pe + k).flatten(1).contiguous()
        pe_names = (('w1a', 'position_encoder.0'), ('w1b', 'position_encoder.2'), ('w2a', 'adapt_pos3d.0'), ('w2b', 'adapt_pos3d.2'),
                    ('wr', 'fpe.conv_reduce'), ('we', 'fpe.conv_expand'))
        # (the submodules the PE's switches leave out have no weights: nothing of theirs is read or packed)
        pe_names = tuple((n_, k_) for n_, k_ in pe_names if (self.with_fpe or n_[1] not in 're') and (not self.no_sin_enc or n_[1] != '2'))
        for n_, k_ in pe_names:
            w['pe_b' + n_[1:]] = g(pe + k_ + '.bias')
        self._pe_w32 = {n_: c1(k_ + '.weight') for n_, k_ in pe_names}               # fp32 originals (3 MB): _c3 builds split copies on demand
        # fragment-major key16 copies for the fused PE kernel (one allocation, in the order the kernel streams them)
        names = ('wr', 'we', 'w1a', 'w1b')
        if self.with_fpe:                  # (the key16 mode's kernel has no gate-less form: route.resolve refuses it)
            packs = [k16(c1(dict(pe_names)[n] + '.weight')).view(-1) for n in names]
            flat, off = torch.cat(packs), 0
            w['pe_pack'] = dict(b1a=w['pe_b1a'], b1b=w['pe_b1b'], br=w['pe_br'], be=w['pe_be'], flat=flat)
            for n, t in zip(names, packs):
                w['pe_pack'][n] = flat[off:off + t.numel()]
                off += t.numel()
        # the sine branch's table is built in fp32-class arithmetic (split-precision linears on the unrounded sine rows; once per (weights, geometry))
        for n_, k_ in pe_names:
            if n_ in ('w2a', 'w2b'):
                w['pe_' + n_ + '_x3'] = ops.pack_x3(c1(k_ + '.weight'))
        if self.exact:
            # bf16 hi / lo fragment-major pairs for the split-precision PE kernel (csrc/pe_x3.hip)
            w['pe_x3'] = dict(b1a=w['pe_b1a'], b1b=w['pe_b1b'], **({'br': w['pe_br'], 'be': w['pe_be']} if self.with_fpe else {}),
                              **{n_: ops.pack_x3(c1(k_ + '.weight')) for n_, k_ in pe_names if n_ in ('w1a', 'w1b', 'wr', 'we')})
            # first-layer weights with their rows in the order csrc/pe_x3b.hip chains the two layers in registers with
            if self.with_fpe:
                w['pe_x3']['w1a_p'] = ops.pack_x3_rowperm(c1('position_encoder.0.weight'))
                w['pe_x3']['wr_p'] = ops.pack_x3_rowperm(c1('fpe.conv_reduce.weight'))
            if self.qg.is_default:
                w['qg_conv_wx3'] = ops.pack_key16_x3(conv)
        self.w = w

    def _load_qg_shape(self, g, w):
        """Packed weights and the launch plan of a query generator of other than the shipped shape (self.qg): w['qg_convs'] = [(key16 hi / lo
        fragment-major weight pair, bias)] per shared conv, w['qg_lin'] = the linears up to fc_center in execution order, each a dict(wx, b, N, K,
        src, dst, ldc, clamp) over workspace buffer names.  K is zero-padded to a multiple of 32 (every activation buffer has that many zeroed
        columns), the first fc of an un-pooled trunk gets its columns in the engine's cell-major order."""
        qs, q, s, d = self.qg, 'query_generator.', self.roi_size, self.dev
        p32 = qg_shape.pad32
        w['qg_convs'] = []
        for i in range(qs.convs):
            cw = g(q + f'shared_convs.{i}.conv.weight').permute(0, 2, 3, 1).reshape(C, 9 * C).contiguous()          # [out][tap][cin]
            w['qg_convs'].append((ops.pack_key16_x3(cw), g(q + f'shared_convs.{i}.conv.bias')))

        def padded(W, n_to=None):
            Wp = torch.zeros((n_to or W.shape[0], p32(W.shape[1])), device=d, dtype=F32)
            Wp[:W.shape[0], :W.shape[1]] = W
            return Wp
        lin, src, bufs = [], 'x2' if qs.pooled else 'qg_flat', {}
        for name, n, k, _ in qs.linears(s)[:-1]:
            W = g(q + name + '.weight')
            if name == 'shared_fcs.0' and not qs.pooled:
                W = W[:, qg_shape.flatten_perm(s, d)].contiguous()
            last_fc = name == f'shared_fcs.{qs.fcs - 1}'
            dst = 'enc' if last_fc else 'qg_' + name.replace('.', '_')
            width = p32(qs.enc_in) if last_fc else p32(n)
            bufs[dst] = width
            lin.append(dict(wx=ops.pack_x3(padded(W)), b=g(q + name + '.bias'), N=n, K=p32(k), src=src, dst=dst, ldc=width, clamp=5e3 if last_fc else 0.0))
            src = dst
        w['qg_lin'], w['qg_bufs'], w['qg_last'] = lin, bufs, src
        w['qg_c_w'], w['qg_c_b'] = g(q + 'fc_center.weight'), g(q + 'fc_center.bias')
        if qs.center_in != C:
            # fc_center on the tile linear: 3 output rows padded to one column tile of 16
            w['qg_c_wx'] = ops.pack_x3(padded(w['qg_c_w'], 16))
            w['qg_c_b16'] = torch.zeros(16, device=d, dtype=F32)
            w['qg_c_b16'][:3] = w['qg_c_b']

    @staticmethod
    def check_decoder_shape(sd, num_layers, feedforward_channels):
        """ValueError naming the key unless the state dict holds exactly ``num_layers`` ``bbox_head.transformer.decoder.layers.{i}`` and every
        layer's FFN is ``feedforward_channels`` wide (``ffns.0.layers.0.0.weight`` [F, 256], ``ffns.0.layers.1.weight`` [256, F])."""
        dec = 'bbox_head.transformer.decoder.layers.'
        have = sorted({int(k[len(dec):].split('.')[0]) for k in sd if k.startswith(dec)})
        if have != list(range(num_layers)):
            raise ValueError(f'HeadEngine: num_layers={num_layers}, the state dict holds {len(have)} decoder layers ({dec}{{i}}, i in {have})')
        F = feedforward_channels
        for i in range(num_layers):
            for name, want in (('ffns.0.layers.0.0.weight', (F, C)), ('ffns.0.layers.1.weight', (C, F))):
                k = f'{dec}{i}.{name}'
                if k not in sd or tuple(sd[k].shape) != want:
                    got = tuple(sd[k].shape) if k in sd else 'missing'
                    raise ValueError(f'HeadEngine: feedforward_channels={F} expects {k} to be {want}, the state dict has {got}')

    @staticmethod
    def check_reg_layout(sd, use_reg_layer, group_reg_dims):
        """ValueError unless the regression branches of the state dict have the layout of the switch: a Sequential
        (``reg_branches.{l}.{0,2,4}.*``) without it, a RegLayer (``reg_branches.{l}.reg_branch.{0,3}.*`` and
        ``reg_branches.{l}.task_heads.{g}.{0,2}.*``) of exactly ``group_reg_dims`` with it."""
        rb = 'bbox_head.reg_branches.0.'
        layouts = {False: 'the Sequential layout (reg_branches.{l}.{0,2,4}.*)',
                   True: 'the RegLayer layout (reg_branches.{l}.reg_branch.{0,3}.*, reg_branches.{l}.task_heads.{g}.{0,2}.*)'}
        found = {False: rb + '0.weight' in sd, True: rb + 'reg_branch.0.weight' in sd}
        if not found[bool(use_reg_layer)] or found[not use_reg_layer]:
            held = ' and '.join(layouts[k] for k in (False, True) if found[k]) or 'neither layout'
            raise ValueError(f'HeadEngine: use_reg_layer={bool(use_reg_layer)} expects {layouts[bool(use_reg_layer)]}, the state dict holds {held}; '
                             f'the other switch value expects {layouts[not use_reg_layer]}')
        if use_reg_layer:
            dims, g = [], 0
            while f'{rb}task_heads.{g}.2.weight' in sd:
                dims.append(int(tuple(sd[f'{rb}task_heads.{g}.2.weight'].shape)[0]))
                g += 1
            if tuple(dims) != tuple(group_reg_dims):
                raise ValueError(f'HeadEngine: group_reg_dims={tuple(group_reg_dims)}, the task heads of the state dict are {tuple(dims)} wide')

    @staticmethod
    def branch_depths(sd):
        """(class depth, regression depth) of layer 0's prediction branches as the state dict's keys spell them: hidden class blocks at
        ``cls_branches.0.{3i, 3i+1}`` (Linear, LayerNorm) before the output Linear, Sequential regression blocks at ``reg_branches.0.{2i}`` before the
        output Linear, RegLayer shared blocks at ``reg_branches.0.reg_branch.{3i}``."""
        cb, rb = 'bbox_head.cls_branches.0.', 'bbox_head.reg_branches.0.'
        nc = 0
        while f'{cb}{3 * nc}.weight' in sd and f'{cb}{3 * nc + 1}.weight' in sd:
            nc += 1
        nr = 0
        if f'{rb}reg_branch.0.weight' in sd:
            while f'{rb}reg_branch.{3 * nr}.weight' in sd:
                nr += 1
        else:
            while f'{rb}{2 * nr}.weight' in sd and f'{rb}{2 * nr + 2}.weight' in sd:
                nr += 1
        return nc, nr

    @staticmethod
    def check_branch_depth(sd, num_reg_fcs, use_reg_layer=False):
        """ValueError naming ``num_reg_fcs`` unless the prediction branches of the state dict have exactly that many hidden layers: decided by
        which keys exist AND by the shapes under them (a depth-1 class branch has its [num_classes, 256] output layer under the key where a
        depth-2 branch has a [256, 256] hidden one)."""
        n = ops.check_num_reg_fcs(num_reg_fcs, 'HeadEngine')
        cb, rb = 'bbox_head.cls_branches.0.', 'bbox_head.reg_branches.0.'
        shp = lambda k: tuple(sd[k].shape) if k in sd else None
        want = [(f'{cb}{3 * i}.weight', (C, C)) for i in range(n)] + [(f'{cb}{3 * i + 1}.weight', (C,)) for i in range(n)]
        if use_reg_layer:
            want += [(f'{rb}reg_branch.{3 * i}.weight', (C, C)) for i in range(n)]
            absent = [f'{rb}reg_branch.{3 * n}.weight']
        else:
            want += [(f'{rb}{2 * i}.weight', (C, C)) for i in range(n)] + [(f'{rb}{2 * n}.weight', (10, C))]
            absent = [f'{rb}{2 * n + 2}.weight']
        absent += [f'{cb}{3 * n + 1}.weight', f'{cb}{3 * n + 3}.weight']
        out = shp(f'{cb}{3 * n}.weight')
        ok = (all(shp(k) == s_ for k, s_ in want) and out is not None and len(out) == 2 and out[1] == C and 1 <= out[0] <= 64
              and not any(k in sd for k in absent))
        if not ok:
            nc, nr = HeadEngine.branch_depths(sd)
            kind = 'RegLayer shared' if use_reg_layer else 'Sequential regression'
            raise ValueError(f'HeadEngine: num_reg_fcs={n} expects {n} hidden layer(s) per prediction branch (class blocks at cls_branches.{{l}}.{{3i, 3i+1}} '
                             f'with the output layer at {3 * n}; {kind} blocks at {"reg_branch.{3i}" if use_reg_layer else "{2i} with the output layer at " + str(2 * n)}); '
                             f'the state dict\'s class branches have {nc} and its regression branches {nr} -- build the engine with the num_reg_fcs of the checkpoint')

    @staticmethod
    def check_pe_layout(sd, with_fpe=True, no_sin_enc=False):
        """ValueError naming the switch (``with_fpe`` / ``no_sin_enc``) when the state dict's ``position_encoding.fpe.*`` / ``adapt_pos3d.*`` keys
        disagree with it, in either direction.  Needs neither the library nor a GPU."""
        pe = 'position_encoding.'
        for sub, want, switch, value in (('fpe.', with_fpe, 'with_fpe', with_fpe), ('adapt_pos3d.', not no_sin_enc, 'no_sin_enc', no_sin_enc)):
            have = sorted(k for k in sd if k.startswith(pe + sub))
            if have and not want:
                raise ValueError(f'HeadEngine: the state dict holds {pe}{sub}* ({have[0]}, ...) but {switch}={value} builds no such submodule')
            if want and not have:
                raise ValueError(f'HeadEngine: the state dict has no {pe}{sub}* keys but {switch}={value} needs them')

    def _c3(self, name):
        """K-concatenated split-precision copy [w_hi | w_hi | w_lo] of a PE weight ('w1a', 'w1b', 'w2a', 'w2b', 'wr', 'we'), built on first use
        on the default route (which only keeps the sine branch's pair; the index-exact route holds all six)."""
        k = 'pe_' + name + '_c3'
        if k not in self.w:
            self.w[k] = ops.cat3_weight(self._pe_w32[name])
        return self.w[k]

    # ------------------------------------------------------------------------------------------ workspace
    def _workspace(self, V, h, w, R, Vg, map_dtype, st):
        """Buffers of one (map shape, R) problem.  The number of RoIs changes from frame to frame in real use, so the STORAGE is
        allocated once per (map shape, R rounded up to a multiple of 32, at least 64) and every exact R only gets a dict of dense views into it
        (kernels index [*, R, *] tensors densely) plus its own hipGraph; staging buffers, calibration cache and the stream-order
        guard are shared by all R of a bucket.  Vg = views per sample, V = all views of the batch; st = the route's storage part (route.Storage):
        routes that store their rows differently never share buffers."""
        # (the dtype of the feature map is part of both keys: ws['featcl'] has it, and a captured graph holds the launches of ONE element format)
        key = (V, h, w, R, Vg, self.num_classes, self.roi_size, map_dtype, st, self.num_reg_fcs)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        cap = max(64, -(-R // 32) * 32)
        bkey = (V, h, w, cap, Vg, self.num_classes, self.roi_size, map_dtype, st, self.num_reg_fcs)
        base = self._ws_base.get(bkey)
        if base is None:
            store = []

            def alloc(shape, dt=F32, zero=False, pinned=False):
                shape = (shape,) if isinstance(shape, int) else tuple(shape)
                t = (torch.zeros if zero else torch.empty)(shape, dtype=dt, device='cpu' if pinned else self.dev)
                if pinned:
                    t = t.pin_memory()
                store.append(t)
                return t
            self._build_ws(V, h, w, cap, alloc, Vg, map_dtype, st)
            base = self._ws_base[bkey] = dict(store=store, shared={})
        it = iter(base['store'])

        def view(shape, dt=F32, zero=False, pinned=False):
            shape = (shape,) if isinstance(shape, int) else tuple(shape)
            n = 1
            for v_ in shape:
                n *= v_
            t = next(it)
            assert t.dtype == dt and t.numel() >= n
            return t.view(-1)[:n].view(shape)
        ws = self._build_ws(V, h, w, R, view, Vg, map_dtype, st)
        ws['shared'] = base['shared']
        self._ws[key] = ws
        return ws

    def _build_ws(self, V, h, w, R, alloc, Vg, map_dtype, st):
        d, L = self.dev, self.L
        P = V * h * w
        B = V // Vg                                      # samples sharing every launch
        e = lambda shape, dt=F32: alloc(shape, dt)
        z = lambda shape, dt=F32: alloc(shape, dt, zero=True)
        ws = dict(P=P, B=B, Vg=Vg, map_dtype=map_dtype)
        # calibration blob layout (fp64 tables first, then fp32, then bytes)
        lay, off = {}, 0
        for name, n, dt in [('viewK', V * 16, torch.float64), ('viewE', V * 16, torch.float64), ('img2lidar', V * 16, torch.float64),
                            ('trans', V * Vg * 16, torch.float64), ('coords_w', w, torch.float64), ('coords_h', h, torch.float64),
                            ('coords_d', self.depth_num, torch.float64), ('embeds', 3 * P, F32), ('pad_mask', P, torch.uint8)]:
            sz = n * torch.empty(0, dtype=dt).element_size()
            lay[name] = (off, n, dt)
            off += (sz + 15) // 16 * 16
        ws['blob_layout'], ws['blob_bytes'] = lay, off
        ws['blob_h'] = alloc(off, torch.uint8, pinned=True)
        ws['blob_d'] = e(off, torch.uint8)
        ws['tab'] = {k: ws['blob_d'][o:o + n * torch.empty(0, dtype=dt).element_size()].view(dt) for k, (o, n, dt) in lay.items()}
        # per-frame dynamic inputs: RoI list, per-view offsets, first query row of every sample, per-row time step (T path);
        # one pinned staging buffer -> one H2D copy
        o1, o2, o3 = R * 5, R * 5 + (V + 1), R * 5 + (V + 1) + (B + 1)
        dyn_words = o3 + R
        ws['dyn_h'] = alloc(dyn_words, torch.int32, pinned=True)
        ws['dyn_d'] = e(dyn_words, torch.int32)
        for sfx, buf in (('_h', ws['dyn_h']), ('', ws['dyn_d'])):
            ws['rois' + sfx] = buf[:o1].view(F32).view(R, 5)
            ws['view_start' + sfx] = buf[o1:o2]
            ws['grp_start' + sfx] = buf[o2:o3]
            ws['dt_rows' + sfx] = buf[o3:].view(F32)
        K16 = self.K16
        NC = self.cells                                  # RoI cells (s x s)
        ws['featcl'] = e((P, C), map_dtype)               # position-major feature map in the INPUT's dtype (fp32 / fp16 / bf16): its readers widen in registers
        qs = self.qg
        ws['enc'] = z((R, 1056 if qs.is_default else qg_shape.pad32(qs.enc_in))); ws['minv'] = e((R, 16))
        ws['roi_feat'] = e((R, NC, C), K16)
        if qs.is_default:
            ws['enc1'] = e((R, 512)); ws['enc2'] = e((R, C)); ws['center'] = e((R, 3))
            ws['intr'], ws['ld_intr'] = ws['enc'][:, 1024:], 1056
        else:
            # buffers of the shape's launch plan (_load_qg_shape): zeroed, so that the pad columns behind a width that is no multiple of 32 stay 0
            for name, width in self.w['qg_bufs'].items():
                if name != 'enc':
                    ws[name] = z((R, width))
            for i in range(min(max(qs.convs - 1, 0), 2)):                  # cells between two convs: key16 hi + lo, ping-pong
                ws[f'qg_cells_hi{i}'] = e((R, NC, C), K16); ws[f'qg_cells_lo{i}'] = e((R, NC, C), K16)
            if not qs.pooled:
                ws['qg_flat'] = e((R, NC * C))                              # the cell-major flattening the first fc reads
            if qs.center_in != C:
                ws['qg_center16'] = e((R, 16))
                ws['center'] = ws['qg_center16'][:, :3]
            else:
                ws['center'] = e((R, 3))
            if qs.intrinsic:
                ws['intr'], ws['ld_intr'] = ws['enc'][:, qs.fc_out:], ws['enc'].shape[1]
            else:
                ws['intr'], ws['ld_intr'] = e((R, 16)), 16                  # the per-RoI camera kernel writes them; nothing reads them
        ws['xyz'] = e((R, 3)); ws['ref'] = e((R, 3)); ws['posemb'] = e((R, 384)); ws['qe1'] = e((R, C)); ws['qpos'] = e((R, C))
        ws['match'] = e((R, Vg, self.topk), torch.int32)
        Pp = (P + 15) // 16 * 16
        ws['zbuf'] = z(Pp + 32, torch.uint8)                     # roi_mask | nnz[2] | qt_ctl[2] | grp_ctl[2] | lo8_flag: cleared by ONE fill per frame
        ws['roi_mask'] = ws['zbuf'][:P]
        ws['nnz'] = ws['zbuf'][Pp:Pp + 8].view(torch.int32)
        ws['qt_ctl'] = ws['zbuf'][Pp + 8:Pp + 16].view(torch.int32)      # query-order flags (zeroed with zbuf)
        ws['grp_ctl'] = ws['zbuf'][Pp + 16:Pp + 24].view(torch.int32)    # shared-tile cross attention: union entries allocated | capacity flag
        ws['lo8_flag'] = ws['zbuf'][Pp + 24:Pp + 28].view(torch.int32)   # e4m3 lo rows: a remainder left the format's range in this frame (csrc/common.h lo8_pack4_flag)
        ws['ctl'] = ws['zbuf'][Pp:Pp + 32].view(torch.int32)             # the eight words above as one array (_check_capacity: one copy to the host)
        ws['zero_mask'] = z(P, torch.uint8)
        ws['rect'] = e((R, 5), torch.int32); ws['pos2s'] = e(P, torch.int32); ws['s2pos'] = e(P, torch.int32)
        ws['S_dev'] = z(1, torch.int32)
        ws['row_ptr'] = e(R + 1, torch.int32)
        if st.kind == 'T':
            ws['bits'] = e(max(ops.csr_workspace_bytes(R, Vg, h, w) // 4, 1), torch.int32)
            ws['row_count'] = e(R, torch.int32)
            ws['col_cap'] = R * self.col_cap_per_query
            ws['S_kv'] = P
        else:
            ws['col_cap'] = R * (1 + Vg * self.topk) * NC
            ws['S_kv'] = R * NC
            ws['roi_sum'] = e((R, NC, C), K16)
        ws['q_order'] = alloc(R, torch.int32, zero=True) if st.q_order else None
        ws['col_idx'] = e(ws['col_cap'], torch.int32)
        # group tables of the shared-tile cross attention (csrc/xattn_group.hip): g_slot | g_cnt | g_ptr | g_len per group, the groups' union key lists
        ws['grp_tab'] = None
        if st.group_tab:
            ng = ops.xattn_group_max(R, B)
            ucap = ws['col_cap'] + 16 * ng
            ws['grp_tab'] = dict(ng=ng, g=alloc((4, ng), torch.int32, zero=True), ucol=alloc(ucap, torch.int32, zero=True),
                                 umask=alloc(ucap, torch.uint8, zero=True), ucap=ucap, ctl=ws['grp_ctl'])
        # key16 rows of the PE block's inputs: frustum [.,192], sine [.,384] (training route only: the inference kernel reads the folded
        # table), feature rows [.,256] (the SE gate's input; the value rows of the T path)
        ws['A1'] = e((P, self.pe_kp), K16); ws['A2'] = None if self.no_sin_enc else e((P, 384), K16)      # (no sine branch: no sine rows)
        ws['Xf_b'] = e((P, C), K16)
        if st.exact:
            # index-exact route: the unrounded fp32 frustum rows of the PE block (the feature rows are read from the map), the lo halves of the
            # key / value rows and RoI cells -- all pre-allocated (no per-frame allocation, no host synchronisation: the route is
            # graph-replayable like the default one)
            ws['xa1'] = e((P, self.pe_kp)); ws['xa2'] = None if self.no_sin_enc else e((P, 384))
            lo8, LO = st.lo8, torch.uint8 if st.lo8 else K16
            if st.kind == 'T':
                ws['xk_lo'] = z((P, C), LO); ws['xv_lo'] = z((P, C), LO)
                ws['roi_lo'] = e((R, NC, C), K16)                 # lo halves of the RoI cells (conv input)
            else:
                ws['xk_lo'] = z((R * NC, C), LO); ws['xv_lo'] = z((R * NC, C), LO)
                # S path: the value rows ARE the RoI cells (key16 lo rows: one array for both; lo8 rows: the split-precision conv, when it runs, reads its own key16 lo cells)
                ws['roi_lo'] = e((R, NC, C), K16) if lo8 else ws['xv_lo'].view(R, NC, C)
            # (the launches take the lo rows' format from the route, the kernels' binding from the buffers: they have to agree)
            assert ws['xk_lo'].dtype == ws['xv_lo'].dtype == LO
        ws['pe'] = e((P, C)); ws['Xk'] = e((P, C), K16)
        ws['pe_pos'] = z((P, C)) if st.pe_pos else None      # never-listed rows stay 0 (they only ever meet weight 0)
        # cross attention in the raw key space: per-query operand Qt (key16 hi | lo rows of the 8 per-head maps), per-head context sums z
        ws['Qt'] = e((R, 16 * C), K16); ws['zh'] = e((R, 8 * C))
        # unprojected key / value input rows of the cross attention (key + key_pos, key): shared by all layers
        if st.kind == 'T':
            ws['xk_rows'], ws['xv_rows'] = ws['Xk'], ws['Xf_b']
        else:
            ws['xk_rows'], ws['xv_rows'] = ws['roi_sum'].view(R * NC, C), ws['roi_feat'].view(R * NC, C)
        for n in ('x', 'x1', 'x2', 'ctx', 'q'):
            ws[n] = e((R, C))
        ws['zero_rows'] = z((R, C))                              # never written
        ws['sa0_ctx'] = e((R, C))                                # rows of the layer-0 self-attention value bias (fold_sa0), filled per weights version
        ws['qkv'] = e((R, 3 * C)); ws['parts'] = e((self.ffn_slabs, R, C)); ws['outs'] = e((L, R, C))
        ws['cls'] = e((L, R, self.num_classes)); ws['reg'] = e((L, R, 10))
        ws['boxes'] = z((B, self.max_num, 9)); ws['scores'] = z((B, self.max_num))
        ws['labels'] = z((B, self.max_num), torch.int64); ws['bbox_index'] = z((B, self.max_num), torch.int64); ws['count'] = z(B, torch.int32)
        return ws

    # ------------------------------------------------------------------------------------------ forward
    def _shape_tables(self, img_metas, h, w):
        """Tables of the padding geometry (frustum grid, padding mask, sine embeds: tens of ms to build), pure functions of the shapes
        they are cached by."""
        skey = (calib.meta_shapes(img_metas), h, w)
        sht = self._shape_cache.get(skey)
        if sht is None:
            sht = calib.shape_tables(skey[0], h, w, stride=self.stride, depth_num=self.depth_num, depth_start=self.depth_start,
                                     position_range=tuple(self.pe_range_h64.tolist()), lid=self.LID)
            if len(self._shape_cache) >= 16:
                self._shape_cache.pop(next(iter(self._shape_cache)))
            self._shape_cache[skey] = sht
        return skey, sht

    def _host_prepare(self, proposals_list, metas_list, V, h, w, rt):
        """Host side of one batch of samples: RoI lists + calibration tables into the workspace's pinned staging buffers.
        The camera matrices are compared with the previous frame's and, when they differ (every frame on the two-frame path: ego motion),
        the derived tables are rebuilt with batched calls and uploaded; the tables of the padding geometry only when the shapes change."""
        B = len(proposals_list)
        Vg = V // B
        # bbox2roi (mmdet) + the dummy proposal rule (RH/mv2d_head.py:105-108), in numpy straight into the staging buffer
        arrs, counts, grp = [], [], [0]
        for b, (props, metas) in enumerate(zip(proposals_list, metas_list)):
            assert len(props) == Vg and len(metas) == Vg, 'every sample of a batch needs the same number of views'
            pa = [(p.detach().to('cpu', F32).numpy() if torch.is_tensor(p) else np.asarray(p, dtype=np.float32)).reshape(-1, 6 if len(p) == 0 else np.shape(p)[-1])
                  for p in props]
            if sum(a.shape[0] for a in pa) == 0:
                pa[0] = np.array([[0, 50, 50, 100, 100, 0]], dtype=np.float32)
            arrs += pa
            counts += [a.shape[0] for a in pa]
            grp.append(grp[-1] + sum(a.shape[0] for a in pa))
        R = grp[-1]
        # The number of RoIs changes with every real frame.  All launches run on the BUCKET size (R rounded up to a multiple of 32, at least 64): the
        # rows R..cap-1 are copies of the last RoI that belong to no sample (not in view_start / grp_start), so nothing attends to them,
        # nothing decodes them and the key set is unchanged; every R of a bucket shares one workspace and ONE captured graph.
        cap = max(64, -(-R // 32) * 32)
        ws = self._workspace(V, h, w, cap, Vg, rt.map_dtype, rt.storage)
        sh = ws['shared']
        if 'done_ev' in sh:
            sh['done_ev'].synchronize()      # the previous frame on this workspace must have consumed the pinned staging buffers (its uploads have run)
        rois_np = ws['rois_h'].numpy()
        rois_np[:R, 0] = np.repeat(np.arange(V, dtype=np.float32), counts)
        rois_np[:R, 1:] = np.concatenate([a[:, :4] for a in arrs if a.shape[0]], 0)
        rois_np[R:] = rois_np[R - 1]
        bh, lay = ws['blob_h'], ws['blob_layout']

        bh_np = bh.numpy()

        def put(k, src):
            # numpy, not Tensor.copy_: above 32768 elements torch spreads a CPU copy over all host threads, and waking 128-256 of them costs
            # milliseconds (measured: 16 two-frame samples per launch -> 3.8 ms per copy, 435 instead of 4500 samples/s on one stream)
            o_, n, dt_ = lay[k]
            nb = n * torch.empty(0, dtype=dt_).element_size()
            a = src.detach().cpu().numpy() if torch.is_tensor(src) else np.asarray(src)
            a = np.ascontiguousarray(a, dtype={torch.float64: np.float64, torch.float32: np.float32, torch.uint8: np.uint8}[dt_])
            bh_np[o_:o_ + nb] = a.reshape(-1).view(np.uint8)
        split = lay['coords_w'][0]                     # [0, split): camera matrices (per frame); [split, end): padding geometry (per rig)
        shp = [self._shape_tables(m, h, w) for m in metas_list]
        shape_key = tuple(k for k, _ in shp)
        fts = [t for _, t in shp]
        f0 = fts[0]
        if sh.get('shape_key') != shape_key:
            assert all(t['pad_h'] == f0['pad_h'] and t['pad_w'] == f0['pad_w'] for t in fts), 'samples of a batch share one pad_shape'
            for k in ('coords_w', 'coords_h', 'coords_d'):
                put(k, f0[k])
            put('embeds', torch.cat([t['embeds'] for t in fts], 1) if B > 1 else f0['embeds'])        # [3, P]: the samples side by side
            put('pad_mask', torch.cat([t['pad_mask'] for t in fts]) if B > 1 else f0['pad_mask'])
            ws['blob_d'][split:].copy_(bh[split:], non_blocking=True)
            sh['shape_key'] = shape_key
        flat = [m for metas in metas_list for m in metas]
        mats = np.stack([np.stack([np.asarray(m[k]) for m in flat]) for k in ('intrinsics', 'extrinsics', 'lidar2img')]).astype(np.float64, copy=False)
        ts = np.array([m.get('timestamp', 0.0) for m in flat], dtype=np.float64).reshape(B, Vg)
        prev = sh.get('mats')
        if prev is None or prev.shape != mats.shape or not np.array_equal(prev, mats):
            # the camera matrices changed: inverse / view-to-view tables rebuilt on the host (batched, ~0.5 ms for 8 x 12 views) and uploaded
            # here, stream-ordered before the frame (23 KB per 12-view sample)
            _, img2lidar, trans, _ = calib.geometry_tables_batch(metas_list)
            put('viewK', torch.from_numpy(mats[0])); put('viewE', torch.from_numpy(mats[1]))
            put('img2lidar', img2lidar); put('trans', trans)
            ws['blob_d'][:split].copy_(bh[:split], non_blocking=True)
            sh['mats'] = mats
            sh['mats_gen'], sh['mats_one_rig'] = sh.get('mats_gen', 0) + 1, None       # (pe_cache below: the matrices moved)
        nv = self.num_views
        dts = [float(ts[b, nv:].mean() - ts[b, :nv].mean()) if (self.kind == 'T' and Vg > nv) else 0.0 for b in range(B)]
        sh['frame_scalars'] = dict(pad_h=f0['pad_h'], pad_w=f0['pad_w'], dt=dts[0])
        # the sine branch adapt_pos3d(sine) depends on the padding geometry of the samples only (not on calibration): its table is rebuilt when
        # that (or the weights) change -- in fp32-class arithmetic on both routes (fp32 sine rows, K-concatenated split-precision GEMMs:
        # a once-per-rig cost), so that the table adds no 16-bit rounding of its own to pe
        skey = (self._weights_version,) + tuple(k[0] for k in shape_key)
        if self.no_sin_enc:
            # no sine branch (MU/pe.py:163-166 skipped): the PE kernel's table is ONE all-zero row of period 1, built once -- no sine rows, no weights
            if sh.get('sine_tab') is None:
                sh['sine_tab'] = torch.zeros((1, C), device=self.dev, dtype=F32)
                sh['sine_gen'], sh['sine_period'] = sh.get('sine_gen', 0) + 1, 1
        elif sh.get('sine_key') != skey:
            same = all(k == skey[1] for k in skey[1:])
            P = V * h * w
            Pt = P // B if same else P                                  # one sample's positions when all samples share the geometry
            T, o, W_ = ws['tab'], ops, self.w
            s2 = torch.arange(Pt, dtype=torch.int32, device=self.dev)
            k16e = lambda n_: torch.empty((Pt, n_), device=self.dev, dtype=self.K16)
            a2f = torch.empty((Pt, 384), device=self.dev, dtype=F32)
            a1f = torch.empty((Pt, self.pe_kp), device=self.dev, dtype=F32)
            o.pe_inputs(s2, torch.tensor([Pt], dtype=torch.int32, device=self.dev), Pt, ws['featcl'], T['img2lidar'], T['coords_w'], T['coords_h'],
                        T['coords_d'], T['embeds'], self.const['dim_t'], k16e(self.pe_kp), k16e(384), k16e(C), None, V, h, w, self.depth_num,
                        self.pe_range_h64, A_frustum_f32=a1f, A_sine_f32=a2f, ld=self.pe_kp)
            w2a, w2b = self._pe_w32['w2a'], self._pe_w32['w2b']
            h2 = o.linear_x3(a2f, W_['pe_w2a_x3'], W_['pe_b2a'], N=w2a.shape[0], K=w2a.shape[1], act=1)
            tab = o.linear_x3(h2, W_['pe_w2b_x3'], W_['pe_b2b'], N=w2b.shape[0], K=w2b.shape[1])
            del a1f, a2f, h2
            # kept with the tables the workspaces of this map shape share; a captured graph holds the pointer: same shape -> refreshed in place
            if sh.get('sine_tab') is None or sh['sine_tab'].shape != tab.shape:
                sh['sine_tab'] = tab
                sh['sine_gen'] = sh.get('sine_gen', 0) + 1
            else:
                sh['sine_tab'].copy_(tab)
            sh['sine_period'] = Pt
            sh['sine_key'] = skey
        if ws.get('sine_gen') != sh['sine_gen']:
            ws['sine_gen'] = sh['sine_gen']
            ws['graph_stale'] = True                                     # this workspace's graphs were captured with another table
        # the frustum MLP of the PE depends on the weights, the padding geometry and the camera matrices: on a rig whose matrices repeat it is kept
        # as a table Q per position of one sample and a frame runs only the gate (route option pe_cache, mv2d_amd/pe_cache.py, csrc/pe_x3_gate.hip)
        ws['pe_hit'], ws['pe_cache_state'] = False, 'off'
        if rt.pe_cache:
            pol = sh.get('pe_q_policy')
            if pol is None:
                pol = sh['pe_q_policy'] = pe_cache.PeCachePolicy()
            Pt = (V * h * w) // B
            usable = sh['sine_period'] == Pt                             # (Q and the sine table share the kernel's one period)
            if usable and pol.prev is not None and pol.prev[2] == sh['mats_gen'] and sh['mats_one_rig'] is None:
                sh['mats_one_rig'] = pe_cache.one_rig(mats, B)           # the matrices repeat: do the samples share them?  (asked once per set of matrices)
            state = pol.observe(pe_cache.rig_key(self._weights_version, shape_key, sh['mats_gen'], sh['mats_one_rig'] is not False) if usable else None)
            if state == 'build':
                self._build_pe_q(ws, sh, Pt, V, h, w)
            ws['pe_hit'], ws['pe_cache_state'] = state != 'miss', state
            if ws.get('pe_q_gen') != sh.get('pe_q_gen'):
                ws['pe_q_gen'] = sh.get('pe_q_gen')
                ws['graph_stale'] = True                                 # (a re-allocated table: captured graphs hold the old pointer)
        # the two-frame head keeps that table PER VIEW (route option pe_cache_views): the views whose matrices repeat (the current frame of a fixed
        # calibration) read their slice of Q, the others (ego motion) run the full kernel; the mask of cached views is DATA, uploaded here
        ws['pe_views'] = ()
        if rt.pe_cache_views:
            Pt = (V * h * w) // B
            usable = sh['sine_period'] == Pt and Vg <= 32                # (Q and the sine table share the kernel's one period; one mask word)
            pol = sh.get('pe_qv_policy')
            if pol is None and Vg <= 32:
                pol = sh['pe_qv_policy'] = pe_cache.PeViewCachePolicy(Vg)
            mask, build, state = 0, (), 'miss'
            if pol is not None:                                          # (an unusable frame drops every slice)
                mask, build, state = pol.observe(pe_cache.view_keys(self._weights_version, shape_key, mats, B) if usable else [None] * Vg)
            if build:
                self._build_pe_q_views(ws, sh, Pt, V, h, w, build)
            ws['pe_hit'], ws['pe_cache_state'], ws['pe_views'] = mask != 0, state, pe_cache.mask_views(mask)
            if ws.get('pe_q_gen') != sh.get('pe_q_gen'):
                ws['pe_q_gen'] = sh.get('pe_q_gen')
                ws['graph_stale'] = True                                 # (a re-allocated table: captured graphs hold the old pointer)
            if sh.get('pe_vmask') is None:
                sh['pe_vmask_h'] = torch.zeros(1, dtype=torch.int32).pin_memory()
                sh['pe_vmask'] = torch.zeros(1, dtype=torch.int32, device=self.dev)
            sh['pe_vmask_h'].numpy().view(np.uint32)[0] = mask
            sh['pe_vmask'].copy_(sh['pe_vmask_h'], non_blocking=True)    # stream-ordered in front of the frame, outside any captured graph
        ws['view_start_h'].numpy()[:] = np.concatenate([[0], np.cumsum(counts)])
        ws['grp_start_h'].numpy()[:] = grp
        if self.kind == 'T':
            # the frame time step is DATA (per row), not a scalar baked into a captured graph: real time stamps differ from frame to frame
            dtr = ws['dt_rows_h'].numpy()
            dtr[:R] = np.repeat(np.asarray(dts, dtype=np.float32), np.diff(grp))
            dtr[R:] = dts[-1]
        sc = dict(sh['frame_scalars'])
        assert max(counts) <= 1024, 'at most 1024 RoIs per view (mv2d_box_correlation)'
        sc['max_per_view'] = max(counts)
        # top-k decode: the kernel sizes its candidate buffer by a power of two >= rows * classes; the launch gets the largest row count
        # of that size class, so that frames with different RoI counts share the launch configuration (and the graph).  Above 16384
        # candidates per sample the decode streams its keys from cls (mv2d_decode_topk), up to 65536 = 1024 queries x 64 classes
        n_max = max(grp[b + 1] - grp[b] for b in range(B)) * self.num_classes
        if n_max > 65536:
            raise ValueError(f'mv2d engine: {n_max} decode candidates in one sample (queries x num_classes), at most 65536')
        n_pow2 = 1024
        while n_pow2 < n_max:
            n_pow2 <<= 1
        sc['max_rows'] = min(n_pow2 // self.num_classes, cap)
        sc['cap'] = cap
        return ws, R, sc

    def _tick(self, name):
        if self.prof is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.prof.setdefault(name, []).append(ev)

    def _enqueue(self, ws, feat, R, V, h, w, sc):
        """Device side of one frame: everything below is enqueued on the current stream, no host sync."""
        o, W_, rt = ops, self.w, ws['route']
        P, L, T = ws['P'], self.L, ws['tab']
        B, Vg = ws['B'], ws['Vg']
        grp = ws['grp_start']                             # first query row of every sample (device): sample-local self attention / top-k; the rows behind the last sample are bucket padding
        tk = self._tick
        tk('h2d')
        rois = ws['rois']                                 # (the RoI list / row tables were uploaded by _run, outside any captured graph)
        # position-major feature map.  Round 5: only the rows somebody reads are transposed (roi_mask: the RoIAlign taps, the key positions and the
        # rows the PE block gates all lie inside some RoI's rectangle), so the transposition runs BEHIND the kernels that build the position list;
        # the whole map is transposed for the training route, for keep_stages runs and when the query-generator chain is forked (key16 mode, T path)
        forked = rt.forked
        # (T path: roi_mask = the correlation rectangles, which contain every RoIAlign tap only when expand_stride >= 1 -- with the default 0 of
        #  BoxCorrelation a bilinear tap can lie one cell outside its RoI's rectangle; the S path marks the exact tap range.  ADVICE r5)
        masked = (rt.masked and (rt.kind == 'S' or self.expand >= 1.0) and (h * w) % 4 == 0 and not (torch.is_tensor(feat) and feat.is_contiguous(memory_format=torch.channels_last) and not feat.is_contiguous()))

        def transpose(mask):
            if isinstance(feat, (list, tuple)):
                fcl, Pg = ws['featcl'], P // B
                for b_, f in enumerate(feat):
                    o.nchw_to_nhwc(f, fcl[b_ * Pg:(b_ + 1) * Pg], mask=None if mask is None else mask[b_ * Pg:(b_ + 1) * Pg])
                return fcl
            if feat.is_contiguous(memory_format=torch.channels_last) and not feat.is_contiguous():
                return feat.permute(0, 2, 3, 1).reshape(P, C)                          # already position-major: no copy
            return o.nchw_to_nhwc(feat, ws['featcl'], mask=mask)
        tk('transpose')
        featcl = ws['featcl'] if masked else transpose(None)
        ws['featcl_cur'], ws['map_shape'], ws['max_rows'] = featcl, (V, h, w), sc['max_rows']
        ws['feat_in'], ws['featcl_masked'] = feat, masked            # (train_forward: the masked transposition leaves rows outside every RoI rectangle unwritten)
        tk('box_params'); tk('box_corr')
        # a3/a5/a7 per-RoI camera + a9 epipolar correlation (both independent of the features) + the clearing of the frame's mask / flag
        # bytes: one launch (round 4; a one-sample frame is bound by its NUMBER of kernels)
        o.frame_geometry(rois, T['viewK'], T['viewE'], ws['intr'], ws['ld_intr'], ws['minv'], ws['view_start'], T['trans'], self.const['lin'],
                         self.const['depths'], ws['match'], Vg, self.topk, sc['pad_h'], sc['pad_w'], sc['max_per_view'], iou_thr=self.iou_thr,
                         ratio=self.ratio, zero=ws['zbuf'], roi_size=float(self.roi_size), intr_scale=self.intrins_feat_scale,
                         sample_size=self.sample_size, num_depth=self.num_depth, depth_start=self.corr_depth_start)
        tk('csr')
        # T path: the query-generator chain (RoIAlign -> conv -> fcs -> ref points -> query_pos) only needs the feature map and
        # the per-RoI cameras, the key chain (correlation -> key list -> PE -> K/V) only the boxes: run them on two streams
        if forked:
            side = ws.get('side_stream')
            if side is None:
                side = ws['side_stream'] = torch.cuda.Stream(device=self.dev)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                o.roi_align(featcl, rois, h, w, out0=ws['roi_feat'], R=R, roi_size=self.roi_size)
                self._enqueue_qg(ws, R)
        order = ws['q_order']                             # (None unless the route orders the attention blocks)
        if rt.kind == 'T':
            # a11/a12: key list + CSR
            o.mask_compact(rois, ws['match'], T['pad_mask'], ws['roi_mask'], ws['rect'], ws['pos2s'], ws['s2pos'], ws['S_dev'],
                           ws['bits'], ws['row_count'], ws['row_ptr'], ws['col_idx'], ws['nnz'], R, Vg, h, w, self.topk,
                           self.stride, self.expand, col_cap=ws['col_cap'], n_samples=B)
            if rt.q_order:
                o.xattn_query_order(ws['row_ptr'], ws['col_idx'], grp, R, order, ws['qt_ctl'][1:])
        else:
            if rt.force_nc is not None:
                # the synthetic rig barely correlates RoIs across views, so the S-path sweep over n_c
                # (RoIs per query) substitutes a synthetic correlation list: own RoI + (n_c - 1) others
                fm = ws.get('forced_match')
                if fm is None or fm.shape != ws['match'].shape:
                    assert rt.force_nc - 1 <= Vg * self.topk, 'raise corr_topk for this n_c'
                    fmh = torch.full((R, Vg * self.topk), -1, dtype=torch.int32)
                    ar = torch.arange(R, dtype=torch.int32)
                    for j in range(1, rt.force_nc):
                        fmh[:, j - 1] = (ar + 37 * j) % R
                    fm = ws['forced_match'] = fmh.view(R, Vg, self.topk).to(self.dev)
                ws['match'].copy_(fm)
            # positions the RoIAlign taps touch (exact ranges, expand_stride < 0: csrc/geometry.hip roi_tap_range) -> PE only there; CSR over the correlated RoIs' feature rows; launch order of
            # the attention blocks (queries ranked by the smallest RoI they list)
            o.roi_positions_csr(rois, ws['zero_mask'], ws['roi_mask'], ws['rect'], ws['pos2s'], ws['s2pos'], ws['S_dev'], R, V, h, w, ws['match'],
                                ws['row_ptr'], ws['col_idx'], ws['nnz'], Vg, self.topk, stride=self.stride, expand_stride=-1.0, grp_start=grp,
                                order=order, order_flags=ws['qt_ctl'][1:] if rt.q_order else None, roi_size=self.roi_size)
        if rt.grouped:
            o.xattn_group_tables(ws['row_ptr'], ws['col_idx'], grp, R, ws['grp_tab'], order=order)
        if masked:
            transpose(ws['roi_mask'])
        if rt.kind == 'T' and not forked:
            tk('roi_align')                               # a4: RoIAlign of the feature half only
            o.roi_align(featcl, rois, h, w, out0=ws['roi_feat'], out0_lo=ws['roi_lo'] if rt.conv_x3 else None, R=R, roi_size=self.roi_size)
        md = ws['S_dev']
        # a2: PE at the listed positions only
        if rt.pe_x3:
            tk('pe_inputs'); tk('pe_fused')
            self._exact_pe(ws, featcl, P, V, h, w)
        else:
            tk('pe_inputs')
            o.pe_inputs(ws['s2pos'], md, P, featcl, T['img2lidar'], T['coords_w'], T['coords_h'], T['coords_d'], T['embeds'],
                        self.const['dim_t'], ws['A1'], ws['A2'] if rt.keep_sine_rows else None, ws['Xf_b'], None,
                        V, h, w, self.depth_num, self.pe_range_h64, ld=self.pe_kp)
            tk('pe_fused')
            # only what the path reads is written: S: pe (RoIAlign reads it; its keys are RoI-aligned rows), T: Xk (nothing reads pe);
            # a keep_stages run writes both
            dbg = rt.stages or rt.exact
            o.pe_fused_tab(ws['A1'], ws['Xf_b'], featcl, md, W_['pe_pack'], ws['shared']['sine_tab'], ws['shared']['sine_period'],
                           ws['pe'] if (rt.kind == 'S' or dbg) else None, ws['Xk'] if (rt.kind == 'T' or dbg) else None, M=P,
                           row_index=ws['s2pos'])
        if rt.kind == 'S':
            tk('roi_align')
            # key rows = RoIAlign(feat) + RoIAlign(pe), value rows = RoIAlign(feat) (index-exact route: both as key16 hi + lo pairs)
            pe_map, pe_idx = (ws['pe_pos'], None) if rt.pe_at_pos else (ws['pe'], ws['pos2s'])
            if rt.lo8:
                lo = dict(out0_lo=ws['roi_lo'] if rt.conv_x3 else None, out0_lo8=ws['xv_lo'], out1_lo8=ws['xk_lo'], lo8_flag=ws['lo8_flag'])
            else:
                lo = dict(out0_lo=ws['xv_lo'], out1_lo=ws['xk_lo']) if rt.exact else {}
            o.roi_align(featcl, rois, h, w, map1=pe_map, out0=ws['roi_feat'], out1=ws['roi_sum'], map1_index=pe_idx, out1_is_sum=True, R=R,
                        roi_size=self.roi_size, **lo)
        if rt.ablate_zero_lo:                                # (key16 lo rows: route.resolve refuses it on lo8 rows)
            zero = rt.ablate_zero_lo
            for c_ in 'vk':
                if c_ in zero:
                    ws[f'x{c_}_lo'].zero_()
            if '8' in zero:                   # the lo halves rounded to 8-bit floats: what 256-byte lo rows would carry.  '8f': OCP e4m3 under the
                for t in (ws['xk_lo'], ws['xv_lo']):         # FIXED scale 2^12 (|lo| <= 2^-12 |x|: the format a kernel can write without a reduction); '8z': e4m3fnuz, '8': e5m2fnuz, per-tensor scale
                    if '8f' in zero:
                        t.copy_(((t.float() * 4096.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float() / 4096.0).to(t.dtype))
                        continue
                    f8 = torch.float8_e4m3fnuz if '8z' in zero else torch.float8_e5m2fnuz
                    m = t.float().abs().max().clamp_min(1e-30)
                    q8 = torch.exp2(torch.floor(torch.log2((100.0 if f8 == torch.float8_e4m3fnuz else 16000.0) / m)))
                    t.copy_(((t.float() * q8).to(f8).float() / q8).to(t.dtype))
        if forked:
            torch.cuda.current_stream().wait_stream(side)
        else:
            self._enqueue_qg(ws, R)
        if rt.stop_before_decoder:
            tk('end')
            return
        # a16-a19: decoder
        tk('decoder')
        self._enqueue_decoder(ws, R)
        tk('heads')
        self._enqueue_heads(ws, R, sc['dt'])
        tk('decode')
        # a21: NMS-free decode of the last layer (one top-k per sample)
        o.decode_topk(ws['cls'][L - 1], ws['reg'][L - 1], R, self.num_classes, self.max_num, self.post_range_h, ws['boxes'], ws['scores'],
                      ws['labels'], ws['bbox_index'], ws['count'], grp_start=grp, max_grp_rows=sc['max_rows'], payload=ws.get('payload_out'))
        tk('end')

    def _exact_pe(self, ws, featcl, P, V, h, w):
        """Index-exact route: the PE block (MU/pe.py:36-48,64-77,150-166) on UNROUNDED fp32 inputs in ONE split-precision launch
        (mv2d_pe_fused_x3, csrc/pe_x3.hip: a_hi w_hi + a_lo w_hi + a_hi w_lo on bf16 MFMAs, hidden layer hi / lo in LDS, sigmoid, gate
        product and sine-table sum in its epilogue; device-side row count S): pe rows into ws['pe'] (S path), key / value rows as key16 hi +
        lo pairs (T path).  Round 3 ran it as four K-concatenated products on the tile GEMM (hidden layer through HBM) + four split passes:
        1.09 ms (S) / 2.17 ms (T) per 16-sample launch.  No host synchronisation, no allocation: graph-replayable."""
        o, W_, T, rt = ops, self.w, ws['tab'], ws['route']
        md = ws['S_dev']
        if ws.get('pe_hit') and rt.pe_cache_views:
            # some views' matrices repeat (route option pe_cache_views): the frustum rows and the full kernel on the rows of the OTHER views, the gate alone
            # on the table Q for the rows of the repeated ones -- three launches into the same row buffers, every row bit for bit the full kernel's.  The
            # mask is read from device memory (sh['pe_vmask'], uploaded by _host_prepare): one captured graph serves every mask but 0
            sh = ws['shared']
            hw, period, vm = h * w, sh['sine_period'], sh['pe_vmask']
            flag = ws['lo8_flag'] if rt.lo8 else None
            o.pe_frustum_f32(ws['s2pos'], md, P, T['img2lidar'], T['coords_w'], T['coords_h'], T['coords_d'], ws['xa1'], V, h, w, self.depth_num,
                             self.pe_range_h64, ld=self.pe_kp, view_mask=vm, tab_period=period)
            o.pe_fused_x3(ws['xa1'], featcl, md, W_['pe_x3'], sh['sine_tab'], period, Xk=(ws['Xk'], ws['xk_lo']), Xv=(ws['Xf_b'], ws['xv_lo']), M=P,
                          row_index=ws['s2pos'], lo8_flag=flag, Kp=self.pe_kp, view_mask=vm, hw=hw)
            o.pe_gate_rows_x3(sh['pe_q'], featcl, md, W_['pe_x3'], sh['sine_tab'], period, (ws['Xk'], ws['xk_lo']), (ws['Xf_b'], ws['xv_lo']), P, vm, hw,
                              row_index=ws['s2pos'], lo8_flag=flag)
            return
        if ws.get('pe_hit'):
            # the rig's matrices repeat (route option pe_cache): no frustum rows, no frustum MLP -- the gate alone on the table Q, same pe bits
            sh = ws['shared']
            o.pe_gate_x3(sh['pe_q'], featcl, md, W_['pe_x3'], sh['sine_tab'], sh['sine_period'], ws['pe_pos'] if rt.pe_at_pos else ws['pe'], P,
                         row_index=ws['s2pos'], pe_at_index=rt.pe_at_pos)
            return
        if rt.keep_sine_rows:
            # (training route: it also reads the key16 rows and the sine rows)
            o.pe_inputs(ws['s2pos'], md, P, featcl, T['img2lidar'], T['coords_w'], T['coords_h'], T['coords_d'], T['embeds'],
                        self.const['dim_t'], ws['A1'], ws['A2'], ws['Xf_b'], None, V, h, w, self.depth_num,
                        self.pe_range_h64, A_frustum_f32=ws['xa1'], A_sine_f32=ws['xa2'], ld=self.pe_kp)
        else:
            # the unrounded frustum rows alone (round 5: 156 -> ~50 us per 141 k positions; the feature rows are read from the map by the PE kernel)
            o.pe_frustum_f32(ws['s2pos'], md, P, T['img2lidar'], T['coords_w'], T['coords_h'], T['coords_d'], ws['xa1'], V, h, w, self.depth_num,
                             self.pe_range_h64, ld=self.pe_kp)
        sh = ws['shared']
        rows = rt.kind == 'T'
        at_pos = rt.pe_at_pos
        # (pe_fused_x3b, opt-in, has the shipped PE's one instance: route.resolve lets it through for 64 bins with the gate only)
        size = {} if rt.pe_rows_in_waves else dict(Kp=self.pe_kp, gate=self.with_fpe)
        (o.pe_fused_x3b if rt.pe_rows_in_waves else o.pe_fused_x3)(
            ws['xa1'], featcl, md, W_['pe_x3'], sh['sine_tab'], sh['sine_period'], pe=(ws['pe_pos'] if at_pos else ws['pe']) if (not rows or rt.stages) else None,
            Xk=(ws['Xk'], ws['xk_lo']) if rows else None, Xv=(ws['Xf_b'], ws['xv_lo']) if rows else None, M=P, row_index=ws['s2pos'], pe_at_index=at_pos, lo8_flag=ws['lo8_flag'] if (rows and rt.lo8) else None,
            **size)

    def _build_pe_q(self, ws, sh, Pt, V, h, w):
        """The table of the cached frustum MLP, Q [Pt,256] = position_encoder(frustum rows) + b1b at every position of ONE sample, with the matrices
        this frame uploaded: the gate-less PE kernel on a one-row zero table (the gated kernel's bits of P1 + b1b; x + 0.0f keeps every value but
        -0.0f).  Enqueued on the current stream in front of the frame, outside any captured graph; written in place when the table exists, so that
        captured graphs keep a valid pointer.  A once-per-calibration cost (17 MB and ~0.13 ms at cfg2_s)."""
        T, o, d = ws['tab'], ops, self.dev
        a1 = torch.zeros((Pt, self.pe_kp), device=d, dtype=F32)
        o.pe_frustum_f32(torch.arange(Pt, dtype=torch.int32, device=d), torch.tensor([Pt], dtype=torch.int32, device=d), Pt, T['img2lidar'], T['coords_w'],
                         T['coords_h'], T['coords_d'], a1, V, h, w, self.depth_num, self.pe_range_h64, ld=self.pe_kp)
        q = sh.get('pe_q')
        if q is None or tuple(q.shape) != (Pt, C):
            if q is not None:
                sh['pe_q_gen'] = sh.get('pe_q_gen', 0) + 1
            q = sh['pe_q'] = torch.empty((Pt, C), device=d, dtype=F32)
        if sh.get('pe_q_zero') is None:
            sh['pe_q_zero'] = torch.zeros((1, C), device=d, dtype=F32)
        o.pe_fused_x3(a1, None, None, self.w['pe_x3'], sh['pe_q_zero'], 1, pe=q, M=Pt, Kp=self.pe_kp, gate=False)
        self.pe_cache_builds = getattr(self, 'pe_cache_builds', 0) + 1

    def _build_pe_q_views(self, ws, sh, Pt, V, h, w, views):
        """The slices of the per-view table Q [Pt,256] (route option pe_cache_views) of the given views of ONE sample, with the matrices this frame
        uploaded: _build_pe_q's launches on the positions of those views only, each row written in place at its position (pe_at_index).  Enqueued on
        the current stream in front of the frame, outside any captured graph; the slices of the other views are not touched."""
        T, o, d, hw = ws['tab'], ops, self.dev, h * w
        pos = torch.cat([torch.arange(v * hw, (v + 1) * hw, dtype=torch.int32) for v in views]).to(d)
        n = int(pos.numel())
        a1 = torch.empty((n, self.pe_kp), device=d, dtype=F32)
        o.pe_frustum_f32(pos, torch.tensor([n], dtype=torch.int32, device=d), n, T['img2lidar'], T['coords_w'], T['coords_h'], T['coords_d'], a1, V, h, w,
                         self.depth_num, self.pe_range_h64, ld=self.pe_kp)
        q = sh.get('pe_q')
        if q is None or tuple(q.shape) != (Pt, C):
            if q is not None:
                sh['pe_q_gen'] = sh.get('pe_q_gen', 0) + 1
            q = sh['pe_q'] = torch.zeros((Pt, C), device=d, dtype=F32)
        if sh.get('pe_q_zero') is None:
            sh['pe_q_zero'] = torch.zeros((1, C), device=d, dtype=F32)
        o.pe_fused_x3(a1, None, None, self.w['pe_x3'], sh['pe_q_zero'], 1, pe=q, M=n, row_index=pos, pe_at_index=True, Kp=self.pe_kp, gate=False)
        self.pe_cache_builds = getattr(self, 'pe_cache_builds', 0) + 1

    def pe_input_rows(self, ws, positions, V, h, w, f32=False):
        """PE input rows (frustum [n,Kp] = 3 * depth_num columns + zero pad, 192 at 64 bins; sine [n,384]; key16, or unrounded fp32 with f32=True) at the given map positions (int32, device)
        with the calibration tables of the workspace's current frame: the training route needs them for a key position no RoI lists
        (RH/mv2d_t_head.py:80-82)."""
        n = int(positions.numel())
        T, d = ws['tab'], self.dev
        a1 = torch.empty((n, self.pe_kp), device=d, dtype=self.K16)
        a2 = None if self.no_sin_enc else torch.empty((n, 384), device=d, dtype=self.K16)       # (no sine branch: no sine rows, None in their place)
        xb = torch.empty((n, C), device=d, dtype=self.K16)
        a1f = torch.empty((n, self.pe_kp), device=d, dtype=F32) if f32 else None
        a2f = torch.empty((n, 384), device=d, dtype=F32) if (f32 and not self.no_sin_enc) else None
        ops.pe_inputs(positions.contiguous(), torch.tensor([n], dtype=torch.int32, device=d), n, ws['featcl'], T['img2lidar'], T['coords_w'],
                      T['coords_h'], T['coords_d'], T['embeds'], self.const['dim_t'], a1, a2, xb, None, V, h, w, self.depth_num, self.pe_range_h64,
                      A_frustum_f32=a1f, A_sine_f32=a2f, ld=self.pe_kp)
        return (a1f, a2f) if f32 else (a1, a2)

    def _enqueue_qg(self, ws, R):
        """a6-a8, a13: QueryGenerator on the RoI features -> reference points -> query positional embedding."""
        o, W_, tk = ops, self.w, self._tick
        if not self.qg.is_default:
            return self._enqueue_qg_shape(ws, R)
        # a6: QueryGenerator: conv3x3 + ReLU + AvgPool2d(s) fused, one block per RoI (index-exact route: in split precision on the hi + lo cells)
        tk('qg_conv_gemm')
        if ws['route'].conv_x3:
            o.qg_conv_pool_x3(ws['roi_feat'], ws['roi_lo'], W_['qg_conv_wx3'], W_['qg_conv_b'], ws['x2'], R=R, roi_size=self.roi_size)
        else:
            o.qg_conv_pool(ws['roi_feat'], W_['qg_conv_wp'], W_['qg_conv_b'], ws['x2'], R=R, roi_size=self.roi_size)
        tk('qg_rest')
        rt = ws['route']
        if rt.qg_tail_fused and self._qg_tail_dims and not rt.keep_sine_rows:
            # the three linears and the query-embedding kernel below as one launch (bitwise the same outputs; enc[:, :1024], enc1, enc2 are not written)
            o.qg_tail_x3(ws['x2'], ws['enc'], W_['qg_fc_wx'], W_['qg_fc_b'], W_['qg_e0_wx'], W_['qg_e0_b'], W_['qg_e2_wx'], W_['qg_e2_b'],
                         W_['qg_c_w'], W_['qg_c_b'], ws['minv'], self.const['dim_t'], self.pc_range_h, W_['qe_w0x'], W_['qe_b0'], W_['qe_w2x'],
                         W_['qe_b2'], ws['center'], ws['xyz'], ws['ref'], ws['posemb'], ws['qpos'], R=R)
            return
        o.linear_x3(ws['x2'], W_['qg_fc_wx'], W_['qg_fc_b'], N=1024, K=256, act=1, clamp=5e3, out=ws['enc'], ldc=1056, M=R)
        o.linear_x3(ws['enc'], W_['qg_e0_wx'], W_['qg_e0_b'], N=512, K=1056, act=1, out=ws['enc1'], M=R)
        o.linear_x3(ws['enc1'], W_['qg_e2_wx'], W_['qg_e2_b'], N=256, K=512, act=1, out=ws['enc2'], M=R)
        # fc_center + reference points (a7/a8) + pos2posemb3d + query_embedding (a13) in one row-fused kernel
        o.query_embed_fused_x3(ws['enc2'], W_['qg_c_w'], W_['qg_c_b'], ws['minv'], self.const['dim_t'], self.pc_range_h, W_['qe_w0x'],
                               W_['qe_b0'], W_['qe_w2x'], W_['qe_b2'], ws['center'], ws['xyz'], ws['ref'], ws['posemb'], ws['qpos'], R=R)

    def _enqueue_qg_shape(self, ws, R):
        """_enqueue_qg for a query generator of other than the shipped shape (index-exact route: the cells are key16 hi + lo pairs).  Trunk: every
        shared conv but the last writes its cells for the next one (mv2d_qg_conv_cells_x3); the last one is the fused conv + AvgPool launch of the
        shipped shape, or writes the fp32 cell-major rows the first fc reads (with_avg_pool=False); without convs the RoI cells are pooled /
        widened by mv2d_avgpool_cells.  Then the plan's linears on mv2d_linear_x3, and fc_center + reference points + query embedding: the row-fused
        kernel when fc_center reads 256 columns, the tile linear + mv2d_refpoint_posemb + two linears otherwise."""
        o, W_, tk, qs, s = ops, self.w, self._tick, self.qg, self.roi_size
        tk('qg_conv_gemm')
        hi, lo = ws['roi_feat'], ws['roi_lo']
        for i, (wx3, b) in enumerate(W_['qg_convs']):
            if i < qs.convs - 1:
                nh, nl = ws[f'qg_cells_hi{i & 1}'], ws[f'qg_cells_lo{i & 1}']
                o.qg_conv_cells(hi, lo, wx3, b, out_hi=nh, out_lo=nl, R=R, roi_size=s)
                hi, lo = nh, nl
            elif qs.pooled:
                o.qg_conv_pool_x3(hi, lo, wx3, b, ws['x2'], R=R, roi_size=s)
            else:
                o.qg_conv_cells(hi, lo, wx3, b, out_f32=ws['qg_flat'], R=R, roi_size=s)
        if qs.convs == 0:
            if qs.pooled:
                o.avgpool_cells(hi, lo, ws['x2'], R, self.cells)
            else:
                o.avgpool_cells(hi, lo, ws['qg_flat'].view(R * self.cells, C), R * self.cells, 1)
        tk('qg_rest')
        for l in W_['qg_lin']:
            o.linear_x3(ws[l['src']], l['wx'], l['b'], N=l['N'], K=l['K'], act=1, clamp=l['clamp'], out=ws[l['dst']], ldc=l['ldc'], M=R)
        last = ws[W_['qg_last']]
        if qs.center_in == C:
            o.query_embed_fused_x3(last, W_['qg_c_w'], W_['qg_c_b'], ws['minv'], self.const['dim_t'], self.pc_range_h, W_['qe_w0x'],
                                   W_['qe_b0'], W_['qe_w2x'], W_['qe_b2'], ws['center'], ws['xyz'], ws['ref'], ws['posemb'], ws['qpos'], R=R)
            return
        o.linear_x3(last, W_['qg_c_wx'], W_['qg_c_b16'], N=16, K=last.shape[1], out=ws['qg_center16'], M=R)
        o.refpoint_posemb(ws['qg_center16'], 16, ws['minv'], self.const['dim_t'], ws['xyz'], ws['ref'], ws['posemb'], R, self.pc_range_h)
        o.linear_x3(ws['posemb'], W_['qe_w0x'], W_['qe_b0'], N=C, K=384, act=1, out=ws['qe1'], M=R)
        o.linear_x3(ws['qe1'], W_['qe_w2x'], W_['qe_b2'], N=C, K=C, out=ws['qpos'], M=R)

    def _enqueue_decoder(self, ws, R):
        """CrossAttentionBoxHead.forward's transformer call on already-prepared inputs (qpos, key / value rows, CSR):
        the "decoder ms/iter" half of the headline metric.  Per layer: self attention (bf16x3 MFMA, K / V through LDS), out_proj + LN +
        cross-attention q projection (row-fused, bf16x3), cross attention in the raw key space (query map, tile kernel, context map), out_proj
        + LN, fused FFN (bf16x3) and its tail (slab sum + LN + post_norm + the next layer's in_proj)."""
        o, W_, L, rt = ops, self.w, self.L, ws['route']
        x = ws['x']
        dn = ws.get('dn')                                 # the training forward's own workspace (its route: Route.denoising)
        dbg = ws['dbg_logits'] if rt.debug_attn else None
        maps_fused = not (rt.grouped or rt.xattn_fused) and rt.maps_fused(R)
        # the cross attention's rows, shared by all layers (raw key space): key16 hi rows, their lo halves on the index-exact route, launch order
        xk_rows, xv_rows = ws['xk_rows'], ws['xv_rows']
        lo_k, lo_v = (ws['xk_lo'], ws['xv_lo']) if rt.attn_lo else (None, None)
        rows = dict(Xk_lo=lo_k, Xv_lo=lo_v, empty_nan=self.empty_nan, order=ws['q_order'] if rt.q_order else None)

        def tile_attn(i):
            if dbg is not None:
                ws['dbg_q'][i].copy_(ws['q'])
            o.xattn_tile(ws['Qt'], xk_rows, xv_rows, ws['row_ptr'], ws['col_idx'], ws['zh'], R, waves=rt.xattn_waves,
                         dbg_logits=None if dbg is None else dbg[i], **rows)

        # the decoder starts from target = 0 (cross_attention_head.py:32): layer 0 reads a constant zero buffer and qpos directly, from
        # layer 1 on x / xq are the buffers the fused FFN tail writes
        x_in, xq_in = ws['zero_rows'], ws['qpos']
        fold0 = rt.fold_sa0
        if fold0 and ws.get('sa0_ver') != self._weights_version:
            # (first run on this workspace after the weights changed: the eager warm-up in front of a graph capture comes through here)
            ws['sa0_ctx'].copy_(W_['sa_in_b0'][2 * C:].expand(ws['sa0_ctx'].shape[0], C))
            ws['sa0_ver'] = self._weights_version
        for i in range(L):
            if i == 1:
                x_in = x
            sa_ctx = ws['ctx']
            if i == 0 and fold0:
                sa_ctx = ws['sa0_ctx']
            else:
                if i == 0:
                    o.linear_x3(xq_in, W_['sa_in_wx0'], W_['sa_in_b0'], N=3 * C, K=C, A2=x_in, n_split=2 * C, out=ws['qkv'], M=R)
                if dn:
                    o.self_attn_dn(ws['qkv'], dn[0], dn[1], out=ws['ctx'])      # training: denoising rows first (train_forward)
                else:
                    o.self_attn(ws['qkv'], ws['ctx'], R, grp_start=ws['grp_start'], max_grp_rows=ws.get('max_rows', 0))
            sa_args = (sa_ctx, x_in, W_[f'sa_out_wx{i}'], W_[f'sa_out_b{i}'], (W_[f'ln0_w{i}'], W_[f'ln0_b{i}']), ws['x1'])
            q_args = dict(qpos=ws['qpos'], Wq_x3=W_[f'ca_q_wx{i}'], bq=W_[f'ca_q_b{i}'], qscale=ops.SCALE_Q, M=R)
            out_args = (ws['x1'], W_[f'ca_out_wx{i}'], W_[f'ca_out_b{i}'], (W_[f'ln1_w{i}'], W_[f'ln1_b{i}']), ws['x2'])
            mapA, mapB, bv = W_[f'ca_mapA{i}'], W_[f'ca_mapB{i}'], W_[f'ca_v_b{i}']
            if maps_fused:
                o.attn_out_qmap_x3(*sa_args, WA=mapA, Qt=ws['Qt'], **q_args)
                tile_attn(i)
                o.attn_out_zmap_x3(ws['zh'], mapB, bv, ws['row_ptr'], *out_args, empty_nan=self.empty_nan, M=R)
            else:
                o.attn_out_fused_x3(*sa_args, q_out=ws['q'], **q_args)
                if rt.grouped:
                    o.xattn_group(ws['q'], mapA, mapB, bv, xk_rows, xv_rows, ws['row_ptr'], ws['grp_tab'], out=ws['ctx'], R=R, **rows)
                elif rt.xattn_fused:
                    o.xattn_fused(ws['q'], mapA, mapB, bv, xk_rows, xv_rows, ws['row_ptr'], ws['col_idx'], out=ws['ctx'], R=R, deal=rt.xattn_deal, qb=rt.xattn_qb or None, **rows)
                else:
                    o.xattn_qmap(ws['q'], mapA, ws['Qt'], R=R)
                    tile_attn(i)
                    o.xattn_ctxmap(ws['zh'], mapB, bv, ws['row_ptr'], ws['ctx'], R, empty_nan=self.empty_nan)
                o.attn_out_fused_x3(ws['ctx'], *out_args, M=R)
            # eight hidden slices accumulated per block: 4 slabs to write and re-read instead of 32 at the shipped width (round 3: 8371 vs 8289
            # samples/s for 8 vs 4 slices, and half the slab traffic).  It fixes the summation order, so it is NOT chosen by the row count or the
            # width: a sample's result must not depend on the batch it is in.  ws['parts'] holds exactly the ceil(F / 512) slabs the kernel writes
            # (ops.ffn_fused_x3 checks it), and the tail sums exactly those.
            G = ops.FFN_GROUPS
            parts = ws['parts']
            o.ffn_fused_x3(ws['x2'], W_[f'ffn_w1x{i}'], W_[f'ffn_b1{i}'], W_[f'ffn_w2x{i}'], parts, R, groups=G)
            nxt = i + 1 < L
            o.ffn_out_fused_x3(parts, W_[f'ffn_b2{i}'], ws['x2'], (W_[f'ln2_w{i}'], W_[f'ln2_b{i}']), (W_['post_w'], W_['post_b']),
                               x, ws['qpos'], None, outs=ws['outs'][i], Win_x3=W_[f'sa_in_wx{i + 1}'] if nxt else None,
                               b_in=W_[f'sa_in_b{i + 1}'] if nxt else None, qkv=ws['qkv'] if nxt else None, M=R)

    def _enqueue_heads(self, ws, R, dt):
        # a14: every per-layer cls / reg branch + the reference-point tail in ONE launch (row-block fused, bf16x3).  Route.last_stage_heads: the
        # branches of the LAST decoder layer only (the reference evaluates all six and reads [-1], cross_attention_head.py:202-242 /
        # RH/mv2d_head.py:170-194); cls / reg of the other layers are then not written
        dt_rows = ws['dt_rows'] if self.kind == 'T' else None
        last = ws['route'].last_stage_heads
        ll, n = (self.L - 1, 1) if last else (0, self.L)
        cls_p, reg_p = (self.cls_ptrs_x3_last, self.reg_ptrs_x3_last) if last else (self.cls_ptrs_x3, self.reg_ptrs_x3)
        outs, cls, reg = ws['outs'][ll:], ws['cls'][ll:], ws['reg'][ll:]
        nf = self.num_reg_fcs
        if self.use_reg_layer:
            # RegLayer regression branches: the class branch alone through the fused kernel, the regression branch + tail through its own
            ops.heads_cls_depth_x3(outs, cls_p, cls, R, n, nf, num_classes=self.num_classes)
            ops.reg_layer_depth_x3(outs, reg_p, ws['ref'], reg, R, n, nf, self.group_reg_dims, self.pc_range_h, dt, dt_rows=dt_rows)
        else:
            ops.heads_depth_x3(outs, cls_p, reg_p, ws['ref'], cls, reg, R, n, nf, self.pc_range_h, dt, dt_rows=dt_rows, num_classes=self.num_classes)

    def _result(self, ws, R, batch=False):
        sel = (lambda t: t) if batch else (lambda t: t[0])
        out = dict(R=R, ws=ws, cls=ws['cls'][:, :R], reg=ws['reg'][:, :R], boxes=sel(ws['boxes']), scores=sel(ws['scores']), labels=sel(ws['labels']),
                   bbox_index=sel(ws['bbox_index']), count=ws['count'] if batch else ws['count'][:1], grp_start=ws['grp_start_h'].clone(),
                   pe_cache=ws.get('pe_cache_state', 'off'),     # 'off' | 'miss' | 'build' | 'hit': what this frame's PE launch was (route options pe_cache, pe_cache_views)
                   pe_cache_views=ws.get('pe_views', ()))        # the views of a sample whose rows read the cached table (pe_cache_views; () otherwise)
        if ws['route'].stages:
            # copies of the intermediate buffers restricted to the REAL rows (the launches run on the bucket size, see _host_prepare)
            rows0 = ('rois', 'minv', 'enc', 'roi_feat', 'center', 'xyz', 'ref', 'posemb', 'qpos', 'match')
            st = {}
            for kk in rows0 + ('roi_mask', 'pos2s', 's2pos', 'S_dev', 'col_idx', 'pe', 'Xk', 'Xf_b', 'dbg_logits', 'dbg_q'):
                if ws.get(kk) is not None:
                    st[kk] = (ws[kk][:R] if kk in rows0 else ws[kk]).clone()
            for kk in ('outs', 'cls', 'reg'):
                st[kk] = ws[kk][:, :R].clone()
            st['row_ptr'] = ws['row_ptr'][:R + 1].clone()
            st['nnz'] = torch.stack([ws['row_ptr'][R], ws['nnz'][1]])          # allowed pairs of the real rows | capacity-overflow flag
            out['stages'] = st
        return out

    def run(self, feat, proposals, img_metas, keep_stages=False, use_graph=False, payload=None):
        """One sample.  feat [V,256,h,w] on the GPU, torch.float32, torch.float16 or torch.bfloat16 (NCHW, or channels_last memory format: zero-copy);
        a 16-bit map is widened element by element inside the kernels that read it (the reference's force_fp32 = x.float(): exact), so the
        results are bit for bit those of run(feat.float(), ...) and no fp32 copy of the map is made.  proposals list of [n,6].
        Enqueues the frame on the current stream; use_graph replays a captured hipGraph of the same shape.  payload (optional): fp32
        [1, max_num * 11 + 1] on the GPU -- the decode kernel also writes the wire row of the all-gather of decoded boxes (mv2d_amd.dist)
        there (its address is part of the graph key)."""
        return self._run([feat], [proposals], [img_metas], keep_stages, use_graph, batch=False, payload=payload)

    def run_batch(self, feats, proposals_list, metas_list, keep_stages=False, use_graph=False, payload=None):
        """Several samples through ONE sequence of launches (the reference runs one sample per call): feats = list of [V,256,h,w]
        maps (or one stacked [B*V,256,h,w] tensor; fp32, fp16 or bf16 like run's, one dtype per call), proposals_list / metas_list = one entry per sample.  Outputs: cls / reg
        [L,R_total,num_classes] / [L,R_total,10] with the samples' queries concatenated (out['grp_start']), boxes [B,max_num,9], scores, labels, count [B]."""
        return self._run(feats, proposals_list, metas_list, keep_stages, use_graph, batch=True, payload=payload)

    def _run(self, feats, proposals_list, metas_list, keep_stages, use_graph, batch, payload=None):
        B = len(proposals_list)
        if payload is not None:
            assert payload.is_cuda and payload.dtype == F32 and payload.is_contiguous() and tuple(payload.shape) == (B, self.max_num * 11 + 1), \
                'payload: fp32 [samples, max_num * 11 + 1] on the GPU'
        stacked = torch.is_tensor(feats)
        fl = [feats] if stacked else list(feats)
        for f in fl:
            assert f.is_cuda and f.dim() == 4 and f.shape[1] == C
        map_dtype = fl[0].dtype
        ops.map_format(map_dtype)                         # ValueError for anything but fp32 / fp16 / bf16
        if any(f.dtype != map_dtype for f in fl):
            raise ValueError(f'mv2d engine: the feature maps of a batch must share one dtype, got {sorted({str(f.dtype) for f in fl})}')
        rt = route.resolve(self, self.kind, self.exact, self.depth_num, map_dtype, keep_stages, use_graph,     # (ValueError for impossible combinations)
                           pe_options=dict(with_fpe=self.with_fpe, no_sin_enc=self.no_sin_enc, LID=self.LID))
        if not self.qg.is_default and not rt.conv_x3:
            raise ValueError('mv2d engine: a query generator of other than the shipped shape runs on the index-exact route only (exact=True, the default, '
                             "without 'conv' in exact_skip): the engine has no key16-mode plan for " + repr(tuple(self.qg)))
        if stacked or B == 1:
            feat = fl[0]
            if not (feat.is_contiguous(memory_format=torch.channels_last) and not feat.is_contiguous()):
                feat = feat.contiguous()
            V, _, h, w = feat.shape
            ptrs = (feat.data_ptr(),)
        else:
            assert len(fl) == B
            feat = [f.contiguous() for f in fl]
            Vg, _, h, w = feat[0].shape
            assert all(tuple(f.shape) == tuple(feat[0].shape) for f in feat), 'samples of a batch share one map shape'
            V = Vg * B
            ptrs = tuple(f.data_ptr() for f in feat)
        assert V % B == 0
        ws, R, sc = self._host_prepare(proposals_list, metas_list, V, h, w, rt)
        # upload of the per-frame tables (RoI list, view / sample offsets, time steps): stream-ordered before the frame, outside the captured graph.
        # The "staging consumed" event stays at the END of the frame: recording it right behind this copy would let the host run a frame ahead on every
        # stream; measured in round 3: +1 % in long runs but 7400-7900 instead of 8300 samples/s in short ones -- without the host's wait the four
        # streams drift into phase and their wide kernels collide (LOG.md section 8)
        ws['dyn_d'].copy_(ws['dyn_h'], non_blocking=True)
        ws['payload_out'], ws['route'] = payload, rt
        Rc = sc['cap']                     # launches run on the bucket size; R = the real rows
        if rt.debug_attn:
            ws['dbg_logits'] = torch.zeros((self.L, 8, ws['col_cap']), device=self.dev, dtype=F32)
            ws['dbg_q'] = torch.zeros((self.L, Rc, C), device=self.dev, dtype=F32)
        else:
            ws.pop('dbg_logits', None); ws.pop('dbg_q', None)
        if not use_graph:
            self._enqueue(ws, feat, Rc, V, h, w, sc)
            self._mark_done(ws)
            return dict(self._result(ws, R, batch), dt=sc['dt'])
        # the graph bakes in the input pointers (the producer's output buffers are static under graph replay) and the
        # frame scalars; anything else changing (RoI boxes, calibration tables, feature values) is data.  The route carries every option;
        # load_state() re-allocates the weights.
        gkey = (ptrs, 0 if payload is None else payload.data_ptr(), sc['pad_h'], sc['pad_w'], sc['max_rows'], self.num_classes, self.roi_size,
                self.use_reg_layer, self.group_reg_dims, self.num_reg_fcs, self._weights_version, rt)
        graphs = ws.setdefault('graphs', {})             # one graph per (input buffers, frame scalars): a producer that alternates between
        g = graphs.get(gkey)                             # a few static output buffers replays a few graphs, it does not re-capture
        # A key's graph exists in up to two FORMS: with the full PE launches, or with the gate-only one (pe_hit, route option pe_cache; pe_cache_views: the
        # three split launches, whatever the mask's value).  ws['graphs']
        # holds the form the key's last frame ran, the other one is parked beside it and swapped back in when the form flips (a rig's first frame
        # captures the full form, its second the hit form; a stream never re-captures a form it has)
        hit, parked = ws['pe_hit'], ws.setdefault('graphs_other_pe_form', {})
        if g is not None and g[2] != hit:
            other = parked.pop(gkey, None)
            if len(parked) >= 32:
                parked.pop(next(iter(parked)))
            parked[gkey] = graphs.pop(gkey)
            g = other
            if g is not None:
                graphs[gkey] = g
        if ws.pop('graph_stale', False):
            graphs.clear(); parked.clear()
            g = None
        if g is None:
            prof, self.prof = self.prof, None
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._enqueue(ws, feat, Rc, V, h, w, sc)                   # warm-up outside capture (lazy inits)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            # thread-local capture mode: another thread of the process (RCCL's proxy, a data loader) may call into HIP while this one captures
            with torch.cuda.graph(g, capture_error_mode='thread_local'):
                self._enqueue(ws, feat, Rc, V, h, w, sc)
            self.prof = prof
            if len(graphs) >= 32:      # (input buffers x payload rows a producer cycles through: bench.py replays 12 per engine)
                graphs.pop(next(iter(graphs)))
            graphs[gkey] = (g, feat, hit)
        else:
            g = g[0]
        g.replay()
        self._mark_done(ws)
        return dict(self._result(ws, R, batch), dt=sc['dt'])

    def train_forward(self, out, dn_ref=None, dn_single=0):
        """Training forward of the decoder + heads on top of a finished ``run`` of ONE sample: the decoder runs again
        over [denoising queries | the sample's queries] with the self-attention mask of ``prepare_for_dn`` evaluated in the kernel and the
        denoising rows attending to every key some RoI can see (RH/mv2d_t_head.py:90-98: ``cross_attn_mask.all(dim=0)``;
        RH/mv2d_s_head.py:158-171).  ``dn_ref`` [pad,3] normalised reference points of the denoising queries (``train.prepare_for_dn``),
        ``dn_single`` rows per group.  Returns (all_cls [L,pad+R,num_classes], all_reg [L,pad+R,10]); the denoising rows' velocities are not divided
        by the frame time step (the reference splits them off before ``_bbox_forward`` does that, RH/mv2d_t_head.py:104-110,132-137).
        Without ``dn_ref`` the inference outputs of all layers are returned (use_denoise=False).  Forward only; synchronises."""
        ws, R = out['ws'], out['R']
        L, d, o, W_ = self.L, self.dev, ops, self.w
        if ws['B'] != 1:
            raise ValueError('train_forward: one sample per run (the reference asserts the same, RH/mv2d_s_head.py:249)')
        row_ptr = ws['row_ptr'][:R + 1]
        nnz = int(row_ptr[R].item())
        if int(ws['nnz'][1].item()) != 0:
            raise RuntimeError('mv2d engine: CSR capacity exceeded (raise col_cap_per_query)')
        col_fb = None
        if self.kind == 'T' and bool((row_ptr[1:] == row_ptr[:-1]).any().item()):
            # the reference un-masks the key at map position (view 0, 0, 0) for a RoI without a visible key in training
            # (RH/mv2d_t_head.py:80-82); if no RoI lists that position its key / value rows are appended behind the S listed ones
            from .train import fallback_key_csr
            s0 = int(ws['pos2s'][0].item())
            if s0 < 0:
                s0 = int(ws['S_dev'].item())
                V_, h_, w_ = ws['map_shape']
                # the PE row of that one position, fp32-class (K-concatenated products like the index-exact route; one row, outside any graph)
                a1f, a2f = self.pe_input_rows(ws, torch.zeros(1, dtype=torch.int32, device=d), V_, h_, w_, f32=True)
                # the feature row of map position 0 comes from the INPUT map: the masked transposition (round 5) writes only the rows inside some RoI's
                # rectangle, and position 0 is by construction outside all of them here
                fin = ws['feat_in']
                fin0 = fin[0] if isinstance(fin, (list, tuple)) else fin
                if fin0.is_contiguous(memory_format=torch.channels_last) and not fin0.is_contiguous():
                    f0 = fin0.permute(0, 2, 3, 1).reshape(-1, C)[:1].float().contiguous()
                else:
                    f0 = fin0[0, :, 0, 0].reshape(1, C).float().contiguous()     # (one row of a 16-bit map, widened: the map itself is never copied)
                def mlp1(x32, n1, n2, **kw):
                    h3 = o.gemm_bf16(o.split3_rows(x32), self._c3(n1), W_['pe_b' + n1[1:]], act=1, split3=True)
                    return o.gemm_bf16(h3, self._c3(n2), W_['pe_b' + n2[1:]], out_dtype=F32, **kw)
                pg = mlp1(a1f, 'w1a', 'w1b', **(dict(mul=mlp1(f0, 'wr', 'we', act=2)) if self.with_fpe else {}))        # (the PE's switches: no gate / no sine term)
                pe0 = pg if self.no_sin_enc else mlp1(a2f, 'w2a', 'w2b', add=pg)
                ws['Xk'][s0:s0 + 1].copy_(o.f32_to_key16(pe0 + f0)); ws['Xf_b'][s0:s0 + 1].copy_(o.f32_to_key16(f0))
            row_ptr, col_fb, _ = fallback_key_csr(row_ptr.clone(), ws['col_idx'][:int(row_ptr[R].item())].clone(), s0)
        no_dn = dn_ref is None or dn_ref.shape[0] == 0
        if no_dn and col_fb is None:
            return ws['cls'][:, :R].clone(), ws['reg'][:, :R].clone()
        if no_dn:
            dn_ref = torch.zeros((0, 3), device=d, dtype=F32)
        pad = int(dn_ref.shape[0])
        T = pad + R
        col = ws['col_idx'][:nnz] if col_fb is None else col_fb
        nnz = int(col.numel())
        keys = torch.unique(col).to(torch.int32)               # every key at least one RoI can see (sorted)
        nk = int(keys.numel())
        e = lambda *shape: torch.empty(shape, device=d, dtype=F32)  # noqa: E731
        posemb = o.posemb3d(dn_ref.to(F32).contiguous(), self.const['dim_t'])
        q1 = o.linear_x3(posemb, W_['qe_w0x'], W_['qe_b0'], N=C, K=384, act=1)
        qdn = o.linear_x3(q1, W_['qe_w2x'], W_['qe_b2'], N=C, K=C)
        tws = dict(B=1, Vg=ws['Vg'], dn=(pad, max(int(dn_single), 1)), route=ws['route'].denoising(), grp_start=None, xk_rows=ws['xk_rows'], xv_rows=ws['xv_rows'],
                   Qt=torch.empty((T, 16 * C), device=d, dtype=self.K16), zh=e(T, 8 * C),
                   row_ptr=torch.cat([torch.arange(pad, device=d, dtype=torch.int32) * nk, row_ptr + pad * nk]),
                   col_idx=torch.cat([keys.repeat(pad), col]).contiguous(),
                   ref=torch.cat([dn_ref.to(F32), ws['ref'][:R]]).contiguous(), qpos=torch.cat([qdn, ws['qpos'][:R]]).contiguous(),
                   zero_rows=torch.zeros(T, C, device=d), qkv=e(T, 3 * C), parts=e(self.ffn_slabs, T, C), outs=e(L, T, C), cls=e(L, T, self.num_classes),
                   reg=e(L, T, 10), dt_rows=torch.cat([torch.zeros(pad, device=d), torch.full((R,), float(out.get('dt', 0.0)), device=d)]))
        for n in ('x', 'x1', 'x2', 'ctx', 'q'):
            tws[n] = e(T, C)
        self._enqueue_decoder(tws, T)
        self._enqueue_heads(tws, T, float(out.get('dt', 0.0)))
        return tws['cls'], tws['reg']

    @staticmethod
    def _mark_done(ws):
        sh = ws['shared']
        if 'done_ev' not in sh:
            sh['done_ev'] = torch.cuda.Event()
        sh['done_ev'].record()

    def clone_shared(self):
        """A second engine sharing the packed weights / constant tables but with its own workspaces, so that several
        frames can be in flight on different HIP streams (one engine per stream)."""
        other = object.__new__(HeadEngine)
        other.__dict__.update(self.__dict__)
        other._ws = {}
        other._ws_base = {}
        other._shape_cache = self._shape_cache      # pure functions of the padding geometry: shared
        other.prof = None
        return other

    @staticmethod
    def _check_capacity(ws):
        _, nnz_over, _, _, _, grp_over, lo8_sat, _ = ws['ctl'].tolist()       # nnz[2] | qt_ctl[2] | grp_ctl[2] | lo8_flag: one copy to the host
        if nnz_over != 0:
            raise RuntimeError('mv2d engine: CSR capacity exceeded (raise col_cap_per_query)')
        if grp_over != 0:
            raise RuntimeError('mv2d engine: union-list capacity of the shared-tile cross attention exceeded (a CSR row lists a key twice?)')
        if lo8_sat != 0:
            import warnings
            warnings.warn('mv2d engine: key / value rows beyond +-224 in this frame: their 8-bit lo halves saturated (those elements keep key16 precision); '
                          'set HeadEngine.lo8_rows = False for fp16 lo rows', RuntimeWarning, stacklevel=3)

    def results(self, out):
        """Synchronising accessor: sliced (boxes [K,9], scores [K], labels [K]) like simple_test returns."""
        n = int(out['count'][0].item())
        self._check_capacity(out['ws'])
        return out['boxes'][:n], out['scores'][:n], out['labels'][:n]

    def results_batch(self, out):
        """Synchronising accessor of run_batch: one (boxes [K,9], scores [K], labels [K]) per sample."""
        counts = out['count'].tolist()
        self._check_capacity(out['ws'])
        return [(out['boxes'][b, :n], out['scores'][b, :n], out['labels'][b, :n]) for b, n in enumerate(counts)]
