"""The route of one frame through the engine -- which kernels run, which buffers they use -- resolved ONCE per call from the option attributes of
a ``HeadEngine``, its ``kind`` / ``exact`` / ``depth_num`` and the call's ``map_dtype`` / ``keep_stages`` / ``use_graph``.  The single list of
switches: ``Route.storage`` is part of the workspace keys, the whole ``Route`` of the hipGraph key.  Needs neither the library nor a GPU."""
import os
from collections import namedtuple
from typing import NamedTuple

import torch


def default_options():
    """name -> default of every option attribute (environment variables are for A/B runs and read when an engine is built)."""
    env = os.environ.get
    return dict(
        prof=None,                    # dict name -> [events] when stage timing is on (bench.py): eager runs then keep to one stream
        fork_qg=True, fuse_maps={'0': False, '1': True}.get(env('MV2D_FUSE_MAPS', ''), None), fuse_xattn=None, group_xattn=None,
        xattn_waves=int(env('MV2D_XATTN_WAVES', '2')), q_order=True, fold_sa0=True, masked_transpose=True, last_stage_heads=False,
        exact_skip=frozenset({'conv'}), lo8_rows=True, pe_at_positions=env('MV2D_PE_AT_POS', '1') != '0', pe_rows_in_waves=False,
        ablate_zero_lo=frozenset(), keep_sine_rows=False, stop_before_decoder=False, force_nc=None, debug_attn=False,
        fuse_qg_tail=env('MV2D_QG_TAIL', '1') != '0', pe_cache=env('MV2D_PE_CACHE', '1') != '0', pe_cache_views=env('MV2D_PE_CACHE_VIEWS', '0') == '1',
        xattn_deal=0,                 # forced block dealing of the one-launch cross attention (0 = the library's policy)
        xattn_qb=0)                   # forced queries per block of the same launch (0 = the library's choice)


OPTIONS = tuple(default_options())


class Route(NamedTuple):
    # ---- the first six fields are the STORAGE part (Route.storage): what HeadEngine._build_ws reads.  Routes that agree in them share workspaces.
    kind: str
    # INDEX-EXACT ROUTE = THE DEFAULT since round 5 (exact=None -> True; exact=False / MV2D_EXACT=0 / test_cfg.index_exact=False selects the
    # opt-in "key16" mode with ONE fp16 rounding of the key side: ~1.3 x faster, 4-22 of 300 ranked indices differ from the reference's).
    # Every 16-bit rounding of the key side is replaced by fp32-class arithmetic -- the PE block in one split-precision kernel on unrounded
    # inputs (csrc/pe_x3.hip), the key / value rows of the tile attention (and, with conv_x3, the query generator's conv) as key16 hi + lo
    # pairs -- so that the INTEGER outputs (labels, bbox_index) can be compared bit for bit with the reference's (tests/test_gpu_golden.py).
    # Enqueue-only and hipGraph-replayable like the key16 mode (bench.py: samples_s_index_exact).
    exact: bool
    # option lo8_rows, round 6: the lo halves of the key / value rows as 8-BIT floats (csrc/common.h "lo8": OCP e4m3 of lo * 2^12, 256-byte
    # rows) -- a (query, key) pair of the cross attention gathers 1.5 KB instead of 2 KB and the row producers write a quarter less.  The lo
    # part carries 2^-12 of a product, its e4m3 rounding 2^-16: all 17 reference parity cases keep their ranked indices (class logits 6.2e-7
    # .. 1.1e-6 of their range against 6.3e-7 .. 8.0e-7 with key16 lo rows, bound 3e-6; an e5m2 lo half or a missing one moves ranks:
    # profiles/r06_ablate_exact.txt).  The kernels decode the bytes to key16 in registers: results are bitwise those of key16 lo rows holding
    # the decoded values.  False: key16 lo rows (rounds 3-5).  The shared-tile kernel (group_xattn) reads key16 lo rows only: it forces lo8 off.
    lo8: bool
    # option pe_at_positions, round 6, S path: the PE rows are written AT THEIR MAP POSITIONS (a position-indexed fp32 map, zero-filled once)
    # instead of compacted in key-list order, so that RoIAlign reads its second map without the position -> row table: one dependent load less
    # in front of every bilinear tap of the PE map (the kernel is a chain of such round trips).  Same values, same arithmetic.  pe_pos: the map
    # is allocated (S path, index-exact route); pe_at_pos: this frame uses it -- not a keep_stages run (it exposes the compact rows), not with
    # the key16 PE kernel; MV2D_PE_AT_POS=0 turns it off (A/B runs).
    pe_pos: bool
    # option group_xattn, round 6, OPT-IN: key tiles SHARED between the queries of a group (csrc/xattn_group.hip: one block per 8 queries that
    # are neighbours in the launch order walks the union of their key lists once through an LDS-DMA ring; wave = head, query / context maps in
    # the same launch).  It reads what it should (1.34-1.68 x the distinct rows instead of 2.99 x at cfg3_t) and is SLOWER than the per-query
    # kernels (242-326 us against 158 + 33 us per cfg3_t layer): eight heads x every union tile is 2.7 x the (wave, tile) steps of the
    # per-query walk, and the 32 KB tiles of the hi + lo route leave the 160 KB of LDS no room to run the queries' own walks side by side
    # (LOG.md, round 6).  None / False: off.  group_tab: its tables are allocated; grouped: this frame runs it (not with debug_attn).
    group_tab: bool
    # T path: the blocks of the per-query tile kernel run in the order of the queries' SMALLEST KEY (mv2d_xattn_query_order): neighbouring
    # blocks of an XCD then read overlapping key sets from its L2 (cfg3_t 54.8 -> 47.6 us per layer; bitwise the same results)
    # S path (round 4): the queries ranked by the smallest RoI they list (own or matched; computed from the correlation lists inside the
    # launch that builds the CSR) -- matched RoIs of different views then run side by side; a no-op for queries that read only their own RoI
    q_order: bool
    # ---- launch-only fields
    map_dtype: torch.dtype  # element format of the feature map: a captured graph holds the launches of ONE format
    # keep_stages run: intermediate buffers nothing downstream reads are written too (pe on the T path, Xk on the S path), whole-map transposition
    stages: bool
    # option exact_skip: stages of the index-exact route that run with the key16 mode's single rounding -- any of 'attn' (hi rows only in the
    # tile attention), 'pe' (fused key16 PE kernel), 'conv' (single-precision RoI conv).  Round 4 (tools/ablate_exact.py,
    # profiles/r04_ablate_exact.txt): with fp16 cells the query generator's conv in SINGLE precision leaves the ranked indices and the
    # class-logit error of the index-exact route where they are (cfg2_s 2 -> 2, cfg3_t 4 -> 4, cfg5_t 2 -> 0 of 300; cls 5.0e-6 -> 6.2e-6 /
    # 5.1e-6 -> 4.9e-6 / 5.8e-6 -> 5.7e-6): its 2304-term dot products average the 2^-12 roundings down, and the 3 x MFMA-bound split-
    # precision kernel (362 vs 123 us per 2400 RoIs) leaves the route: the default skips 'conv'.  Attention rows and PE stay hi + lo:
    # dropping either costs ranks.
    pe_x3: bool             # the split-precision PE block runs (exact and 'pe' not skipped)
    conv_x3: bool           # the split-precision RoI conv runs (exact and 'conv' not skipped)
    attn_lo: bool           # the cross attention reads the lo rows (exact and 'attn' not skipped)
    pe_at_pos: bool         # this frame's PE rows go to the position-indexed map (pe_pos above)
    # option pe_rows_in_waves, round 6, OPT-IN: the split-precision PE block on the second shape of its kernel (csrc/pe_x3b.hip: a wave owns 32
    # rows through both layers of each MLP, the hidden layer stays in registers, the weights go through an LDS-DMA ring shared by the block's 4
    # waves; BITWISE the outputs of csrc/pe_x3.hip).  Measured no faster (1213 vs 1165-1244 us per 250 k rows; 8 waves x 16 rows: 1056 us,
    # bound by 8 x 32 KB of LDS reads per k-step): LOG.md round 6.
    pe_rows_in_waves: bool
    keep_sine_rows: bool    # the training route reads the per-key sine rows (ws['A2']) although the inference kernel does not
    grouped: bool           # this frame's cross attention runs on shared key tiles (group_tab above)
    # option fuse_xattn, S path (rows of similar length): query map -> tile attention -> context map as ONE launch per layer
    # (csrc/xattn_fused.hip, round 5: blocks of 8 queries, Qt / z stay on chip; bitwise the three kernels with one wave per query).  None: on
    # the S path; False / True forces it (xattn_fused_forced: also for the training forward's denoising rows).  Never with debug_attn.
    xattn_fused: bool
    xattn_fused_forced: bool
    # The per-head query / context maps of the tile cross attention run inside the neighbouring row kernels (mv2d_attn_out_qmap_x3 /
    # _zmap_x3: 6 instead of 8 launches per layer, bitwise the same results) for SMALL launches (<= 512 query rows, i.e. one sample per
    # call: the two saved launches per layer count there) and as separate kernels for batches (a row kernel is bound by streaming its
    # weights through ONE CU per 32 rows; the fused ones stream twice as much).  None: by the row count (maps_fused); True / False forces it.
    fuse_maps: object
    # waves per query of the tile kernel: the kernel alone takes the same time with 1, 2 or 4 (it is bound by what the memory system
    # delivers), but a launch with fewer waves leaves more of the chip to the other streams' kernels: cfg2_s 8067 / 8043 / 7869
    # samples/s for 1 / 2 / 4, cfg3_t (rows of ~200 keys) 5803 / 5868 / 5758
    xattn_waves: int
    # Layer 0 of the decoder starts from target = 0 (RH/bbox_heads/cross_attention_head.py:32): the VALUE rows of its self attention are
    # in_proj_v(0) + b_v = b_v for every query, the softmax weights of a row sum to 1, so its context is b_v whatever the queries are
    # (MU/petr_transformer.py:317-370: value = key before the positional embedding = target).  The engine feeds rows of b_v to the
    # out-projection kernel instead of launching the in-projection and the attention core of layer 0 (the reference's own sum of
    # probabilities is 1 +- 1e-7; a NaN query position still poisons the frame one layer later, through its cross attention).  The training
    # forward (denoising mask) keeps the launches.
    fold_sa0: bool
    # T path, key16 mode: the query-generator chain (RoIAlign -> conv -> fcs -> ref points -> query_pos) on a second stream (option fork_qg;
    # not while stage timing is on)
    forked: bool
    # option masked_transpose (round 5): transpose only the map rows inside some RoI's rectangle (see HeadEngine._enqueue, which adds what
    # depends on the call's map); not when forked, for the training route or for keep_stages runs
    masked: bool
    # OPT-IN: evaluate the cls / reg branches of the last decoder layer only (what decoding reads).  Not the default: out['cls'] / out['reg']
    # then carry stale rows for the other layers, and the reference's forward does evaluate all six.  Never for keep_stages runs.
    last_stage_heads: bool
    # tests only (eager runs): keep the pre-softmax per-head logits of every layer's cross attention (out['stages']['dbg_logits']
    # [L,8,col_cap] in CSR order, WITHOUT the per-(query, head) constant q_h . bk_h that cancels in the softmax) and the scaled,
    # projected queries ('dbg_q' [L,R,256]) they were computed from
    debug_attn: bool
    stop_before_decoder: bool   # the autograd training route only needs geometry, RoI features, PE inputs and reference points of a run
    force_nc: object        # bench only (S path): overwrite the correlation lists so that every query reads n_c RoIs
    # experiments only (tools/ablate_exact.py; needs lo8_rows = False): zero the lo halves of the value / key rows after they were written --
    # what a route with hi-only value (or key) rows would compute, at the full route's cost
    ablate_zero_lo: frozenset
    # option fuse_qg_tail: the query generator's MLP tail (shared_fcs.0 -> extra_enc.0 -> extra_enc.2) and the query-embedding kernel run as ONE
    # launch (csrc/qg_tail.hip: the hidden layers stay in LDS, the weights stream through a register ring; BITWISE the four launches it
    # replaces).  Not for keep_stages runs (they expose enc, which the launch does not write); the engine also keeps the four launches for
    # the training route and for weights of other than the shipped dimensions.  MV2D_QG_TAIL=0 turns it off (A/B runs).
    qg_tail_fused: bool
    # option pe_cache: on a rig whose camera matrices repeat from frame to frame, the frustum MLP of the PE (56 of the 72 k-steps of csrc/pe_x3.hip at 64
    # bins, and the frustum-row launch in front of it) is computed ONCE into a per-position table Q = position_encoder(A1) + b1b and a frame runs only
    # the gate (csrc/pe_x3_gate.hip: pe = tab + Q * gate, bit for bit the full kernel's pe).  This field: the route ALLOWS it -- S path, split-precision
    # PE with its gate (with_fpe) and its sine table (not no_sin_enc: Q and the table share one period), no keep_stages run, not the training route's
    # sine rows, not the rows-in-waves shape.  Whether a frame does use the table is decided per frame from its matrices (mv2d_amd/pe_cache.py) and is
    # part of the graph key next to the route.  MV2D_PE_CACHE=0 turns it off (A/B runs).
    pe_cache: bool
    # option pe_cache_views, OPT-IN (default off; MV2D_PE_CACHE_VIEWS=1 or test_cfg.pe_cache_views turns it on): the same cache PER VIEW on the two-frame
    # head.  A sample has 2 * num_views views; the current-frame views of a fixed calibration repeat their matrices, the previous-frame views carry the
    # ego motion.  The table Q holds one slice per view; a frame whose mask of repeated views is not 0 runs three launches into the same key / value row
    # buffers -- the frustum rows of the other views (mv2d_pe_frustum_f32_sel), the full kernel on them (csrc/pe_x3_sel.h) and the gate with row outputs on
    # the repeated views (csrc/pe_x3_gate.hip pe_x3_gate_rows_kernel), every row bit for bit the full kernel's.  The mask is read from device memory: it is
    # not part of the graph key, only "full launches" / "split launches" is.  This field: the route ALLOWS it -- T path, and the conditions of pe_cache.
    # The S path ignores the option.
    pe_cache_views: bool
    # option xattn_deal, tests only: the FORCED block dealing of the one-launch cross attention, handed to ops.xattn_fused(deal=...) -- 1 = a launch of
    # more blocks of 8 queries than CUs is cut into whole rounds of CUs, 2 = into full blocks of 8 (csrc/xattn_fused.hip).  0, the default: the
    # library's policy, a function of the row count alone.  Which block computes a row changes, the row does not (tests/test_gpu_batch_shapes.py).
    # Launch-only.
    xattn_deal: int
    # option xattn_qb, tests only: the FORCED queries per block of the same launch, handed to ops.xattn_fused(qb=...): 4, 8, or with e4m3 lo rows 12.
    # 0, the default: the library's choice, a function of the row count alone.  Launch-only, and the rows do not depend on it (tests/test_gpu_xattn_fused_qb.py).
    xattn_qb: int

    @property
    def storage(self):
        return Storage(*self[:6])

    def maps_fused(self, R):           # do the query / context maps of the tile cross attention run inside the row kernels for a launch of R rows?
        return ((R <= 512) if self.fuse_maps is None else bool(self.fuse_maps)) and not self.debug_attn

    def denoising(self):
        """The route of the training forward's own decoder workspace (ws['dn']: denoising rows first) on top of a finished run of this route: no lo
        rows, no group tables, no launch order, and a masked self attention in layer 0 (so it runs)."""
        return self._replace(attn_lo=False, grouped=False, xattn_fused=self.xattn_fused_forced, q_order=False, fold_sa0=False, debug_attn=False)


Storage = namedtuple('Storage', Route._fields[:6])


def resolve(opts, kind, exact, depth_num, map_dtype=torch.float32, keep_stages=False, use_graph=False, pe_options=None):
    """The Route of one call.  ``opts``: any object with the attributes ``OPTIONS`` (a HeadEngine).  ``pe_options``: the engine's PE switches as a
    dict with any of ``with_fpe`` / ``no_sin_enc`` / ``LID`` (None or a missing key: the shipped value).  ValueError for impossible combinations."""
    o, stages = opts, bool(keep_stages)
    skip, debug, group = o.exact_skip, bool(o.debug_attn), bool(o.group_xattn)
    pe_x3 = exact and 'pe' not in skip
    if depth_num != 64 and not pe_x3:
        raise ValueError(f'mv2d engine: the key16 mode\'s PE kernel (csrc/pe_tab96.hip) is built for depth_num = 64 only; run the index-exact route (exact=True, the default) with depth_num = {depth_num}')
    if depth_num != 64 and o.pe_rows_in_waves:
        raise ValueError(f'mv2d engine: pe_rows_in_waves (csrc/pe_x3b.hip) is built for depth_num = 64 only; unset it for depth_num = {depth_num}')
    # the PE's switches (HeadEngine.with_fpe / no_sin_enc / LID): the key16 mode's PE kernel and the second shape of the split-precision one are
    # built for the shipped PE only
    for key, shipped in (('with_fpe', True), ('no_sin_enc', False), ('LID', True)):
        v = (pe_options or {}).get(key, shipped)
        if v != shipped and not pe_x3:
            raise ValueError(f'mv2d engine: the key16 mode\'s PE kernel (csrc/pe_tab96.hip) is built for {key}={shipped} only; run the index-exact route (exact=True, the default) with {key}={v}')
        if v != shipped and o.pe_rows_in_waves:
            raise ValueError(f'mv2d engine: pe_rows_in_waves (csrc/pe_x3b.hip) is built for {key}={shipped} only; unset it for {key}={v}')
    if map_dtype != torch.float32 and o.pe_rows_in_waves and pe_x3:
        raise ValueError('mv2d engine: pe_rows_in_waves (csrc/pe_x3b.hip) reads fp32 feature maps only; unset it for a torch.float16 / torch.bfloat16 map')
    lo8 = bool(o.lo8_rows) and exact and not group
    if o.ablate_zero_lo and lo8:
        raise ValueError('ablate_zero_lo works on key16 lo rows: set lo8_rows = False')
    assert not (debug and use_graph), 'debug_attn: eager runs only'
    if int(o.xattn_deal) not in (0, 1, 2):
        raise ValueError('mv2d engine: xattn_deal is 0 (the library\'s policy), 1 (whole rounds) or 2 (full blocks)')
    if int(o.xattn_qb) not in (0, 4, 8, 12):
        raise ValueError('mv2d engine: xattn_qb is 0 (the library\'s choice), 4, 8 or 12')
    pe_pos = kind == 'S' and exact and bool(o.pe_at_positions)
    pe_opt = lambda key, shipped: (pe_options or {}).get(key, shipped)      # noqa: E731
    pe_cache_ok = (pe_x3 and bool(pe_opt('with_fpe', True)) and not pe_opt('no_sin_enc', False) and not stages and not o.keep_sine_rows
                   and not o.pe_rows_in_waves)
    pe_cache = bool(o.pe_cache) and kind == 'S' and pe_cache_ok
    pe_cache_views = bool(o.pe_cache_views) and kind == 'T' and pe_cache_ok
    forked = kind == 'T' and (o.prof is None or use_graph) and bool(o.fork_qg) and not exact        # (a graph is captured with stage timing off)
    return Route(
        kind=kind, exact=exact, lo8=lo8, pe_pos=pe_pos, group_tab=group, q_order=bool(o.q_order), map_dtype=map_dtype, stages=stages,
        pe_x3=pe_x3, conv_x3=exact and 'conv' not in skip, attn_lo=exact and 'attn' not in skip, pe_at_pos=pe_pos and pe_x3 and not stages,
        pe_rows_in_waves=bool(o.pe_rows_in_waves), keep_sine_rows=bool(o.keep_sine_rows), grouped=group and not debug,
        xattn_fused=(kind == 'S' if o.fuse_xattn is None else bool(o.fuse_xattn)) and not debug, xattn_fused_forced=bool(o.fuse_xattn),
        fuse_maps=o.fuse_maps, xattn_waves=int(o.xattn_waves), fold_sa0=bool(o.fold_sa0), forked=forked,
        masked=bool(o.masked_transpose) and not forked and not o.keep_sine_rows and not stages,
        last_stage_heads=bool(o.last_stage_heads) and not stages, debug_attn=debug, stop_before_decoder=bool(o.stop_before_decoder),
        force_nc=o.force_nc, ablate_zero_lo=frozenset(o.ablate_zero_lo) if exact else frozenset(),
        qg_tail_fused=bool(o.fuse_qg_tail) and not stages, pe_cache=pe_cache, pe_cache_views=pe_cache_views,
        xattn_deal=int(o.xattn_deal), xattn_qb=int(o.xattn_qb))
