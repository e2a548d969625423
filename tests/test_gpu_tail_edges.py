"""The last four kernels of a frame -- decode_topk_kernel<STREAM> / decode_rank_emit, result_pack_kernel, pack_detections_kernel (csrc/geometry.hip)
and nms_bev_kernel (csrc/nms.hip) -- against the CPU expectations of tests/tail_cases.py (-m gpu): sizes around max_num, the 1024 survivor
slots and the LDS / streamed split, ties of every size at the K-th rank (a plateau of equal logits, one NaN pattern, neighbouring floats, the
signed zeros and infinities), centres on and one ulp outside the range, counts 0 / 1 / 1024, scores equal to the threshold, NaN and -inf
scores, garbage behind `count`, and rotated boxes that are identical, nested, touching, degenerate, chained and tied.
Integers (labels, bbox_index, counts, keep masks, the order of the packed rows) and copies (pack and wire outputs) are compared exactly; the
decoded floats with the bounds of test_gpu_kernels.py::test_decode_topk_bit_exact (1e-6 scores, 1e-5 boxes).  Every output buffer handed to
a kernel is filled with a sentinel first and must be untouched behind `count` (ops.nms_bev allocates its own output: there the rows behind
`count` are not looked at).  The tie cases run twice and must agree bit for bit.
tests/test_tail_cases_cpu.py shows what these comparisons can tell apart."""
import pytest
import torch

import tail_cases as tc

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = -777.0, -7


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    from mv2d_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def relerr(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _bits(ts):
    """the tensors as integers: bit-for-bit comparison, NaN included"""
    return [t.cpu().view(torch.int32) if t.dtype == torch.float32 else t.cpu() for t in ts]


def _decode_launch(dev, cls, reg, R, N, max_num, grp_start=None, max_grp_rows=0, payload=False):
    """(boxes [G*max_num,9], scores, labels, bbox_index, count [G], payload or None) of one launch on sentinel-filled buffers"""
    from mv2d_amd import ops
    G = 1 if grp_start is None else grp_start.numel() - 1
    boxes = torch.full((G * max_num, 9), SENT_F, device=dev)
    scores = torch.full((G * max_num,), SENT_F, device=dev)
    labels = torch.full((G * max_num,), SENT_I, dtype=torch.int64, device=dev)
    bidx = torch.full((G * max_num,), SENT_I, dtype=torch.int64, device=dev)
    cnt = torch.full((G,), SENT_I, dtype=torch.int32, device=dev)
    pay = torch.full((G, max_num * 11 + 1), SENT_F, device=dev) if payload else None
    ops.decode_topk(cls.to(dev), reg.to(dev), R, N, max_num, tc.POST, boxes, scores, labels, bidx, cnt, grp_start=None if grp_start is None
                    else grp_start.to(dev), max_grp_rows=max_grp_rows, payload=pay)
    torch.cuda.synchronize()
    return boxes, scores, labels, bidx, cnt, pay


def _check_decoded(what, boxes, scores, labels, bidx, n, exp):
    """one sample's [max_num] output rows against (boxes, scores, labels, bbox_index) of decode_ranked"""
    eb, es, el, ei = exp
    assert n == eb.shape[0], f'{what}: count {n}, expected {eb.shape[0]}'
    boxes, scores, labels, bidx = boxes.cpu(), scores.cpu(), labels.cpu(), bidx.cpu()
    assert torch.equal(labels[:n], el) and torch.equal(bidx[:n], ei), \
        f'{what}: {int(((labels[:n] != el) | (bidx[:n] != ei)).sum())} of {n} ranked (query, class) entries differ'
    assert bool((boxes[n:] == SENT_F).all()) and bool((scores[n:] == SENT_F).all()) and bool((labels[n:] == SENT_I).all()) and \
        bool((bidx[n:] == SENT_I).all()), f'{what}: rows behind count were written'
    if n:
        nan = torch.isnan(es)
        assert torch.equal(torch.isnan(scores[:n]), nan), f'{what}: NaN scores'
        if not bool(nan.all()):
            assert relerr(scores[:n][~nan], es[~nan]) < 1e-6, what
        assert relerr(boxes[:n], eb) < 1e-5, what


@pytest.mark.parametrize('name', tc.DECODE_CASES)
def test_decode_topk_edge_cases(dev, name):
    c, exp = tc.decode_case(name), tc.decode_expected(name)
    out = _decode_launch(dev, c.cls, c.reg, c.R, c.N, c.max_num)
    _check_decoded(name, *out[:4], int(out[4].item()), exp)
    if c.tie:                                                     # which of the equal logits are taken must not depend on arrival order
        again = _decode_launch(dev, c.cls, c.reg, c.R, c.N, c.max_num)
        assert all(torch.equal(a, b) for a, b in zip(_bits(out[:5]), _bits(again[:5]))), f'{name}: two launches differ'


def test_decode_topk_grouped_launch_with_payload(dev):
    """samples of 1, 0, 130 and 103 rows in one launch: n < max_num, an empty sample, a plain one and 1030 equal logits; the payload rows of the
    same launch are mv2d_pack_detections of its outputs"""
    from mv2d_amd import ops
    g = tc.group_case()
    G, M = len(tc.GROUP_ROWS), g.max_num
    runs = [_decode_launch(dev, g.cls, g.reg, g.R, g.N, M, g.grp_start, g.max_grp_rows, payload=True) for _ in range(2)]
    boxes, scores, labels, bidx, cnt, pay = runs[0]
    counts = cnt.cpu().tolist()
    for s in range(G):
        sl = slice(s * M, (s + 1) * M)
        _check_decoded(f'sample {s}', boxes[sl], scores[sl], labels[sl], bidx[sl], counts[s], g.expected[s])
    assert counts[1] == 0
    want = torch.full((G, M * 11 + 1), SENT_F, device=dev)
    ops.pack_detections(boxes.view(G, M, 9), scores.view(G, M), labels.view(G, M), cnt, want, M)
    assert torch.equal(pay, want)
    pay = pay.cpu()
    for s in range(G):
        assert float(pay[s, -1]) == counts[s] and bool((pay[s, counts[s] * 11:-1] == 0).all()), f'payload of sample {s}'
    assert all(torch.equal(a, b) for a, b in zip(_bits(runs[0]), _bits(runs[1]))), 'two launches differ'


# ------------------------------------------------------------------------------------------------ pack
def _result_pack(dev, boxes, scores, labels, count, score_thr, max_num, n_samples=1, in_stride=0):
    from mv2d_amd import ops
    B = n_samples
    ob = torch.full((B, max_num, 9), SENT_F, device=dev)
    os_ = torch.full((B, max_num), SENT_F, device=dev)
    ol = torch.full((B, max_num), SENT_I, dtype=torch.int64, device=dev)
    oc = torch.full((B,), SENT_I, dtype=torch.int32, device=dev)
    ops.result_pack(boxes.to(dev).contiguous(), scores.to(dev).contiguous(), labels.to(dev).contiguous(), count.to(dev), score_thr, max_num, ob, os_,
                    ol, oc, n_samples=B, in_stride=in_stride)
    return ob.cpu(), os_.cpu(), ol.cpu(), oc.cpu()


def _check_packed(what, ob, os_, ol, n, exp):
    eb, es, el = exp
    assert n == es.shape[0], f'{what}: count {n}, expected {es.shape[0]}'
    assert torch.equal(ol[:n], el) and torch.equal(os_[:n], es) and torch.equal(ob[:n], eb), \
        f'{what}: {int(((ol[:n] != el) | (os_[:n] != es)).sum())} of {n} packed rows differ'
    assert bool((ob[n:] == SENT_F).all()) and bool((os_[n:] == SENT_F).all()) and bool((ol[n:] == SENT_I).all()), f'{what}: rows behind count written'


@pytest.mark.parametrize('name', tc.PACK_CASES)
def test_result_pack_edge_cases(dev, name):
    from mv2d_amd import postprocess
    c = tc.pack_case(name)
    exp = tc.pack_expected(c)
    cnt = torch.tensor([c.count], dtype=torch.int32)
    ob, os_, ol, oc = _result_pack(dev, c.boxes, c.scores, c.labels, cnt, c.score_thr, c.max_num, in_stride=c.stride)
    _check_packed(name, ob[0], os_[0], ol[0], int(oc[0]), exp)
    res = postprocess.pack_results(c.boxes.to(dev), c.scores.to(dev), c.labels.to(dev), cnt.to(dev), c.score_thr, c.max_num)
    assert torch.equal(res['labels_3d'], exp[2]) and torch.equal(res['scores_3d'], exp[1]) and torch.equal(res['boxes_3d'], exp[0])
    if name.startswith('ones'):
        again = _result_pack(dev, c.boxes, c.scores, c.labels, cnt, c.score_thr, c.max_num, in_stride=c.stride)
        assert all(torch.equal(a, b) for a, b in zip(_bits((ob, os_, ol, oc)), _bits(again)))


def test_result_pack_batch_of_three(dev):
    from mv2d_amd import postprocess
    bc = tc.pack_batch_case()
    ob, os_, ol, oc = _result_pack(dev, bc.boxes, bc.scores, bc.labels, bc.count, bc.score_thr, bc.max_num, n_samples=3, in_stride=tc.BATCH_STRIDE)
    res = postprocess.pack_results_batch(bc.boxes.to(dev), bc.scores.to(dev), bc.labels.to(dev), bc.count.to(dev), bc.score_thr, bc.max_num)
    for b, c in enumerate(bc.samples):
        exp = tc.pack_expected(c)
        _check_packed(f'sample {b}', ob[b], os_[b], ol[b], int(oc[b]), exp)
        assert torch.equal(res[b]['labels_3d'], exp[2]) and torch.equal(res[b]['scores_3d'], exp[1]) and torch.equal(res[b]['boxes_3d'], exp[0])


# ------------------------------------------------------------------------------------------------ wire
def test_pack_detections_wire_rows(dev):
    from mv2d_amd import dist as mdist, ops
    c = tc.wire_case()
    B = c.count.numel()
    out = torch.full((B, c.max_num * 11 + 1), SENT_F, device=dev)
    ops.pack_detections(c.boxes.to(dev), c.scores.to(dev), c.labels.to(dev), c.count.to(dev), out, c.max_num)
    out = out.cpu()
    assert torch.equal(out, c.expected)
    for b, cnt in enumerate(tc.WIRE_COUNTS):
        n = min(cnt, c.max_num)
        assert float(out[b, -1]) == cnt and bool((out[b, n * 11:-1] == 0).all())
        bx, sc, lb = mdist.unpack_detections(out[b], c.max_num)
        assert torch.equal(bx, c.boxes[b, :n]) and torch.equal(sc, c.scores[b, :n]) and torch.equal(lb, c.labels[b, :n])
    one = torch.full((1, c.max_num * 11 + 1), SENT_F, device=dev)                      # a single sample, its [stride] arrays unbatched
    ops.pack_detections(c.boxes[3].to(dev), c.scores[3].to(dev), c.labels[3].to(dev), c.count[3:4].to(dev), one, c.max_num)
    assert torch.equal(one[0].cpu(), c.expected[3])


# ------------------------------------------------------------------------------------------------ NMS
def _nms(dev, c, stride=None):
    """ops.nms_bev on the case's boxes at in_stride n + 3 (garbage behind count), at most 1024: scores_out[:n] on the host"""
    from mv2d_amd import ops
    stride = min(c.n + 3, 1024) if stride is None else stride
    b, s, l_ = tc._padded(c.boxes, c.scores, c.labels, c.n, stride)
    out = ops.nms_bev(b.to(dev), s.to(dev), l_.to(dev), torch.tensor([c.n], dtype=torch.int32, device=dev), c.thr)
    return out[:c.n].cpu()


def _check_nms(what, out, scores, keep):
    got = torch.isfinite(out)
    assert torch.equal(got, keep), f'{what}: {int((got != keep).sum())} of {keep.numel()} keep flags differ'
    assert torch.equal(out[keep], scores[keep]) and bool((out[~keep] == float('-inf')).all()), what


@pytest.mark.parametrize('name', tc.NMS_CASES)
def test_nms_bev_edge_cases(dev, name):
    c = tc.nms_case(name)
    out = _nms(dev, c)
    _check_nms(name, out, c.scores, tc.nms_expected(name))
    if name in ('identical', 'score_ties'):
        assert torch.equal(_nms(dev, c).view(torch.int32), out.view(torch.int32)), f'{name}: two launches differ'


def test_nms_bev_batch_of_three_through_pack_results(dev):
    from mv2d_amd import ops, postprocess
    from oracle import mv2d_oracle as O
    bc = tc.nms_batch_case()
    args = (bc.boxes.to(dev), bc.scores.to(dev), bc.labels.to(dev), bc.count.to(dev))
    out = ops.nms_bev(*args, bc.thr, n_samples=3).cpu()
    res = postprocess.pack_results_batch(*args, score_thr=0.0, max_per_scene=bc.max_num, nms_thr=bc.thr)
    for b, n in enumerate(tc.BATCH_COUNTS):
        keep = bc.keep[b]
        _check_nms(f'sample {b}', out[b, :n], bc.scores[b, :n], keep)
        exp = O.post_nms_pack(bc.boxes[b, :n][keep], bc.scores[b, :n][keep], bc.labels[b, :n][keep], score_thr=0.0, max_num=bc.max_num)
        assert torch.equal(res[b]['labels_3d'], exp[2]) and torch.equal(res[b]['scores_3d'], exp[1]) and torch.equal(res[b]['boxes_3d'], exp[0])


def test_nms_bev_nan_scores_take_no_part(dev):
    """three NaN scores among 40 boxes: they come out non-finite, suppress nothing and leave the ranks of the others alone"""
    c = tc.nms_nan_case()
    out = _nms(dev, c)
    assert not bool(torch.isfinite(out[list(tc.NAN_AT)]).any())
    _check_nms('finite subset', out[c.finite], c.scores[c.finite], c.keep_finite)
    assert torch.equal(_nms(dev, c).view(torch.int32), out.view(torch.int32)), 'two launches differ'
