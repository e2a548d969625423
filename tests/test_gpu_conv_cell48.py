"""The query generator's conv3x3 + ReLU + AvgPool2d(7) as two launches (-m gpu; csrc/roiconv.hip): roi_conv_cell48_kernel computes cell 48 of
every RoI with 16 RoIs per MFMA row tile and leaves it in the output buffer, the pooling kernels run three row tiles per RoI and add it last.

The reference does not run the code under test: ops.qg_conv_cells (csrc/roiconv_cells.hip) writes relu(conv + bias) per cell, "bit for bit
those the pooled kernels add up", and the 49 cells are pooled here in the kernels' order -- per column s_fg = 0, then for i in 0..3, r in
0..3 the cell 16 i + 4 fg + r if it is < 49; result ((s_0 + s_1) + (s_2 + s_3)) / 49 (the sums in torch fp32 on the GPU, the division by
numpy on the host: torch multiplies by the reciprocal of a scalar divisor).  Against the library of the commit before the two-launch form
this reference matches bit for bit at every case below (profiles/conv_cell48_kernel_stats.txt)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
# tile edges of the cell-48 launch (16 RoIs per row tile, 64 / 32 per block), an odd last block at two RoIs per block, both sides of the
# switch to two RoIs per block (R >= 1024)
RS = (1, 2, 15, 16, 17, 33, 1023, 1024, 1025)
_CACHE = {}


def rnd(shape, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def relerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def pool_like_the_kernels(cells):
    """[R,49,256] fp32 cells (GPU) -> [R,256] fp32 (host): the summation order of the pooling kernels."""
    s = []
    for fg in range(4):
        acc = torch.zeros_like(cells[:, 0])
        for i in range(4):
            for r in range(4):
                c = 16 * i + 4 * fg + r
                if c < 49:
                    acc = acc + cells[:, c]
        s.append(acc)
    tot = ((s[0] + s[1]) + (s[2] + s[3])).cpu().numpy()
    return torch.from_numpy(tot / np.float32(49.0))


def reference(x32, w32, b):
    """(key16 form, split-precision form) of the pooled output for cell-major fp32 RoIs x32 [R,49,256], through the cell-writing conv."""
    from mv2d_amd import ops
    R = x32.shape[0]
    hi, lo = ops.f32_to_key16(x32, with_lo=True)
    out = []
    for lo_, w in ((None, ops.pack_key16(w32)), (lo, ops.pack_key16_x3(w32))):
        cells = torch.full((R, 49, 256), NAN, device=DEV)
        ops.qg_conv_cells(hi, lo_, w, b, out_f32=cells, R=R)
        out.append(pool_like_the_kernels(cells))
    return out


def run(x32, w32, b, form, R=None, ld=256):
    """One call of the pooled conv into a NaN buffer of R + 1 rows of ld columns."""
    from mv2d_amd import ops
    R = x32.shape[0] if R is None else R
    hi, lo = ops.f32_to_key16(x32, with_lo=True)
    out = torch.full((R + 1, ld), NAN, device=DEV)
    if form == 'key16':
        ops.qg_conv_pool(hi, ops.pack_key16(w32), b, out, R=R)
    else:
        ops.qg_conv_pool_x3(hi, lo, ops.pack_key16_x3(w32), b, out, R=R)
    torch.cuda.synchronize()
    return out.cpu()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def operands():
    """Inputs like test_qg_conv_pool_fused for the largest R and their reference: built once, shared by the cases, never written.  A RoI's
    result does not depend on R, so the first R rows serve every R."""
    if not _CACHE:
        R = max(RS)
        x = rnd((R, 256, 7, 7), 70).to(DEV)
        w = rnd((256, 256, 3, 3), 71, 0.03).to(DEV)
        x32 = x.permute(0, 2, 3, 1).reshape(R, 49, 256).contiguous()
        w32 = w.permute(0, 2, 3, 1).reshape(256, 2304).contiguous()
        b = rnd((256,), 72).to(DEV)
        ref = dict(zip(('key16', 'x3'), reference(x32, w32, b)))
        assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in ref.values())
        _CACHE.update(x32=x32, w32=w32, b=b, ref=ref)
    return _CACHE


@pytest.mark.parametrize('form', ['key16', 'x3'])
@pytest.mark.parametrize('R', RS)
def test_pooled_conv_is_bitwise_the_pooled_cells(R, form):
    op = operands()
    out = run(op['x32'][:R].contiguous(), op['w32'], op['b'], form)
    diff = (out[:R].view(torch.int32) != op['ref'][form][:R].view(torch.int32)).nonzero()
    print(f'[conv_cell48] R {R} {form}: {diff.shape[0]} of {R * 256} elements differ from the pooled cells' + (f', first (row, column) {diff[:8].tolist()}' if diff.shape[0] else ''))
    assert diff.shape[0] == 0
    assert bool(torch.isnan(out[R]).all()), 'nothing is stored past row R'


@pytest.mark.parametrize('form', ['key16', 'x3'])
def test_padded_output_keeps_its_padding(form):
    op = operands()
    R = 17
    out = run(op['x32'][:R].contiguous(), op['w32'], op['b'], form, ld=320)
    assert same_bits(out[:R, :256], op['ref'][form][:R])
    assert bool(torch.isnan(out[:R, 256:]).all()) and bool(torch.isnan(out[R]).all())


@pytest.mark.parametrize('form', ['key16', 'x3'])
def test_cell48_term_alone(form):
    """Only cell 48 and the centre tap are non-zero, the bias is 0: every other cell's conv is 0, so the pooled output is the cell-48 launch's
    term / 49."""
    from mv2d_amd import ops
    R = 33
    x48 = rnd((R, 256), 73)
    wc = rnd((256, 256), 74, 0.03)
    x32 = torch.zeros((R, 49, 256)); x32[:, 48] = x48
    w = torch.zeros((256, 3, 3, 256)); w[:, 1, 1] = wc
    x32, w32, b = x32.to(DEV), w.reshape(256, 2304).to(DEV), torch.zeros(256, device=DEV)
    out = run(x32, w32, b, form)[:R]
    ref = reference(x32, w32, b)[0 if form == 'key16' else 1]
    assert int((out > 0).sum()) > R * 64 and same_bits(out, ref)
    if form == 'key16':                                  # fp64 on the key16-rounded operands / on the unrounded ones
        x48, wc = ops.f32_to_key16(x48.to(DEV)).float().cpu(), ops.f32_to_key16(wc.to(DEV)).float().cpu()
    want = torch.relu(x48.double() @ wc.double().T) / 49.0
    e = relerr(out, want)
    print(f'[conv_cell48] cell-48 term alone, {form}: rel err against fp64 {e:.2e} (bound 1e-5)')
    assert e < 1e-5


@pytest.mark.parametrize('form', ['key16', 'x3'])
def test_nan_in_cell48_stays_in_its_roi(form):
    op = operands()
    R, bad = 33, 18
    x32 = op['x32'][:R].clone()
    x32[bad, 48, 5] = NAN
    out = run(x32, op['w32'], op['b'], form)[:R]
    assert bool(torch.isnan(out[bad]).all())
    keep = [r for r in range(R) if r != bad]
    assert bool(torch.isfinite(out[keep]).all()) and same_bits(out[keep], op['ref'][form][keep])
