"""The fused split-precision FFN at widths whose slice count is no multiple of 8 (-m gpu): the ragged instance of csrc/ffn_x3.hip, whose last slab's
block accumulates the remaining hidden/64 - 8 slab slices.  Every slab equals the slab of the same operands zero-padded to a multiple of 512 hidden
units -- zero rows of W1, zeros in b1, zero columns of W2: the padded call runs the instance that existed before, and a padded slice contributes
exact zeros --, the slab sum is within the split-precision bound of tests/test_gpu_kernels.py::test_ffn_fused_x3_split_precision against fp64, and
nothing behind the last slab is written.

F: one slab of one slice | one slab of seven | a full slab and a slab of one | three full slabs and a slab of seven;
M: one row | two blocks of 32 rows, the second one a single row | 1025, the first row count that selects three row tiles per block."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F_

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 3e-5            # test_ffn_fused_x3_split_precision: of the output maximum, against fp64
SENTINEL = -12345.0
_OPS = {}


def rnd(shape, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def _operands(F):
    """Seeded operands of one width as in test_ffn_fused_x3_split_precision, their packed forms, the zero-padded packed forms and the fp64 weights:
    built once per width, shared by the row counts, never written."""
    if F not in _OPS:
        from mv2d_amd import ops
        Fp = 512 * -(-F // 512)
        W1, b1, W2 = rnd((F, 256), 28 + F, 0.1), rnd((F,), 29 + F), rnd((256, F), 30 + F, 0.05)
        W1p, b1p, W2p = torch.zeros(Fp, 256), torch.zeros(Fp), torch.zeros(256, Fp)
        W1p[:F], b1p[:F], W2p[:, :F] = W1, b1, W2
        _OPS[F] = dict(Fp=Fp, W1=W1.double(), b1=b1.double(), W2=W2.double(), b1d=b1.to(DEV), b1pd=b1p.to(DEV),
                       w1x=ops.pack_x3(W1.to(DEV)), w2x=ops.pack_x3(W2.to(DEV)), w1px=ops.pack_x3(W1p.to(DEV)), w2px=ops.pack_x3(W2p.to(DEV)))
    return _OPS[F]


@pytest.mark.parametrize('M', [1, 33, 1025])
@pytest.mark.parametrize('F', [64, 448, 576, 1984])
def test_ragged_ffn_equals_the_zero_padded_launch(F, M):
    from mv2d_amd import ops
    op = _operands(F)
    n = -(-F // 512)
    assert ops.ffn_slabs(F, 8) == n and (F // 64) % 8 != 0
    x = rnd((M, 256), 27 + M)
    xd = x.to(DEV)
    buf = torch.full((n + 1, M, 256), SENTINEL, device=DEV)
    got = ops.ffn_fused_x3(xd, op['w1x'], op['b1d'], op['w2x'], buf[:n], M, groups=8)
    assert got.shape == (n, M, 256)
    assert bool((buf[n] == SENTINEL).all()), 'the slab behind the output is untouched'
    assert tuple(ops.ffn_fused_x3(xd, op['w1x'], op['b1d'], op['w2x'], groups=8).shape) == (n, M, 256)
    # the same operands zero-padded to n full slabs: the existing instance, value for value
    pad = ops.ffn_fused_x3(xd, op['w1px'], op['b1pd'], op['w2px'], groups=8)
    assert pad.shape == (n, M, 256)
    assert torch.equal(got, pad)
    ref = F_.relu(x.double() @ op['W1'].T + op['b1']) @ op['W2'].T
    err = float((got.sum(0).double().cpu() - ref).abs().max() / ref.abs().max())
    print(f'[ffn ragged] F {F} M {M}: {n} slabs, slab sum against fp64 {err:.2e} of the maximum (bound {TOL:.0e})')
    assert err < TOL


def test_ragged_widths_need_eight_slices_per_block_and_exact_slabs():
    """1, 2 and 4 slices per block keep requiring divisibility (an argument error, no launch); a slab buffer of another slab count is refused."""
    from mv2d_amd import _lib, ops
    op = _operands(448)
    x = rnd((5, 256), 3).to(DEV)
    for G in (2, 4):
        with pytest.raises(_lib.Mv2dHipError, match='must divide hidden/64'):
            ops.ffn_fused_x3(x, op['w1x'], op['b1d'], op['w2x'], groups=G)
    assert ops.ffn_fused_x3(x, op['w1x'], op['b1d'], op['w2x'], groups=1).shape == (7, 5, 256)
    with pytest.raises(ValueError, match=r'slabs must be \[1, 5, 256\]'):
        ops.ffn_fused_x3(x, op['w1x'], op['b1d'], op['w2x'], torch.empty((2, 5, 256), device=DEV), 5, groups=8)
