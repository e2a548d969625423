"""The map-format (fp32 / fp16 / bf16 feature map) interface without a GPU: the *_fmt entries are declared in include/mv2d_hip.h, listed in
_lib.SIGNATURES and exported by the built library; the format constants agree between csrc/common.h, the header's text and ops.MAP_FMT; the
entries refuse an unknown format through the return code; the ops wrappers refuse a map whose dtype disagrees with a stated format, and any
dtype beyond the three."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT_ENTRIES = ['mv2d_nchw_to_nhwc_fmt', 'mv2d_nchw_to_nhwc_masked_fmt', 'mv2d_roi_align_fmt', 'mv2d_pe_inputs_fmt', 'mv2d_pe_fused_x3_fmt',
               'mv2d_pe_fused_tab_fmt']


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from mv2d_amd import _lib
    return _lib.load()


def test_fmt_entries_declared_listed_and_exported(lib):
    from mv2d_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mv2d_hip.h')).read(), flags=re.S)
    for n in FMT_ENTRIES:
        decl = re.search(r'\bint\s+' + n + r'\s*\(([^;]*)\)\s*;', hdr)
        assert decl is not None, f'{n} is not declared in include/mv2d_hip.h'
        args = [a.strip() for a in decl.group(1).split(',')]
        assert args[-1] == 'void* stream' and args[-2] == 'int map_fmt', (n, args[-2:])       # the format sits in front of the stream
        assert n in _lib.SIGNATURES and len(_lib.SIGNATURES[n][1]) == len(args), n
        assert hasattr(lib, n), f'{n} is not exported by the built library'
        # the entry it extends keeps its place: same arguments minus the format
        base = {'mv2d_roi_align_fmt': 'mv2d_roi_align_s', 'mv2d_pe_fused_tab_fmt': 'mv2d_pe_fused_tab2'}.get(n, n[:-4])
        assert len(_lib.SIGNATURES[base][1]) == len(args) - 1, (n, base)
    assert lib.mv2d_abi_version() == 6 and _lib.ABI_VERSION == 6


def test_format_constants_agree():
    from mv2d_amd import ops
    src = open(os.path.join(ROOT, 'mv2d_amd', 'csrc', 'common.h')).read()
    c = {k: int(v) for k, v in re.findall(r'#define\s+MV2D_MAP_(F32|F16|BF16)\s+(\d+)', src)}
    assert c == {'F32': 0, 'F16': 1, 'BF16': 2}
    assert ops.MAP_FMT == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    assert [ops.map_format(d) for d in (torch.float32, torch.float16, torch.bfloat16)] == [0, 1, 2]
    hdr = open(os.path.join(ROOT, 'include', 'mv2d_hip.h')).read()
    assert re.search(r'map_fmt 0 = fp32, 1 = (IEEE )?fp16, 2 = bf16', hdr)
    for bad in (torch.float64, torch.int32, torch.uint8, torch.float8_e4m3fn):
        with pytest.raises(ValueError, match='float32.*float16.*bfloat16'):
            ops.map_format(bad)


def test_entries_refuse_an_unknown_format(lib):
    x = torch.zeros(64, dtype=torch.float32)                     # (validation only: nothing is launched, nothing is dereferenced)
    p = x.data_ptr()
    for fmt in (-1, 3):
        assert lib.mv2d_nchw_to_nhwc_fmt(p, p, 1, 4, 4, fmt, None) == -1 and b'map_fmt' in lib.mv2d_last_error()
        assert lib.mv2d_nchw_to_nhwc_masked_fmt(p, p, p, 1, 4, 4, fmt, None) == -1 and b'map_fmt' in lib.mv2d_last_error()
        assert lib.mv2d_roi_align_fmt(p, None, p, p, None, None, None, 1, 4, 4, 256, 0.0625, -1, None, 0, None, None, None, None, None, 7, fmt,
                                      None) == -1 and b'map_fmt' in lib.mv2d_last_error()
        assert lib.mv2d_pe_inputs_fmt(p, p, 1, p, p, p, p, p, p, p, p, p, p, None, None, None, 1, 2, 2, 64, p, fmt, None) == -1
        assert b'map_fmt' in lib.mv2d_last_error()
        assert lib.mv2d_pe_fused_tab_fmt(*([p, p, p, None, None, 1] + [p] * 9 + [1, p, p, 1, fmt, None])) == -1 and b'map_fmt' in lib.mv2d_last_error()
        assert lib.mv2d_pe_fused_x3_fmt(*([p, p, None, None, 1] + [p] * 13 + [1] + [p, None, None, None, None] + [0, 0, None, fmt, None])) == -1
        assert b'map_fmt' in lib.mv2d_last_error()
    # the masked 16-bit form keeps the alignment rule of the fp32 one: HW and C multiples of 4
    assert lib.mv2d_nchw_to_nhwc_masked_fmt(p, p, p, 1, 4, 6, 1, None) == -1 and b'multiples of 4' in lib.mv2d_last_error()
    assert lib.mv2d_nchw_to_nhwc_masked_fmt(p, p, p, 1, 4, 6, 0, None) == -1 and b'multiples of 4' in lib.mv2d_last_error()


def test_ops_wrappers_refuse_a_dtype_that_disagrees_with_the_format(lib):
    from mv2d_amd import _lib, ops
    half, single = torch.zeros((8, 256), dtype=torch.float16), torch.zeros((8, 256), dtype=torch.float32)
    r = torch.zeros((1, 5))
    cases = [lambda m, f: ops.nchw_to_nhwc(m.view(1, 8, 16, 16), map_fmt=f),
             lambda m, f: ops.roi_align(m, r, 2, 4, out0_f32=torch.zeros((1, 49, 256)), map_fmt=f),
             lambda m, f: ops.pe_inputs(None, None, 0, m, *([None] * 6), None, None, None, None, 1, 2, 4, 64, None, map_fmt=f),
             lambda m, f: ops.pe_fused_x3(None, m, None, {}, None, 1, map_fmt=f),
             lambda m, f: ops.pe_fused_tab(None, None, m, None, {}, None, 1, None, None, map_fmt=f)]
    for call in cases:
        for m, f in ((half, 0), (half, 2), (single, 1), (half.to(torch.bfloat16), 1)):
            with pytest.raises(_lib.Mv2dHipError, match='map_fmt'):
                call(m, f)
        with pytest.raises(ValueError, match='float32.*float16.*bfloat16'):
            call(single.double(), None)
    # a map of an accepted dtype on the host is still refused: no CPU path
    with pytest.raises(_lib.Mv2dHipError, match='GPU'):
        ops.nchw_to_nhwc(half.view(1, 8, 16, 16))


def test_native_map_keeps_the_three_dtypes():
    from mv2d_amd.engine import native_map
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        x = torch.zeros((1, 4, 2, 2), dtype=dt)
        assert native_map(x) is x
    assert native_map(torch.zeros(2, dtype=torch.float64)).dtype == torch.float32
