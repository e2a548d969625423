"""The shape of the dynamic query generator (RH/utils/query_generator.py:20-67, 175-203, 281-331): which of the reference's config keys the
plugin module, the engine and the training route accept, and the parameter names and shapes that follow from them.

Accepted: ``num_shared_convs`` 0 .. 3 (256 -> 256, 3x3, padding 1, ReLU), ``num_shared_fcs`` 1 .. 3, ``num_center_fcs`` 0 .. 2 (Linear + ReLU of
``fc_out_channels``), ``fc_out_channels`` and every ``extra_encoding.feat_channels`` entry a multiple of 16 up to 4096 (a list, or one int repeated
``num_layers`` = 1 .. 3 times), ``extra_encoding.features`` either ``[]`` or the one 16-column ``intrinsic`` entry, ``with_avg_pool`` True or False
(False: the first shared fc reads the 256 * s * s flattened cells).  Everything else raises ``ValueError`` naming the key:

* ``num_shared_fcs = 0``: the reference cannot run it either (its ``torch.cat`` of the 4-D RoI tensor with the [R, 16] intrinsics fails);
* ``num_center_convs > 0``: a conv on the [R, C] encoding -- the reference's ConvModule needs a 4-D input there;
* ``with_cls / with_size / with_heading / with_attr`` and their ``num_*`` branch keys: the reference computes and discards their outputs;
* ``conv_out_channels != 256`` / ``in_channels != 256``: the RoI conv kernels are 256-channel kernels;
* a width that is no multiple of 16: the linears run on MFMA column tiles of 16.
"""
from collections import namedtuple

C = 256
MAX_WIDTH = 4096
INTRINSIC = dict(type='intrinsic', in_channels=16)

_Shape = namedtuple('QGShape', 'convs fcs center_fcs fc_out enc intrinsic pooled')


def pad32(n):
    return (int(n) + 31) // 32 * 32


class QGShape(_Shape):
    """convs / fcs / center_fcs: layer counts; fc_out: ``fc_out_channels``; enc: the widths of the extra-encoding layers; intrinsic: the 16
    intrinsics columns are concatenated; pooled: ``with_avg_pool``."""
    __slots__ = ()

    @property
    def is_default(self):
        return self == DEFAULT

    @property
    def enc_in(self):
        """Columns of the concatenated row the extra encoding reads (before the pad to a multiple of 32)."""
        return self.fc_out + (16 if self.intrinsic else 0)

    @property
    def center_in(self):
        """Columns fc_center reads."""
        return self.fc_out if self.center_fcs else self.enc[-1]

    def linears(self, roi_size):
        """[(parameter prefix, out features, in features, ReLU)] of every linear in execution order, fc_center last."""
        out, k = [], C if self.pooled else C * roi_size * roi_size
        for i in range(self.fcs):
            out.append((f'shared_fcs.{i}', self.fc_out, k, True))
            k = self.fc_out
        k = self.enc_in
        for i, n in enumerate(self.enc):
            out.append((f'extra_enc.{2 * i}', n, k, True))
            k = n
        for i in range(self.center_fcs):
            out.append((f'center_fcs.{i}', self.fc_out, k, True))
            k = self.fc_out
        out.append(('fc_center', 3, k, False))
        return out

    def param_shapes(self, roi_size=7):
        """{parameter name: shape} of the reference module built with this shape."""
        d = {}
        for i in range(self.convs):
            d[f'shared_convs.{i}.conv.weight'] = (C, C, 3, 3)
            d[f'shared_convs.{i}.conv.bias'] = (C,)
        for p, n, k, _ in self.linears(roi_size):
            d[p + '.weight'] = (n, k)
            d[p + '.bias'] = (n,)
        return d

    def check_state(self, sd, roi_size, who, prefix='query_generator.', shapes_only=False):
        """ValueError naming the first parameter of ``sd`` that is missing, whose shape is not the configured one, or that the configured shape does
        not have.  ``shapes_only``: only the shapes of the parameters that are present (missing and unexpected keys are left to the caller)."""
        want = self.param_shapes(roi_size)
        for k, shp in want.items():
            if prefix + k not in sd:
                if shapes_only:
                    continue
                raise ValueError(f'{who}: the state dict has no {prefix + k} (the configured query generator has one, {shp})')
            got = tuple(sd[prefix + k].shape)
            if got != tuple(shp):
                raise ValueError(f'{who}: {prefix + k} is {got} in the state dict, the configured query generator has {tuple(shp)}')
        if shapes_only:
            return
        extra = [k for k in sd if k.startswith(prefix) and k[len(prefix):] not in want]
        if extra:
            raise ValueError(f'{who}: the state dict holds {extra[0]}, which the configured query generator does not have')


DEFAULT = QGShape(convs=1, fcs=1, center_fcs=0, fc_out=1024, enc=(512, 256), intrinsic=True, pooled=True)
DEFAULT_EXTRA_ENCODING = dict(num_layers=2, feat_channels=[512, 256], features=[dict(INTRINSIC)])


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _int_in(v, lo, hi, key, who):
    if not _is_int(v) or not lo <= v <= hi:
        raise ValueError(f'{who}: {key} must be an int in [{lo}, {hi}], got {v!r}')
    return v


def _width(v, key, who):
    if not _is_int(v) or v % 16 or not 16 <= v <= MAX_WIDTH:
        raise ValueError(f'{who}: {key} must be a multiple of 16 in [16, {MAX_WIDTH}], got {v!r}')
    return v


def parse(cfg=None, who='QueryGenerator'):
    """QGShape of a reference ``query_generator=dict(...)`` (any subset of its keys; None: the shipped shape).  ValueError naming the key of
    the first setting that is not accepted."""
    if isinstance(cfg, QGShape):
        return cfg
    cfg = dict(cfg or {})
    if not cfg.get('with_center', True):
        raise ValueError(f'{who}: with_center must be True (fc_center is the generator\'s output)')
    for k in ('with_cls', 'with_size', 'with_heading', 'with_attr'):
        if cfg.get(k, False):
            raise ValueError(f'{who}: {k}=True is not supported (the reference discards that branch\'s output)')
    for k in sorted(cfg):
        if k.startswith('num_') and k not in ('num_shared_convs', 'num_shared_fcs', 'num_center_fcs', 'num_classes') and cfg[k] != 0:
            raise ValueError(f'{who}: {k} must be 0, got {cfg[k]!r}')
    for k in ('in_channels', 'conv_out_channels'):
        if cfg.get(k, C) != C:
            raise ValueError(f'{who}: {k} must be {C}, got {cfg[k]!r}')
    for k in ('conv_cfg', 'norm_cfg'):
        if cfg.get(k) is not None:
            raise ValueError(f'{who}: {k} must be None (plain Conv2d + ReLU), got {cfg[k]!r}')
    convs = _int_in(cfg.get('num_shared_convs', 1), 0, 3, 'num_shared_convs', who)
    fcs = _int_in(cfg.get('num_shared_fcs', 1), 1, 3, 'num_shared_fcs', who)
    center_fcs = _int_in(cfg.get('num_center_fcs', 0), 0, 2, 'num_center_fcs', who)
    fc_out = _width(cfg.get('fc_out_channels', 1024), 'fc_out_channels', who)
    ee = dict(cfg.get('extra_encoding', DEFAULT_EXTRA_ENCODING))
    if 'num_layers' not in ee:
        raise ValueError(f'{who}: extra_encoding.num_layers is missing')
    nl = _int_in(ee['num_layers'], 1, 3, 'extra_encoding.num_layers', who)
    fch = ee.get('feat_channels')
    if isinstance(fch, (list, tuple)):
        if len(fch) != nl:
            raise ValueError(f'{who}: extra_encoding.feat_channels has {len(fch)} entries, extra_encoding.num_layers = {nl}')
        fch = list(fch)
    else:
        fch = [fch] * nl
    if any(v is None for v in fch):
        raise ValueError(f'{who}: extra_encoding.feat_channels is missing')
    enc = tuple(_width(v, 'extra_encoding.feat_channels', who) for v in fch)
    feats = list(ee.get('features', []))
    if feats and not (len(feats) == 1 and dict(feats[0]) == INTRINSIC):
        raise ValueError(f'{who}: extra_encoding.features must be [] or [{INTRINSIC}], got {feats!r}')
    pooled = cfg.get('with_avg_pool', True)
    if not isinstance(pooled, bool):
        raise ValueError(f'{who}: with_avg_pool must be True or False, got {pooled!r}')
    return QGShape(convs, fcs, center_fcs, fc_out, enc, bool(feats), pooled)


def flatten_perm(roi_size, device=None):
    """Column permutation of the first shared fc under ``with_avg_pool=False``: the reference flattens [R, 256, s, s] to (channel, y, x) columns,
    the engine's rows are cell-major [R, s * s, 256].  ``W[:, flatten_perm(s)]`` are the weight columns in cell-major order, i.e.
    ``x.flatten(1) @ W.T == x.flatten(2).transpose(1, 2).flatten(1) @ W[:, perm].T``."""
    import torch
    s2 = roi_size * roi_size
    cell = torch.arange(s2, device=device)[:, None]
    ch = torch.arange(C, device=device)[None, :]
    return (ch * s2 + cell).reshape(-1)
