"""Host policy of the per-rig cache of the PE's frustum MLP (route option ``pe_cache``; csrc/pe_x3_gate.hip).  Needs neither the library nor a GPU.

The table Q = position_encoder(frustum rows) + b1b is a function of the weights, the padding geometry and the camera matrices of one sample.  A rig
with fixed calibration repeats its matrices every frame; a stream with per-sample ego compensation in ``lidar2img`` never does.  So a table is
built only when a key is seen on two CONSECUTIVE frames (a stream whose matrices always change never builds one and never pays for one), one
table is kept, and any other key drops it (two rigs alternating through one engine stay on the full kernel).

The two-frame head (route option ``pe_cache_views``) keeps the table PER VIEW: the current-frame views of a vehicle with fixed calibration repeat their
matrices every frame, the previous-frame views carry the ego motion and never do.  ``PeViewCachePolicy`` runs one ``PeCachePolicy`` per view of a
sample; a frame gets the mask of the views whose slice of the table it reads (the gate-only kernel writes their rows, the full kernel the others)."""
import numpy as np


class PeCachePolicy:
    """observe(key) -> 'miss' | 'build' | 'hit' for the frames of one table, in order.  key: anything hashable and comparable (rig_key), or None for a
    frame that cannot use a table (a batch that mixes rigs).  'build': this frame's key equals the previous frame's and no table holds it -- the caller
    builds the table before the frame and the frame uses it; 'hit': the table holds this key; 'miss': the frame runs the full kernel, and a table of
    another key is no longer valid."""

    def __init__(self):
        self.prev = None        # the key of the previous frame (None: none, or unusable)
        self.held = None        # the key the table was built for
        self.builds = 0

    def observe(self, key):
        if key is None:
            self.prev = self.held = None
            return 'miss'
        if key == self.held:
            self.prev = key
            return 'hit'
        if key == self.prev:
            self.held = key
            self.builds += 1
            return 'build'
        self.prev, self.held = key, None
        return 'miss'


class PeViewCachePolicy:
    """observe(keys) -> (mask, build, state) for the frames of one per-view table, in order.  keys: one per view of a sample (view_keys), None for a
    view that cannot use the table.  Each view follows PeCachePolicy on its own key: its slice is built when the key is seen on two consecutive
    frames and dropped when the key changes.  mask: bit v set = this frame reads view v's slice (built now or held); build: the views whose slice the
    caller builds in front of the frame; state: 'miss' = mask 0, nothing built; 'build' = at least one slice built; 'hit' = mask != 0, nothing built."""

    def __init__(self, n_views):
        if not 1 <= n_views <= 32:
            raise ValueError(f'PeViewCachePolicy: 1 to 32 views per sample (one mask word), got {n_views}')
        self.views = [PeCachePolicy() for _ in range(n_views)]
        self.builds = 0         # frames that built at least one slice

    def observe(self, keys):
        if len(keys) != len(self.views):
            raise ValueError(f'PeViewCachePolicy: {len(keys)} keys for {len(self.views)} views')
        states = [pol.observe(k) for pol, k in zip(self.views, keys)]
        mask = sum(1 << v for v, s in enumerate(states) if s != 'miss')
        build = tuple(v for v, s in enumerate(states) if s == 'build')
        self.builds += bool(build)
        return mask, build, 'build' if build else 'hit' if mask else 'miss'


def mask_views(mask):
    """The view indices of a mask word, ascending."""
    return tuple(v for v in range(32) if (mask >> v) & 1)


def view_keys(weights_version, shape_key, mats, n_samples):
    """One key per view of a sample: (weights version, padding geometry, the bytes of the view's three matrices), or None for a view in which the
    samples of the batch carry different matrices; all None when the samples do not share one padding geometry.  shape_key: one entry per sample;
    mats: the stacked matrices [kinds, n_samples * views, ...] of HeadEngine._host_prepare."""
    mats = np.asarray(mats)
    views = mats.shape[1] // n_samples
    if any(k != shape_key[0] for k in shape_key[1:]):
        return [None] * views
    m = np.ascontiguousarray(mats.reshape(mats.shape[0], n_samples, views, -1).transpose(2, 1, 0, 3))        # [view, sample, kind, 16]
    return [(weights_version, shape_key[0], m[v, 0].tobytes()) if bool((m[v, 1:] == m[v, :1]).all()) else None for v in range(views)]


def one_rig(mats, n_samples):
    """Do the samples of a batch share their camera matrices?  mats: the stacked matrices [kinds, n_samples * views, ...] as
    HeadEngine._host_prepare compares them from frame to frame."""
    if n_samples == 1:
        return True
    m = np.asarray(mats).reshape(mats.shape[0], n_samples, -1)
    return bool((m[:, 1:] == m[:, :1]).all())


def rig_key(weights_version, shape_key, mats_gen, shared_rig=True):
    """The key of one batch, or None when its samples do not share one rig.  shape_key: one entry per sample (the padding geometry); mats_gen: a
    counter the engine bumps whenever the camera matrices differ from the previous frame's (it compares them anyway, to rebuild its tables), so a
    frame whose matrices moved costs no second look at them; shared_rig: one_rig() of the matrices -- the engine asks only when the matrices
    repeat, on a frame whose matrices changed it passes True (that frame is a miss whatever the answer is)."""
    if not shared_rig or any(k != shape_key[0] for k in shape_key[1:]):
        return None
    return (weights_version, shape_key[0], mats_gen)
