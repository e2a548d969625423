"""Host policy of the per-rig cache of the PE's frustum MLP (route option ``pe_cache``; csrc/pe_x3_gate.hip).  Needs neither the library nor a GPU.

The table Q = position_encoder(frustum rows) + b1b is a function of the weights, the padding geometry and the camera matrices of one sample.  A rig
with fixed calibration repeats its matrices every frame; a stream with per-sample ego compensation in ``lidar2img`` never does.  So a table is
built only when a key is seen on two CONSECUTIVE frames (a stream whose matrices always change never builds one and never pays for one), one
table is kept, and any other key drops it (two rigs alternating through one engine stay on the full kernel)."""
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
