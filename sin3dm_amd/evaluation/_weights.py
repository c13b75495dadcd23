"""What the evaluation networks (ssfid.VoxelClassifier, sifid.ImageFeatureNet) share: weights by name out of a state dict, and the
plumbing of a device handle that takes them."""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib


def check_weights(state, shapes, what, hint=""):
    """The tensors of `shapes` out of a state dict as contiguous float32 on the host; every other key is ignored.  KeyError names a
    missing key, ValueError a wrong shape (`hint` is appended to it)."""
    out = {}
    for name, shape in shapes.items():
        if name not in state:
            raise KeyError(f"{what} weights: key '{name}' is missing")
        t = torch.as_tensor(state[name]).detach().to("cpu", torch.float32).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"{what} weights: '{name}' has shape {tuple(t.shape)}, expected {shape}{hint}")
        out[name] = t
    return out


def load_state(weights):
    """A state dict from a path (torch.load) or a mapping."""
    if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
        state = torch.load(weights, map_location="cpu")
        if not hasattr(state, "keys"):
            raise ValueError(f"{weights}: a state dict is expected, got {type(state).__name__}")
        return state
    return weights


class FeatureHandle:
    """A handle of the library's s3d_<PREFIX>_* entry points: create(*CREATE_ARGS), parameters by name, STAGES timed stages."""
    PREFIX = None
    CREATE_ARGS = ()
    STAGES = 0
    SHAPES = None
    WHAT = None
    HINT = ""

    def __init__(self, weights=None):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        _lib.check(self._call("create", *self.CREATE_ARGS, C.byref(self._h)))
        if weights is not None:
            self.load_weights(weights)

    def _call(self, name, *args):
        return getattr(self._lib, f"s3d_{self.PREFIX}_{name}")(*args)

    def load_weights(self, weights, shapes=None, what=None):
        for name, t in check_weights(load_state(weights), shapes or self.SHAPES, what or self.WHAT, self.HINT if shapes is None else "").items():
            shape = (C.c_int64 * t.dim())(*t.shape)
            _lib.check(self._call("set_param", self._h, name.encode(), C.c_void_p(t.data_ptr()), shape, t.dim()))

    def close(self):
        if getattr(self, "_h", None):
            self._call("destroy", self._h)
            self._h = None

    __del__ = close

    def profile(self, on=True):
        _lib.check(self._call("profile", self._h, int(bool(on))))

    def stage_ms(self):
        ms = (C.c_double * self.STAGES)()
        _lib.check(self._call("profile_read", self._h, ms))
        return tuple(ms)
