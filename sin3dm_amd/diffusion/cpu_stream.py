"""torch's CPU noise stream, generated on the MI355X.

The reference samples on the CPU: x_T is one `th.randn(*shape)` and every step draws one `th.randn_like(x)`
(src/diffusion/gaussian_diffusion.py:514, 431, 591; src/sample.py:38), all from torch's default CPU generator.  A
`TorchCpuStream` is that generator with its 624 state words on the device: `randn` / `rand` return device tensors holding
the values `torch.randn` / `torch.rand` would have drawn on the CPU (s3d_rng.hip; the stream is defined in DESIGN.md §14).
Pass one wherever the sampling loops take `generator=`:

    diffusion.p_sample_loop(model, shape, model_kwargs=kw, generator=TorchCpuStream(seed))

gives the sample the reference gives after `torch.manual_seed(seed)` (to the trajectory tolerance of README.md "Parity").
Only float32 and calls of at least 16 elements (torch draws fewer through another, double-precision path).
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import torch as th

from .. import _lib

MT_N = 624
_STATE_BYTES = 5056                       # torch.get_rng_state() of the CPU generator (mt19937 engine, legacy layout)
_HEAD = "<QiiQ"                           # seed, left, seeded, next; then 624 x uint64 state words (low 32 bits used)
_KEY_OFF = struct.calcsize(_HEAD)


def init_genrand(seed):
    """(624 state words, position) after `torch.manual_seed(seed)`: MT19937's init_genrand of the low 32 bits; the generator
    regenerates before its first output (position 624)."""
    key = np.empty(MT_N, dtype=np.uint32)
    x = int(seed) & 0xFFFFFFFF
    key[0] = x
    for j in range(1, MT_N):
        x = (1812433253 * (x ^ (x >> 30)) + j) & 0xFFFFFFFF
        key[j] = x
    return key, MT_N


def parse_rng_state(state):
    """(624 state words, position 0..624, seed field) of a `torch.get_rng_state()` tensor.  `left` counts the words until the
    next regeneration (+1), so position = 625 - left also for a freshly seeded generator (left = 1, next = 0)."""
    raw = state.numpy().tobytes()
    if len(raw) != _STATE_BYTES:
        raise ValueError(f"torch CPU generator state of {len(raw)} bytes: expected the {_STATE_BYTES}-byte mt19937 layout")
    seed, left, seeded, _ = struct.unpack_from(_HEAD, raw, 0)
    if not seeded or not 1 <= left <= MT_N + 1:
        raise ValueError(f"torch CPU generator state: seeded={seeded} left={left}")
    key = np.frombuffer(raw, dtype="<u8", count=MT_N, offset=_KEY_OFF).astype(np.uint32)
    return key, MT_N + 1 - left, seed


def pack_rng_state(key, pos, seed=0, template=None):
    """The `torch.set_rng_state` tensor for (state words, position); the normal-distribution caches (unused by float32 draws)
    are taken from `template` (a get_rng_state tensor) or cleared."""
    b = bytearray(template.numpy().tobytes() if template is not None else bytes(_STATE_BYTES))
    struct.pack_into(_HEAD, b, 0, int(seed) & 0xFFFFFFFFFFFFFFFF, MT_N + 1 - int(pos), 1, int(pos))
    b[_KEY_OFF:_KEY_OFF + MT_N * 8] = np.asarray(key, dtype=np.uint32).astype("<u8").tobytes()
    return th.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy())


def words_per_call(numel):
    """32-bit words one float32 `torch.randn(numel)` call consumes (numel >= 16)."""
    return int(numel) + (16 if numel % 16 else 0)


_SIDE = {}


def side_stream(device):
    """The stream the sampling loops draw ahead on (one per device and process)."""
    dev = th.device(device)
    dev = th.device("cuda", th.cuda.current_device()) if dev.index is None else dev
    s = _SIDE.get(str(dev))
    if s is None:
        s = _SIDE[str(dev)] = th.cuda.Stream(device=dev)
    return s


class TorchCpuStream:
    """seed=k: the stream after `torch.manual_seed(k)`; seed=None: adopts the current state of torch's default CPU generator
    (torch's own generator is left where it is: `sync_to_torch` moves it).  Nothing touches the device before the first draw."""

    def __init__(self, seed=None, device=None):
        self.device = None if device is None else th.device(device)
        self._handle = None
        self._reserved = 0
        self._last = None                         # (stream id, event) of the latest launch: a draw on another stream waits for it
        if seed is None:
            self._key, self._pos, self._seed = parse_rng_state(th.get_rng_state())
            self._dirty = True
        else:
            self.manual_seed(seed)

    def manual_seed(self, seed):
        self._key, self._pos = init_genrand(seed)
        self._seed = int(seed)
        self._dirty = True
        return self

    def initial_seed(self):
        return self._seed

    # ------------------------------------------------------------------ device side
    def _ready(self, device=None):
        """The handle, with the host words uploaded, ordered on the current stream of self.device (unset: `device`, or the
        current device, from the first draw on)."""
        _lib.require_gpu()
        if self.device is None and device is not None:
            self.device = th.device(device)
        if self.device is None or self.device.index is None:
            self.device = th.device("cuda", th.cuda.current_device())
        lib = _lib.load()
        if self._handle is None:
            h = C.c_void_p()
            with th.cuda.device(self.device):
                _lib.check(lib.s3d_rng_create(C.byref(h)))
            self._handle = h
        stream = th.cuda.current_stream(self.device)
        if self._last is not None and self._last[0] != stream.cuda_stream:
            stream.wait_event(self._last[1])
        if self._dirty:
            key = np.ascontiguousarray(self._key, dtype=np.uint32)
            with th.cuda.device(self.device):
                _lib.check(lib.s3d_rng_set_state(self._handle, key.ctypes.data_as(C.POINTER(C.c_uint32)), int(self._pos),
                                                 C.c_void_p(stream.cuda_stream)))
            self._dirty = False
        return lib, stream

    def _done(self, stream):
        ev = th.cuda.Event()
        ev.record(stream)
        self._last = (stream.cuda_stream, ev)

    def _reserve(self, lib, words):
        if words > self._reserved:
            with th.cuda.device(self.device):
                _lib.check(lib.s3d_rng_reserve(self._handle, int(words)))
            self._reserved = int(words)

    def randn(self, shape, lead=None, device=None):
        """`torch.randn(shape)` of the stream as a device tensor; lead=k: k consecutive such calls, [k, *shape]."""
        shape = tuple(int(d) for d in shape)
        numel = int(np.prod(shape, dtype=np.int64))
        k = 1 if lead is None else int(lead)
        if numel < 16:
            raise NotImplementedError(f"TorchCpuStream.randn of {numel} elements: torch draws fewer than 16 through a "
                                      "double-precision path that is not implemented")
        lib, stream = self._ready(device)
        out = th.empty((() if lead is None else (k,)) + shape, device=self.device, dtype=th.float32)
        self._reserve(lib, words_per_call(numel) * k)
        with th.cuda.device(self.device):
            _lib.check(lib.s3d_rng_randn(self._handle, _lib.ptr(out), numel, k, C.c_void_p(stream.cuda_stream)))
        self._done(stream)
        return out

    def rand(self, shape, device=None):
        """`torch.rand(shape)` of the stream as a device tensor (bit-equal)."""
        shape = tuple(int(d) for d in shape) if not isinstance(shape, int) else (int(shape),)
        numel = int(np.prod(shape, dtype=np.int64))
        lib, stream = self._ready(device)
        out = th.empty(shape, device=self.device, dtype=th.float32)
        self._reserve(lib, numel)
        with th.cuda.device(self.device):
            _lib.check(lib.s3d_rng_rand(self._handle, _lib.ptr(out), numel, C.c_void_p(stream.cuda_stream)))
        self._done(stream)
        return out

    def get_state(self):
        """(624 state words, position) now; waits for the draws in flight."""
        if self._handle is None or self._dirty:
            return np.array(self._key, dtype=np.uint32), int(self._pos)
        lib, stream = self._ready()
        key = np.empty(MT_N, dtype=np.uint32)
        pos = C.c_int(0)
        with th.cuda.device(self.device):
            _lib.check(lib.s3d_rng_get_state(self._handle, key.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(pos),
                                             C.c_void_p(stream.cuda_stream)))
        return key, int(pos.value)

    def sync_to_torch(self):
        """Move torch's default CPU generator to where this stream stands, so that host code drawing afterwards continues
        the sequence as it would after the reference's run."""
        key, pos = self.get_state()
        th.set_rng_state(pack_rng_state(key, pos, self._seed, template=th.get_rng_state()))

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h is not None:
            try:
                _lib.load().s3d_rng_destroy(h)
            except Exception:
                pass


def is_cpu_stream(generator):
    """True for a TorchCpuStream or a non-empty sequence of them (one per batch element)."""
    if isinstance(generator, TorchCpuStream):
        return True
    return (isinstance(generator, (list, tuple)) and len(generator) > 0
            and all(isinstance(g, TorchCpuStream) for g in generator))
