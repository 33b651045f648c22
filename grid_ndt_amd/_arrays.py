"""Where a call's arrays live: numpy for libgndt's host entry points, torch on a device and a stream for the *_device ones.

A map consumer (map2d.TwoDmap.walk_paths, view_gain, ...) is written once against one of the two backends below.  A backend offers only
what those bodies share — allocation, a pointer-or-NULL, "bring this optional input here", a record's fields, the array module (xp) —
and knows no consumer:
what the two entry points of a consumer really take differently is an `if be.on_dev` in that consumer.
"""
import contextlib
import ctypes as C

import numpy as np

from ._lib import _record_decoder, record_fields, record_is_wide

_HIP_STREAM_LEGACY = 1      # hipStreamLegacy ((hipStream_t)1): the null stream by its explicit name
_NO_CTX = contextlib.nullcontext()      # (stateless: one serves every `with`)


def _stream_ptr(stream):
    """libgndt takes NULL as "the handle's own (non-blocking) stream".  torch's default stream IS the null stream
    (cuda_stream == 0), and work the caller enqueues there — filling the input buffer, say — is not ordered with a
    non-blocking stream: the null stream is therefore passed by its explicit name, hipStreamLegacy."""
    if stream is None:
        try:
            import torch
            if torch.cuda.is_available():
                return C.c_void_p(torch.cuda.current_stream().cuda_stream or _HIP_STREAM_LEGACY)
        except ImportError:
            pass
        return C.c_void_p(0)
    if hasattr(stream, "cuda_stream"):
        return C.c_void_p(stream.cuda_stream or _HIP_STREAM_LEGACY)
    return C.c_void_p(int(stream))


def _torch_stream_ctx(stream):
    """torch's current stream := `stream` while tensors that the call's kernels read or write are made, so that the caching allocator
    ties them to the stream the kernels run on.  A raw hipStream_t is wrapped (torch.cuda.ExternalStream); None: torch's current one."""
    if stream is None:
        return _NO_CTX
    import torch
    if not hasattr(stream, "cuda_stream"):
        stream = torch.cuda.ExternalStream(int(stream))
    return torch.cuda.stream(stream)


def _stream_wait(stream):
    """wait for what was enqueued on `stream` (a torch stream or a raw hipStream_t; None: nothing to wait for here)"""
    if hasattr(stream, "synchronize"):
        stream.synchronize()
    elif stream is not None:
        import torch
        torch.cuda.ExternalStream(int(stream)).synchronize()


class HostArrays:
    """numpy arrays; gndt_X"""
    on_dev = False
    stream = None
    xp = np
    empty, zeros, full = staticmethod(np.empty), staticmethod(np.zeros), staticmethod(np.full)

    @staticmethod
    def ctx():
        return _NO_CTX

    @staticmethod
    def addr(a):
        return C.c_void_p(a.ctypes.data)

    @staticmethod
    def ptr(a):
        """NULL for None and for an array without elements"""
        return C.c_void_p(a.ctypes.data if a is not None and a.size else 0)

    @staticmethod
    def here(a, dtype):
        """an optional input as a contiguous numpy array of `dtype`: integers of its width are taken as they are (uint32 hops are
        int32 hops), anything else is converted"""
        if a is None or (type(a) is np.ndarray and a.dtype == dtype and a.flags.c_contiguous):
            return a
        a = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)
        dtype = np.dtype(dtype)
        same_bits = a.dtype.kind in "iu" and dtype.kind in "iu" and a.dtype.itemsize == dtype.itemsize
        return a.view(dtype) if same_bits else a.astype(dtype, copy=False)

    @staticmethod
    def records(K, dtype, zeroed=True):
        """room for K records of `dtype`; zeroed=False where the call writes every record it is given"""
        return (np.zeros if zeroed else np.empty)(K, dtype)

    @staticmethod
    def fields(raw, dtype, host_as=None):
        """{field: view} of an array of records but `reserved`; host_as: {field: the dtype of the same width it is handed out as}"""
        out = {k: raw[k] for k in record_fields(dtype)}
        if host_as:
            for k, dt in host_as.items():
                out[k] = out[k].view(dt)
        return out


class DeviceArrays:
    """torch tensors on `device` (a torch.device), made under `stream` (ctx()); gndt_X_device with the stream behind its arguments.  Unsigned 32-bit
    is int32 here and unsigned 64-bit int64: the bits are the library's."""
    __slots__ = ("device", "stream")
    on_dev = True
    xp = _DTYPES = None         # torch and {numpy type: torch dtype}, from the first instance on (torch is imported only when it is used)

    def __init__(self, device, stream):
        if DeviceArrays.xp is None:
            import torch
            DeviceArrays._DTYPES = {np.int32: torch.int32, np.uint32: torch.int32, np.float32: torch.float32, np.uint8: torch.uint8,
                                    np.int64: torch.int64, np.float64: torch.float64}
            DeviceArrays.xp = torch
        self.device, self.stream = device, stream

    def ctx(self):
        return _torch_stream_ctx(self.stream)

    def empty(self, shape, dtype):
        return self.xp.empty(shape, dtype=self._DTYPES[dtype], device=self.device)

    def zeros(self, shape, dtype):
        return self.xp.zeros(shape, dtype=self._DTYPES[dtype], device=self.device)

    def full(self, shape, value, dtype):
        return self.xp.full(shape, value, dtype=self._DTYPES[dtype], device=self.device)

    @staticmethod
    def addr(t):
        return C.c_void_p(t.data_ptr())

    @staticmethod
    def ptr(t):
        """NULL for None and for a tensor without elements"""
        return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)

    def here(self, a, dtype):
        """an optional input as a contiguous tensor of `dtype` on the device (call it under ctx(): it may copy)"""
        want = self._DTYPES[dtype]
        if type(a) is self.xp.Tensor:
            if a.dtype == want and a.device == self.device:     # (the common case: it is here already)
                return a if a.is_contiguous() else a.contiguous()
        elif a is None:
            return None
        elif isinstance(a, np.ndarray):
            if not a.flags.c_contiguous:
                a = np.ascontiguousarray(a)
            if a.dtype == np.uint32:
                a = a.view(np.int32)
        t = self.xp.as_tensor(a, device=self.device)
        if t.dtype != want:
            t = t.to(want)
        return t.contiguous()

    def records(self, K, dtype, zeroed=True):
        """room for K records of `dtype`, which fields() takes apart: a [K, words] int32 tensor, int64 for a record of 8-byte fields;
        zeroed=False where the call writes every record it is given"""
        word = 8 if record_is_wide(dtype) else 4
        return (self.xp.zeros if zeroed else self.xp.empty)((K, dtype.itemsize // word), dtype=self._DTYPES[np.int64 if word == 8 else np.int32],
                                                            device=self.device)

    @staticmethod
    def fields(raw, dtype, host_as=None):
        """_lib.record_views: int32 / int64 whatever the sign, so host_as has nothing to say here"""
        return _record_decoder(dtype)(raw)
