"""What the GPU tests share: arrays onto the device and back, a handle and a built map, the C arguments every consumer takes, a debug
option for a block, and the padded call — a C entry point called through its host twin or its device twin on outputs that lie between
sentinels, so that a write before the rows or behind them shows.  Torch is imported where it is used: collecting the tests needs no GPU."""
import contextlib
import ctypes as C

import numpy as np

WORD_FILL = 0x5A5A5A5A
BYTE_FILL = 0x5A


def dev(a, dtype=np.float32, copy=False):
    """a numpy array on the device; copy: of an array that is read-only (the shared clouds)"""
    import torch
    return torch.from_numpy(np.array(a, dtype) if copy else np.ascontiguousarray(a, dtype)).cuda()


def to_np(t):
    """a tensor or an array as numpy; a dict of them value by value"""
    if isinstance(t, dict):
        return {k: to_np(v) for k, v in t.items()}
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def handle(P, strategy=0, **kw):
    """a fresh handle with the cells and the interval of P"""
    import grid_ndt_amd as g
    m = g.TwoDmap(P["grid_len"], P["z_len"], strategy=strategy, **kw)
    m.setInterval(P["slope_interval"])
    return m


def build(cloud, P, strategy=0, demand=None, whole=False):
    """the map of a cloud (row 0 its origin) on a fresh handle, built and synchronised; whole: every column of the points as it is"""
    m = handle(P, strategy)
    m.setCloudFirst(cloud[0])
    m.create2DMap(P.get("demand", "slope") if demand is None else demand, dev(cloud[1:], cloud.dtype) if whole else dev(cloud[1:, :3]))
    m.sync()
    return m


def robot_arg(robot, base):
    """gndt_robot* of `base` with the fields of `robot` over it; None stays None (the library's default robot)"""
    from grid_ndt_amd._lib import Robot
    if robot is None:
        return None
    d = dict(base)
    d.update(robot)
    return C.byref(Robot(d["radius"], d["reachable_height"], d["max_rough"], d["max_angle_deg"]))


def stream_arg(stream):
    """hipStream_t of a torch stream, None the null stream; a stream whose handle reads 0 is the legacy stream, passed as 1"""
    return C.c_void_p(0 if stream is None else (stream.cuda_stream or 1))


@contextlib.contextmanager
def debug_option(option, value, restore):
    """gndt_debug_set_option(option, value) for a block; `restore` comes back whatever happens in it"""
    import grid_ndt_amd as g
    g.TwoDmap.set_debug_option(getattr(g.TwoDmap, option), value)
    try:
        yield
    finally:
        g.TwoDmap.set_debug_option(getattr(g.TwoDmap, option), restore)


# ---- the padded call --------------------------------------------------------------------------------------------------------------------

class Padded:
    """An output the library must fill exactly: `items` items of `words` elements of dtype each, `front` items of fill before them
    and `back` behind.  .a is the whole buffer, .body the items; the library is handed the address of the body."""

    def __init__(self, items, dtype=np.uint32, words=1, front=0, back=0, fill=None):
        dtype = np.dtype(dtype)
        self.fill = (BYTE_FILL if dtype.itemsize == 1 else WORD_FILL) if fill is None else fill
        self.items, self.words, self.front = items, words, front
        self.a = np.full((front + items + back) * words, self.fill, dtype)

    @classmethod
    def over(cls, a, words=1, front=0, fill=None):
        """the layout laid over a buffer that a call has filled"""
        p = cls(0, a.dtype, words, fill=fill)
        p.a, p.front, p.items = a, front, a.size // words - front
        return p

    @property
    def offset(self):
        return self.front * self.words * self.a.itemsize

    @property
    def body(self):
        return self.a[self.front * self.words:(self.front + self.items) * self.words]

    @property
    def tail(self):
        return self.a[(self.front + self.items) * self.words:]

    def untouched(self, written=None):
        """the fill still stands before the items and behind the first `written` of them (None: all of them)"""
        w = self.items if written is None else written
        return bool((self.a[:self.front * self.words] == self.fill).all() and (self.a[(self.front + w) * self.words:] == self.fill).all())


def tails_untouched(got):
    """of a result with "tails" (what lay behind the rows of each output): every tail still holds its dtype's fill"""
    return all((t == (BYTE_FILL if t.dtype.itemsize == 1 else WORD_FILL)).all() for t in got["tails"].values())


class at:
    """an argument of a padded call: the address `offset` bytes into a buffer"""

    def __init__(self, buf, offset):
        self.buf, self.offset = buf, offset


class PaddedCall:
    """call(host_fn, device_fn, *args): the C entry point's host twin on numpy memory (host=True) or its device twin on uploads.
    An argument that is a numpy array is an input, a Padded an output (or an input to read back), at(...) either of them at a byte
    offset; each becomes a pointer — None for an empty input, and for a None.  Everything else is passed as it is.  The device
    twin gets the stream argument appended; the call is synchronised and every Padded read back into its own numpy array.
    wait_for_current: the side stream waits for the uploads, which the current stream made."""

    def __init__(self, host=False, stream=None, wait_for_current=False):
        self.host, self.stream, self.wait_for_current = host, stream, wait_for_current

    def __call__(self, host_fn, device_fn, *args):
        if self.host:
            return host_fn(*[self._pointer(a, lambda arr: arr.ctypes.data) for a in args])
        import torch
        up = {}                                     # id of a numpy array -> (the array, its upload): an array passed twice is one upload

        def address(arr):
            if id(arr) not in up:
                up[id(arr)] = (arr, torch.from_numpy(arr.reshape(-1).view(np.uint8)).cuda())
            return up[id(arr)][1].data_ptr()

        ptrs = [self._pointer(a, address) for a in args]
        if self.wait_for_current and self.stream is not None:
            self.stream.wait_stream(torch.cuda.current_stream())
        rc = device_fn(*ptrs, stream_arg(self.stream))
        torch.cuda.synchronize()
        for a in args:
            a = a.buf if isinstance(a, at) else a
            if isinstance(a, Padded) and id(a.a) in up:
                a.a.view(np.uint8)[:] = up.pop(id(a.a))[1].cpu().numpy()
        return rc

    @staticmethod
    def _pointer(a, address):
        off = 0
        if isinstance(a, at):
            a, off = a.buf, a.offset
        if isinstance(a, Padded):
            a, off = a.a, off + a.offset
        if not isinstance(a, np.ndarray):
            return a
        assert a.flags.c_contiguous
        return C.c_void_p(address(a) + off) if a.size else None
