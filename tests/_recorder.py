"""A stand-in for the ctypes library that records every call instead of launching: shared by test_dispatch_cpu.py (the hot
path of ops.py) and test_gpu_frame_ops_trace.py (the wrappers of frame_ops.py)."""
import ctypes

FAKE_SIZES = (("_bytes", 4096), ("_workspace", 4096), ("_chunks", 4), ("_slots", 4))


class Recorder:
    """stands in for the ctypes library: records every call; forwards to `real` if given (only the names `forward` accepts,
    when that is given too), else answers `sizes` by suffix and 0 (hipSuccess) to everything else"""

    def __init__(self, real=None, forward=None, sizes=FAKE_SIZES):
        self.calls, self.real, self.forward, self.sizes = [], real, forward, sizes

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append([name, [_arg(a) for a in args]])
            if self.real is not None and (self.forward is None or self.forward(name)):
                return getattr(self.real, name)(*args)
            return next((v for suffix, v in self.sizes if name.endswith(suffix)), 0)
        return entry


def _arg(a):
    """the int / float value of an argument, 1 / 0 for a pointer given / null, a list of these for a ctypes array"""
    if a is None:
        return 0
    if isinstance(a, ctypes.c_void_p):
        return 1 if a.value else 0
    if isinstance(a, ctypes.Array):
        return [(1 if v else 0) if a._type_ is ctypes.c_void_p else _arg(v) for v in a]
    return float(a) if isinstance(a, float) else int(a)
