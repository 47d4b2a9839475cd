"""Launch traces of the engine: every call into libkaranta_hip.so, in order, with its arguments in a form that does not depend
on where the allocator put anything.  Two trees whose engines issue the same launches give the same trace, whatever module
the launch is written in: the refactoring check of tests/test_gpu_launch_trace.py.

    with launch_trace(eng) as calls:
        eng.generate(...)
    names(calls), digest(calls)

Per call: [entry point, [argument, ...]].  A non-pointer argument is its value; a struct passed by reference (kr_dec32, kr_spec,
kr_narrow_opts, kr_fork_plan) is a dict of its fields; a pointer is "null", "host", "main" / "other" (a stream), [leaf attribute
name of the engine-owned tensor it falls inside, byte offset], [layout name of the weight it falls inside, byte offset], or
"tmp" for anything else (a per-call buffer, a cached table, a graph handle).  Tensors are looked up at the time of the call
among the attributes of the engine and of the objects of this package it holds (its weights, its components)."""
import bisect
import contextlib
import ctypes as C
import hashlib
import json

import torch

from karanta_ocr_amd import _lib

_POINTERS = (C.c_void_p, C.c_char_p)


def _owners(eng):
    yield eng
    for v in vars(eng).values():
        if type(v).__module__.startswith("karanta_ocr_amd") and hasattr(v, "__dict__"):
            yield v


def _tensor_map(eng):
    """[(first byte, last byte + 1, leaf name)] of every device tensor the engine or one of its components holds as an attribute
    (the extent is the storage's: a view such as d_ctx names the rows behind it too), and the weight arena's layout."""
    spans, arena = [], None
    for o in _owners(eng):
        if getattr(o, "arena", None) is not None and hasattr(o, "layout"):
            base = o.arena.data_ptr()
            names = sorted((off, name) for name, (off, _) in o.layout.items())
            arena = (base, base + o.arena.numel(), [off for off, _ in names], [n for _, n in names])
        for name, v in vars(o).items():
            if isinstance(v, torch.Tensor) and v.is_cuda and name != "arena":
                st = v.untyped_storage()
                spans.append((st.data_ptr(), st.data_ptr() + st.nbytes(), name))
    return spans, arena


def _streams(eng, main):
    other = set()
    for name in ("stream", "_adm_stream", "_dec_stream", "_copy_stream"):
        s = getattr(eng, name, None)
        if s is not None and s.cuda_stream != main:
            other.add(s.cuda_stream)
    return other


class _Resolver:
    def __init__(self, eng):
        self.eng, self.main = eng, eng.stream.cuda_stream

    def begin(self):
        self.spans, self.arena = _tensor_map(self.eng)
        self.other = _streams(self.eng, self.main)

    def pointer(self, p):
        if not p:
            return "null"
        if p == self.main:
            return "main"
        if p in self.other:
            return "other"
        if self.arena is not None and self.arena[0] <= p < self.arena[1]:
            rel = p - self.arena[0]
            i = bisect.bisect_right(self.arena[2], rel) - 1
            return [self.arena[3][i], rel - self.arena[2][i]]
        hits = sorted((name, p - lo) for lo, hi, name in self.spans if lo <= p < hi)
        return list(hits[0]) if hits else "tmp"

    def struct(self, s):
        out, limit = {}, {}
        for name, ctype in s._fields_:
            v = getattr(s, name)
            if issubclass(ctype, C.Array):
                n = limit.get(name, len(v))
                out[name] = [self.struct(e) if isinstance(e, C.Structure) else int(e) for e in list(v)[:max(0, n)]]
            elif issubclass(ctype, _POINTERS):
                out[name] = self.pointer(v)
            else:
                out[name] = self.scalar(v, ctype)
            if name == "n_groups":      # kr_fork_plan / kr_fork_group: only the entries in use
                limit["groups"] = int(v)
            if name == "n_dst":
                limit["dst"] = int(v)
        return out

    @staticmethod
    def scalar(v, ctype):
        if ctype is C.c_float:
            return repr(C.c_float(float(v)).value)
        return int(v)

    def arg(self, v, ctype):
        inner = getattr(v, "_obj", None)            # ctypes.byref(...)
        if isinstance(inner, C.Structure):
            return self.struct(inner)
        if inner is not None or isinstance(v, (C.Array, C._Pointer)) or not issubclass(ctype, _POINTERS + (C._SimpleCData,)):
            return "host"
        if issubclass(ctype, _POINTERS):
            if isinstance(v, C.c_void_p):
                v = v.value
            return self.pointer(v) if v is None or isinstance(v, int) else "host"
        return self.scalar(v, ctype)


@contextlib.contextmanager
def launch_trace(eng):
    """Records every call of an entry point of _lib.SIGNATURES made while the block runs, from any module: the wrappers sit on
    the `lib()` singleton.  Yields the list the calls are appended to."""
    L, res, calls = _lib.lib(), _Resolver(eng), []
    saved = {name: getattr(L, name) for name in _lib.SIGNATURES}

    def wrap(name, fn, argtypes):
        def call(*args):
            res.begin()
            calls.append([name, [res.arg(a, t) for a, t in zip(args, argtypes)]])
            return fn(*args)
        call.__name__ = name
        return call

    for name, fn in saved.items():
        setattr(L, name, wrap(name, fn, _lib.SIGNATURES[name]))
    try:
        yield calls
    finally:
        for name, fn in saved.items():
            setattr(L, name, fn)


def names(calls):
    return [c[0] for c in calls]


def canonical(calls) -> str:
    return json.dumps(calls, sort_keys=True, separators=(",", ":"))


def digest(calls) -> str:
    return hashlib.sha256(canonical(calls).encode()).hexdigest()
