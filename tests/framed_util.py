"""Framed buffers: the only overrun check device code can have here.

A framed tensor is a view into one larger uint8 allocation: 64 KiB of a fixed pattern, the payload, 64 KiB of the pattern again.
The payload starts on a 512-byte boundary (what an ordinary torch allocation has) and the rear frame starts at the byte after
the payload's last byte - nothing is rounded up, so one float4 store past the last element lands in the frame.  The pattern is
the 32-bit word 0x7FC0A5A5: a NaN as fp32, an absurd index as int32 (as fp64 it is finite, about 1e307: compare bits there).

  framed(shape, dtype, device, fill=None)   a framed tensor; fill=None leaves the pattern in the payload too
  check(view) / check_all()                 both frames bit for bit; after torch.cuda.synchronize()
  unwritten(view)                           elements that still carry the pattern, compared as bits
  AbiProxy                                  stands in front of the loaded library and refuses an unframed device pointer
  framed_factories()                        redirects torch.empty / zeros / full / ones / *_like on CUDA devices to framed()
  frame_engine(engine)                      moves a model handle's six bound buffers into framed ones of the exact sizes
"""
import contextlib
import ctypes as C

import numpy as np
import torch

_EMPTY = torch.empty                  # the allocator itself: framed_factories() redirects the name torch.empty
WORD = 0x7FC0A5A5
FRAME = 64 * 1024
ALIGN = 512
_PAT4 = (0xA5, 0xA5, 0xC0, 0x7F)       # the word in memory order (little endian)


class FrameError(AssertionError):
    pass


def _pattern(nbytes, device, phase=0):
    """nbytes of the pattern as uint8, starting `phase` bytes into the word"""
    reps = (nbytes + phase + 3) // 4
    p = torch.tensor(_PAT4, dtype=torch.uint8, device=device).repeat(max(reps, 1))
    return p[phase:phase + nbytes]


class _Entry:
    def __init__(self, name, raw, off, nbytes, dtype, shape):
        self.name, self.raw, self.off, self.nbytes, self.dtype, self.shape = name, raw, off, nbytes, dtype, shape
        self.ptr = raw.data_ptr() + off         # (data_ptr() of an empty view may be null: the entry keeps the address itself)

    def payload_bytes(self):
        return self.raw[self.off:self.off + self.nbytes]

    def view(self):
        v = self.payload_bytes().view(self.dtype).view(self.shape)
        v._framed_entry = self
        return v


class Registry:
    """the framed buffers of one test case"""

    def __init__(self):
        self.entries = []

    def framed(self, shape, dtype=torch.float32, device="cpu", fill=None, name=None):
        if isinstance(shape, int):
            shape = (shape,)
        shape = tuple(int(s) for s in shape)
        device = torch.device(device)
        item = _EMPTY(0, dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * item if shape else item
        raw = _EMPTY(FRAME + nbytes + FRAME + ALIGN, dtype=torch.uint8, device=device)
        off = FRAME + (-(raw.data_ptr() + FRAME)) % ALIGN
        pat = _pattern(FRAME, device)
        raw[off - FRAME:off] = pat
        raw[off + nbytes:off + nbytes + FRAME] = pat
        e = _Entry(name or f"buf{len(self.entries)}:{tuple(shape)}:{str(dtype).replace('torch.', '')}", raw, off, nbytes, dtype, shape)
        v = e.view()
        if fill is None:
            if nbytes:
                e.payload_bytes().copy_(_pattern(nbytes, device))
        elif isinstance(fill, torch.Tensor):
            v.copy_(fill.reshape(shape) if fill.numel() == v.numel() else fill)
        else:
            v.fill_(fill)
        self.entries.append(e)
        return v

    def like(self, t, fill="copy", name=None):
        """a framed contiguous tensor of t's shape, dtype and device; by default with t's values"""
        return self.framed(tuple(t.shape), t.dtype, t.device, t if isinstance(fill, str) else fill, name)

    def find(self, ptr):
        """the entry whose payload holds address ptr (its end included: a zero-length payload, or one-past for length 0 calls)"""
        for e in self.entries:
            if e.ptr <= ptr <= e.ptr + e.nbytes:
                return e
        return None

    def entry_of(self, view):
        e = getattr(view, "_framed_entry", None)
        if e is None and view.numel():
            e = self.find(view.data_ptr())
        if e is None:
            raise FrameError("not a framed tensor of this registry")
        return e

    def check(self, view):
        _check_entry(self.entry_of(view))

    def check_all(self):
        for e in self.entries:
            _check_entry(e)


def _check_entry(e):
    pat = _pattern(FRAME, e.raw.device)
    for side, lo in (("front", e.off - FRAME), ("rear", e.off + e.nbytes)):
        got = e.raw[lo:lo + FRAME]
        if torch.equal(got, pat):
            continue
        bad = torch.nonzero(got != pat).reshape(-1)
        first, last, n = int(bad[0]), int(bad[-1]), int(bad.numel())
        # offsets from the payload's edge: the rear frame counts from the byte after the payload (0), the front frame from the
        # byte in front of it (1); `near` is the damaged byte next to the payload, `far` the one furthest from it
        near, far = (first, last) if side == "rear" else (FRAME - last, FRAME - first)
        raise FrameError(f"{e.name}: {side} frame damaged, first damaged byte {near} byte(s) "
                         f"{'past the end' if side == 'rear' else 'before the start'} of the payload, the damage reaches "
                         f"byte {far} ({n} bytes differ)")


_default = Registry()


def framed(shape, dtype=torch.float32, device="cpu", fill=None, name=None):
    return _default.framed(shape, dtype, device, fill, name)


def check(view):
    _check_entry(getattr(view, "_framed_entry", None) or _default.entry_of(view))


def unwritten(view):
    """how many elements of view still carry the pattern, compared as bits (a NaN result is not the pattern)"""
    if view.numel() == 0:
        return 0
    e = getattr(view, "_framed_entry", None)
    phase = (view.data_ptr() - e.ptr) % 4 if e is not None else 0
    item = view.element_size()
    b = view.contiguous().view(torch.uint8).reshape(-1, item)
    want = _pattern(b.numel(), b.device, phase).reshape(-1, item)
    return int((b == want).all(dim=1).sum())


# ---- the ABI proxy ------------------------------------------------------------------------------------------------------

class AbiProxy:
    """In front of the loaded library (`monkeypatch.setattr(_lib, "_lib", AbiProxy(...))`): every c_void_p argument of every call
    must be null, exempt - `exempt[(entry point, argument index)] = reason` - or point into a payload of `registry`."""

    def __init__(self, real, sigs, registry, exempt):
        self._real, self._sigs, self._registry, self._exempt = real, sigs, registry, exempt
        self.seen = set()
        self.calls = []           # (entry point, its arguments), in call order

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        sig = self._sigs.get(name)
        if sig is None or C.c_void_p not in sig[1]:
            return fn
        argtypes = sig[1]

        def call(*args):
            for i, (a, t) in enumerate(zip(args, argtypes)):
                if t is not C.c_void_p or (name, i) in self._exempt:
                    continue
                v = a.value if isinstance(a, C.c_void_p) else a
                if not v:
                    continue
                if self._registry.find(int(v)) is None:
                    raise FrameError(f"{name}: argument {i} (0x{int(v):x}) points into no framed buffer and is not exempt")
            self.seen.add(name)
            self.calls.append((name, args))
            return fn(*args)

        return call


# ---- framed allocation inside the wrappers -----------------------------------------------------------------------------------

def _size(args, kw):
    if "size" in kw:
        return tuple(kw.pop("size")), args
    if len(args) and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(args[0]), args[1:]
    n = 0
    while n < len(args) and isinstance(args[n], (int, np.integer)) and not isinstance(args[n], bool):
        n += 1
    return tuple(int(a) for a in args[:n]), args[n:]


def _infer_dtype(value):
    if isinstance(value, bool):
        return torch.bool
    if isinstance(value, int):
        return torch.int64
    return torch.get_default_dtype()


@contextlib.contextmanager
def framed_factories(registry, concat=False):
    """torch.empty / zeros / full / ones / empty_like / zeros_like / full_like allocate framed tensors on CUDA devices while
    this is active (`empty` with the pattern in the payload); every frame is checked on exit.  concat: what torch.cat and
    torch.stack return on a CUDA device is moved into a framed tensor as well (a wrapper that concatenates per-stream results
    into one argument of a call)."""
    orig = {k: getattr(torch, k) for k in ("empty", "zeros", "full", "ones", "empty_like", "zeros_like", "full_like")}
    if concat:
        orig.update(cat=torch.cat, stack=torch.stack)
    plain = {"dtype", "device", "requires_grad", "layout", "pin_memory", "memory_format"}

    def is_cuda(dev):
        return dev is not None and torch.device(dev).type == "cuda"

    def shaped(kind, value):
        def f(*args, **kw):
            if not is_cuda(kw.get("device")) or set(kw) - plain - {"size", "fill_value"}:
                return orig[kind](*args, **kw)
            kw = dict(kw)
            shape, rest = _size(args, kw)
            fill = value
            if kind == "full":
                fill = kw.pop("fill_value") if "fill_value" in kw else rest[0]
            dtype = kw.get("dtype") or (_infer_dtype(fill) if kind == "full" else torch.get_default_dtype())
            return registry.framed(shape, dtype, kw["device"], fill, name=f"torch.{kind}{shape}")
        return f

    def like(kind, value):
        def f(t, *args, **kw):
            dev = kw.get("device", t.device)
            if not is_cuda(dev) or set(kw) - plain - {"fill_value"}:
                return orig[kind](t, *args, **kw)
            fill = value
            if kind == "full_like":
                fill = kw["fill_value"] if "fill_value" in kw else args[0]
            return registry.framed(tuple(t.shape), kw.get("dtype") or t.dtype, dev, fill, name=f"torch.{kind}{tuple(t.shape)}")
        return f

    new = {"empty": shaped("empty", None), "zeros": shaped("zeros", 0), "ones": shaped("ones", 1), "full": shaped("full", None),
           "empty_like": like("empty_like", None), "zeros_like": like("zeros_like", 0), "full_like": like("full_like", None)}
    def joined(kind):
        def f(*args, **kw):
            r = orig[kind](*args, **kw)
            return registry.framed(tuple(r.shape), r.dtype, r.device, r, name=f"torch.{kind}{tuple(r.shape)}") if r.is_cuda else r
        return f

    if concat:
        new.update(cat=joined("cat"), stack=joined("stack"))
    for k, f in new.items():
        setattr(torch, k, f)
    try:
        yield registry
    finally:
        for k, f in orig.items():
            setattr(torch, k, f)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    registry.check_all()


# ---- model handles ----------------------------------------------------------------------------------------------------------

def frame_engine(eng, registry, lib):
    """Copy the six buffers the handle is bound to into framed ones of exactly ral_param_floats / ral_state_floats /
    ral_bn_sums_doubles elements, replace the engine's attributes and bind again (ral_bind may be called again: it resets the
    handle's caches).  -> {name: framed tensor}"""
    sizes = {"params": (lib.ral_param_floats(C.byref(eng.cfg)), torch.float32),
             "grads": (lib.ral_param_floats(C.byref(eng.cfg)), torch.float32),
             "adam_m": (lib.ral_param_floats(C.byref(eng.cfg)), torch.float32),
             "adam_v": (lib.ral_param_floats(C.byref(eng.cfg)), torch.float32),
             "state": (lib.ral_state_floats(C.byref(eng.cfg)), torch.float32),
             "bn_sums": (lib.ral_bn_sums_doubles(C.byref(eng.cfg)), torch.float64)}
    out = {}
    for k, (n, dt) in sizes.items():
        old = getattr(eng, k)
        if old is None:
            continue
        assert old.numel() == n and old.dtype == dt, (k, old.numel(), n)
        out[k] = registry.framed((n,), dt, old.device, old, name=f"engine.{k}[{n}]")
        setattr(eng, k, out[k])
    p = lambda k: C.c_void_p(registry.entry_of(out[k]).ptr) if k in out else C.c_void_p(0)
    rc = lib.ral_bind(eng.h, p("params"), p("grads"), p("adam_m"), p("adam_v"), p("state"), p("bn_sums"))
    assert rc == 0, lib.ral_last_error().decode()
    return out
