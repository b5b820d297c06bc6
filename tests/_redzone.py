"""A guarded allocator for tests: every tensor a wrapper allocates sits between two guard zones.

The caching allocator rounds every block up and carves it out of large segments, so a size function that is short by a few words,
a kernel that writes one row past a ragged size or a vector load that reads past an input all go unnoticed.  Inside `RedZone`
the factory functions the wrappers use (torch.empty, zeros, ones, full and their _like forms) hand out tensors of EXACTLY the requested
size inside a larger byte buffer

    [ front guard >= 4 KiB | body: n bytes, 256-byte aligned (+ offset_bytes) | back guard = max(64 KiB, n), from byte n exactly ]

whose guards hold 0xFF (NaN as fp32, -1 as int32) and whose body is pre-filled with 0xFF or 0x00.  The tensors are ordinary ones
over that buffer's storage (no autograd views); growing one with resize_ is not supported, it would grow into its guard.  `check()` asserts that every
guard is intact; `allocations()` is the record of what was asked for, so a test can assert that a scratch buffer of exactly
L.dgm_*_bytes(...) was allocated under the guards.  Works on any device (the harness tests itself on the CPU)."""
import numbers

import torch

FRONT = 4096
BACK_MIN = 65536
ALIGN = 256
GUARD_BYTE = 0xFF

_FACTORIES = ("empty", "zeros", "ones", "full", "empty_like", "zeros_like", "ones_like", "full_like")
_REAL = {name: getattr(torch, name) for name in _FACTORIES}


class Allocation:
    def __init__(self, order, kind, shape, dtype, nbytes, raw, start):
        self.order, self.kind, self.shape, self.dtype, self.nbytes, self.raw, self.start = order, kind, shape, dtype, nbytes, raw, start

    def __repr__(self):
        return f"allocation #{self.order} ({self.kind}, shape {self.shape}, {self.dtype}, {self.nbytes} bytes)"

    def damage(self):
        """None, or (first, last) damaged byte offsets relative to the body's first byte (negative: front guard; >= nbytes: back)."""
        end = self.start + self.nbytes
        front, back = self.raw[:self.start], self.raw[end:]
        if int(torch.minimum(front.min(), back.min())) == GUARD_BYTE:
            return None
        bad = torch.cat(((front != GUARD_BYTE).nonzero().flatten() - self.start, (back != GUARD_BYTE).nonzero().flatten() + self.nbytes))
        return int(bad[0]), int(bad[-1])


def _itemsize(dtype):
    return _REAL["empty"](0, dtype=dtype).element_size()


def _shape(args):
    if len(args) == 1 and not isinstance(args[0], numbers.Integral):
        return tuple(int(s) for s in args[0])
    return tuple(int(s) for s in args)


class RedZone:
    """with RedZone("cuda") as rz: out = wrapper(rz.guarded(x)); rz.check()"""

    def __init__(self, device="cpu", body=0xFF, scratch_offset=0):
        """scratch_offset: the one-dimensional uint8 tensors the factories hand out (the wrappers' idiom for scratch) start that many
        bytes behind the 256-byte grid, to hold a library to the alignment it documents for its scratch."""
        if body not in (0xFF, 0x00):
            raise ValueError("body pattern is 0xFF or 0x00")
        self.device = torch.device(device)
        self.body = body
        self.scratch_offset = int(scratch_offset)
        self.records = []
        self._saved = None

    # ---- the buffers ----
    def _matches(self, device):
        if device is None:  # a factory call without a device: torch's default one
            device = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
        d = torch.device(device)
        return d.type == self.device.type and (d.index is None or self.device.index is None or d.index == self.device.index)

    def _alloc(self, kind, shape, dtype, offset_bytes=0, fill_byte=None):
        shape = tuple(shape)
        item = _itemsize(dtype)
        numel = 1
        for s in shape:
            numel *= s
        n = numel * item
        if offset_bytes % item:
            raise ValueError(f"offset_bytes {offset_bytes} is no multiple of the {item}-byte element")
        raw = _REAL["full"]((FRONT + ALIGN + offset_bytes + n + max(BACK_MIN, n),), GUARD_BYTE, dtype=torch.uint8, device=self.device)
        start = FRONT + (-(raw.data_ptr() + FRONT)) % ALIGN + offset_bytes
        raw = raw[:start + n + max(BACK_MIN, n)]  # the back guard is exactly max(64 KiB, n)
        fill = self.body if fill_byte is None else fill_byte
        if fill != GUARD_BYTE and n:
            raw[start:start + n] = fill
        out = _REAL["empty"](0, dtype=dtype, device=self.device)
        strides, acc = [], 1
        for s in reversed(shape):
            strides.append(acc)
            acc *= max(s, 1)
        out.set_(raw.untyped_storage(), (raw.storage_offset() + start) // item, shape, tuple(reversed(strides)))
        self.records.append(Allocation(len(self.records), kind, shape, dtype, n, raw, start))
        return out

    def guarded(self, x, offset_bytes=0):
        """A copy of x at its exact size between guards; offset_bytes (4, 8) moves the start off the 16-byte grid."""
        x = x.detach()
        out = self._alloc("guarded", x.shape, x.dtype, offset_bytes, fill_byte=GUARD_BYTE)
        out.copy_(x)
        return out

    # ---- the patch ----
    def _wrap(self, name):
        real = _REAL[name]

        def dtype_of(kw, default=None):
            return kw["dtype"] if kw.get("dtype") is not None else (default or torch.get_default_dtype())

        def factory(*args, **kw):
            if set(kw) - {"dtype", "device"} or not args:
                return real(*args, **kw)
            try:
                if name.endswith("_like"):
                    x = args[0]
                    device = kw.get("device") if kw.get("device") is not None else x.device
                    if len(args) != (2 if name == "full_like" else 1) or not self._matches(device) or not x.is_contiguous() \
                            or x.layout != torch.strided:
                        return real(*args, **kw)
                    shape, dtype = tuple(x.shape), dtype_of(kw, x.dtype)
                elif name == "full":
                    if len(args) != 2 or not self._matches(kw.get("device")):
                        return real(*args, **kw)
                    shape = _shape(args[:1])
                    v = args[1]
                    inferred = torch.bool if isinstance(v, bool) else torch.int64 if isinstance(v, int) else None
                    dtype = dtype_of(kw, inferred)
                else:
                    if not self._matches(kw.get("device")):
                        return real(*args, **kw)
                    shape, dtype = _shape(args), dtype_of(kw)
            except (TypeError, ValueError):
                return real(*args, **kw)
            if dtype.is_complex or any(s < 0 for s in shape):
                return real(*args, **kw)
            shift = self.scratch_offset if dtype == torch.uint8 and len(shape) == 1 else 0
            out = self._alloc(name, shape, dtype, shift, fill_byte=0x00 if name.startswith("zeros") else None)
            if name.startswith("full"):
                out.fill_(args[1])
            elif name.startswith("ones"):
                out.fill_(1)
            return out

        factory.__name__ = name
        return factory

    def __enter__(self):
        if self._saved is not None:
            raise RuntimeError("RedZone is not re-entrant")
        self._saved = {name: getattr(torch, name) for name in _FACTORIES}
        for name in _FACTORIES:
            setattr(torch, name, self._wrap(name))
        return self

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(torch, name, fn)
        self._saved = None
        return False

    # ---- what a test asks ----
    def check(self):
        """Every guard of every allocation still holds its pattern (synchronise the device first)."""
        for rec in self.records:
            d = rec.damage()
            assert d is None, (f"red zone damaged: {rec}: bytes {d[0]} .. {d[1]} relative to the body's start "
                               f"(negative: before it; >= {rec.nbytes}: behind it)")

    def allocations(self, kind=None):
        """The coverage record: (order, kind, shape, dtype, nbytes) of everything handed out, in order of creation."""
        return [(r.order, r.kind, r.shape, r.dtype, r.nbytes) for r in self.records if kind is None or r.kind == kind]

    def _scratch_like(self):
        """What a wrapper allocates as scratch: a flat uint8 or float32 tensor from a factory call (not a guarded input)."""
        return [r for r in self.records if r.kind != "guarded" and len(r.shape) == 1 and r.dtype in (torch.uint8, torch.float32)]

    def saw_bytes(self, nbytes):
        """An intercepted factory call asked for a flat uint8 / float32 tensor of exactly nbytes bytes."""
        return any(r.nbytes == int(nbytes) for r in self._scratch_like())

    def require(self, what, nbytes):
        assert self.saw_bytes(nbytes), (f"not covered: no flat uint8 / float32 allocation of exactly {int(nbytes)} bytes ({what}) was seen; "
                                       f"seen: {sorted({r.nbytes for r in self._scratch_like()})}")
