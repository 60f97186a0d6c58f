"""Guard-band allocator for the memory-safety tests (tests/test_memory_guards.py).

`with guarded(fill) as arena:` replaces torch.empty, torch.empty_like, torch.zeros, torch.zeros_like, Tensor.new_empty and
Tensor.new_zeros for the forms the package uses (sizes as varargs or as one tuple, `dtype=`, `device=`); every other form
falls through to the original.  Each replaced allocation is the interior of one uint8 block

    [ GUARD bytes of 0xA5 | nbytes of interior | slack up to a multiple of 256, 0xA5 | GUARD bytes of 0xA5 ]

so the interior keeps the block's own alignment (GUARD is a multiple of 256: the kernels' 16-byte fast paths are the ones
exercised) and has known bytes on both sides.  The interior of the `empty` family is filled with `fill`:

    "ff"       0xFF bytes: float NaN, int32 -1
    "zero"     0x00 bytes
    "garbage"  finite seeded random floats of magnitude about 1e3 (as int32: counters around 1.1e9)

and that of the `zeros` family with zero.  `arena.check()` asserts that every guard and slack byte still holds 0xA5 and
names the allocation (index, shape, dtype, the call site that made it), the side and the first / last offending offset.
`arena.place(t)` copies an input into such a block whose guards and slack hold 0xFF instead (NaN as floats): a read past an
input that reaches a result turns the result NaN.

What this sees and what it does not: a write that lands within GUARD = 64 KiB before or after a buffer the Python layer
allocated through the replaced functions while the context is active.  A WRITE FURTHER THAN 64 KiB OUTSIDE ITS BUFFER IS NOT
SEEN, nor is one into a buffer allocated another way (torch.cat, clone, a tensor made before the context was entered), nor a
write inside the right buffer at the wrong place (the value tests do that).  A read outside a buffer is seen only if the value
reaches an output.  The blocks stay alive until the arena is dropped, so a late write into a buffer the package has already
released is still checked.
"""
from __future__ import annotations

import contextlib
import os
import traceback

import torch

GUARD = 64 * 1024
PAD = 0xA5
INPUT_PAD = 0xFF
FILLS = ("ff", "zero", "garbage")
_POOL = 1 << 16          # floats of seeded garbage per device, tiled over larger interiors
_HERE = os.path.abspath(__file__)


def _round_up(n: int, m: int) -> int:
    return -(-n // m) * m


class GuardViolation(AssertionError):
    pass


class _Record:
    __slots__ = ("index", "base", "nbytes", "shape", "dtype", "site", "pad", "kind")

    def describe(self) -> str:
        return (f"allocation #{self.index} ({self.kind}) shape {tuple(self.shape)} dtype {self.dtype} on {self.base.device}, "
                f"made at {self.site}")


def _site() -> str:
    for fr in reversed(traceback.extract_stack(limit=12)):
        if os.path.abspath(fr.filename) != _HERE and "contextlib" not in fr.filename:
            return f"{fr.filename}:{fr.lineno} in {fr.name}"
    return "?"


def _size_of(args):
    """The size of torch.empty(*args) when args are ints or one sequence of ints; None = a form we do not replace."""
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    if all(isinstance(a, int) and not isinstance(a, bool) for a in args) and all(a >= 0 for a in args):
        return tuple(int(a) for a in args)
    return None


class Arena:
    def __init__(self, fill: str, seed: int = 0, originals=None):
        if fill not in FILLS:
            raise ValueError(f"fill must be one of {FILLS}, got {fill!r}")
        self.fill = fill
        self.seed = seed
        self.records: list[_Record] = []
        self._empty = originals["empty"] if originals else torch.empty
        self._pools: dict = {}

    # -- allocation -------------------------------------------------------------------------------------------------------
    def _garbage(self, device, n_floats: int, index: int):
        pool = self._pools.get(device)
        if pool is None:
            g = torch.Generator().manual_seed(self.seed)
            mag = 1e3 * (0.5 + 1.5 * torch.rand(_POOL, generator=g))
            sign = torch.where(torch.rand(_POOL, generator=g) < 0.5, -1.0, 1.0)
            pool = self._pools[device] = (mag * sign).to(torch.float32).to(device)
        pool = pool.roll(-((index * 977) % _POOL))
        if n_floats <= _POOL:
            return pool[:n_floats]
        return pool.repeat(-(-n_floats // _POOL))[:n_floats]

    def _block(self, shape, dtype, device, kind: str, pad: int, interior: str):
        shape = tuple(shape)
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * self._empty((), dtype=dtype).element_size()
        inner = _round_up(nbytes, 256)
        base = self._empty(GUARD + inner + GUARD, dtype=torch.uint8, device=device)
        base[:GUARD].fill_(pad)
        base[GUARD + nbytes:].fill_(pad)
        body = base[GUARD: GUARD + inner]
        if interior == "zero":
            body[:nbytes].zero_()
        elif interior == "ff":
            body[:nbytes].fill_(0xFF)
        elif interior == "garbage":
            body.view(torch.float32).copy_(self._garbage(base.device, inner // 4, len(self.records)))
            base[GUARD + nbytes: GUARD + inner].fill_(pad)
        r = _Record()
        r.index, r.base, r.nbytes, r.shape, r.dtype, r.site, r.pad, r.kind = len(self.records), base, nbytes, shape, dtype, _site(), pad, kind
        self.records.append(r)
        return base[GUARD: GUARD + nbytes].view(dtype).view(shape)

    def allocate(self, shape, dtype, device, zeros: bool, kind: str):
        return self._block(shape, dtype, device, kind, PAD, "zero" if zeros else self.fill)

    def place(self, t: torch.Tensor) -> torch.Tensor:
        """A contiguous copy of `t` (same device, dtype, shape; detached) inside a block whose guards and slack are 0xFF bytes."""
        src = t.detach().contiguous()
        if src.numel() == 0:
            return src.clone()
        out = self._block(src.shape, src.dtype, src.device, "input", INPUT_PAD, "none")
        out.copy_(src)
        return out

    # -- checking ---------------------------------------------------------------------------------------------------------
    def check(self, when: str = "") -> None:
        """Every guard and slack byte of every recorded block still holds its pad byte, else GuardViolation."""
        by_dev: dict = {}
        for r in self.records:
            by_dev.setdefault(r.base.device, []).append(r)
        bad = []
        for dev, recs in by_dev.items():
            flags = []
            for r in recs:
                flags.append((r.base[:GUARD] != r.pad).any())
                flags.append((r.base[GUARD + r.nbytes:] != r.pad).any())
            flags = torch.stack(flags).tolist()
            for k, r in enumerate(recs):
                if flags[2 * k]:
                    bad.append((r, "before"))
                if flags[2 * k + 1]:
                    bad.append((r, "after"))
        if not bad:
            return
        lines = []
        for r, side in bad:
            if side == "before":
                idx = (r.base[:GUARD] != r.pad).nonzero().flatten()
                first, last = int(idx[0]) - GUARD, int(idx[-1]) - GUARD          # bytes relative to the buffer's start (< 0)
                where = f"bytes {first} .. {last} relative to the buffer's first byte"
            else:
                idx = (r.base[GUARD + r.nbytes:] != r.pad).nonzero().flatten()
                first, last = int(idx[0]), int(idx[-1])                          # bytes past the buffer's end (0 = first byte after)
                where = f"bytes +{first} .. +{last} past the buffer's {r.nbytes} bytes"
            lines.append(f"  {side} {r.describe()}: {idx.numel()} byte(s) changed, {where}")
        raise GuardViolation(f"write outside a buffer{(' (' + when + ')') if when else ''}, fill {self.fill!r}:\n" + "\n".join(lines))


_ORIG = None     # the original functions while a guarded() context is active (contexts do not nest)


def _default_device():
    get = getattr(torch, "get_default_device", None)
    return get() if get is not None else torch.device("cpu")


@contextlib.contextmanager
def guarded(fill: str, seed: int = 0):
    """Patch the allocation functions (module docstring) for the duration of the block; yields the Arena.  The patch is undone
    in a `finally`: torch is never left patched, whatever the block raises."""
    global _ORIG
    if _ORIG is not None:
        raise RuntimeError("guarded() contexts do not nest")
    T = torch.Tensor
    orig = dict(empty=torch.empty, empty_like=torch.empty_like, zeros=torch.zeros, zeros_like=torch.zeros_like,
                new_empty=T.new_empty, new_zeros=T.new_zeros)
    own = {k: (k in T.__dict__) for k in ("new_empty", "new_zeros")}
    arena = Arena(fill, seed, orig)

    def factory(name, zeros):
        def fn(*size, dtype=None, device=None, **kw):
            shape = _size_of(size)
            if kw or shape is None or 0 in shape or len(shape) == 0:
                return orig[name](*size, **_kw(dtype, device), **kw)
            return arena.allocate(shape, dtype or torch.get_default_dtype(), torch.device(device) if device is not None else _default_device(),
                                  zeros, f"torch.{name}")
        return fn

    def like(name, zeros):
        def fn(t, *args, dtype=None, device=None, **kw):
            if args or kw or not isinstance(t, torch.Tensor) or t.numel() == 0 or not t.is_contiguous() or t.layout != torch.strided:
                return orig[name](t, *args, **_kw(dtype, device), **kw)
            return arena.allocate(t.shape, dtype or t.dtype, torch.device(device) if device is not None else t.device, zeros,
                                  f"torch.{name}")
        return fn

    def new(name, zeros):
        def fn(self, *size, dtype=None, device=None, **kw):
            shape = _size_of(size)
            if kw or shape is None or 0 in shape or len(shape) == 0 or self.layout != torch.strided:
                return orig[name](self, *size, **_kw(dtype, device), **kw)
            return arena.allocate(shape, dtype or self.dtype, torch.device(device) if device is not None else self.device, zeros,
                                  f"Tensor.{name}")
        return fn

    def _kw(dtype, device):
        out = {}
        if dtype is not None:
            out["dtype"] = dtype
        if device is not None:
            out["device"] = device
        return out

    _ORIG = orig
    try:
        torch.empty, torch.zeros = factory("empty", False), factory("zeros", True)
        torch.empty_like, torch.zeros_like = like("empty_like", False), like("zeros_like", True)
        T.new_empty, T.new_zeros = new("new_empty", False), new("new_zeros", True)
        yield arena
    finally:
        torch.empty, torch.zeros = orig["empty"], orig["zeros"]
        torch.empty_like, torch.zeros_like = orig["empty_like"], orig["zeros_like"]
        for k in ("new_empty", "new_zeros"):
            if own[k]:
                setattr(T, k, orig[k])
            elif k in T.__dict__:
                delattr(T, k)
        _ORIG = None
