"""Poisoned memory for kernel tests: a kernel may not depend on bytes it does not own, nor write them.

``poisoned_allocations``: while active, every ``torch.empty`` / ``torch.empty_like`` of a device tensor comes out of a pool filled with one
byte value, with 256 guard bytes on either side -- outputs and workspaces no longer hold what the previous call of the same size left there,
and ``check()`` finds a store outside the allocation.  ``moated``: an operand inside a pool of the same byte, with a padded leading
dimension and an odd base if asked, and a checker that everything outside the operand is untouched.

The fill bytes: 0x00 (0 everywhere), 0xFF (NaN as float32 / float64, 255 as uint8, -1 as a counter) and 0x7B (about 1.3e36 as float32, the
impossible pooling decision 123 as uint8; for paths whose contract excludes NaN).  Plain torch, any device.
"""
import threading

import torch

GUARD = 256                     # bytes on either side of a poisoned allocation; keeps every alignment the library tests (16 bytes at most)
FILLS = (0x00, 0xFF, 0x7B)


def _contiguous_strides(shape):
    strides, acc = [], 1
    for s in reversed(shape):
        strides.append(acc)
        acc *= max(int(s), 1)
    return tuple(reversed(strides))


def _size_of(args):
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    if not all(isinstance(s, int) and not isinstance(s, bool) for s in args):
        return None
    return tuple(int(s) for s in args)


class poisoned_allocations:
    """Context manager.  ``cuda_only=False`` lifts the device condition (the CPU tests of the detector itself)."""

    def __init__(self, monkeypatch, fill, cuda_only=True):
        assert 0 <= fill <= 255
        self.monkeypatch, self.fill, self.cuda_only = monkeypatch, int(fill), cuda_only
        self.pools = []                               # (pool, nbytes, shape, dtype)
        self._lock = threading.Lock()                 # autograd runs backward nodes, which allocate, on its own threads
        self._real_empty, self._real_empty_like = torch.empty, torch.empty_like

    # ---- the replacement allocators ----
    def _eligible(self, device):
        if self.cuda_only:
            if device.type != "cuda":
                return False
            if torch.cuda.is_current_stream_capturing():
                return False
        return True

    def _alloc(self, shape, dtype, device, requires_grad=False):
        nbytes = dtype.itemsize
        for s in shape:
            nbytes *= s
        pool = torch.full((nbytes + 2 * GUARD,), self.fill, dtype=torch.uint8, device=device)
        out = pool[GUARD:GUARD + nbytes].view(dtype).view(shape)
        with self._lock:
            self.pools.append((pool, nbytes, tuple(shape), dtype))
        return out.requires_grad_(True) if requires_grad else out

    def _empty(self, *args, **kw):
        size = _size_of(args)
        plain = set(kw) <= {"dtype", "device", "requires_grad"}
        if size is None or not plain:
            return self._real_empty(*args, **kw)
        device = torch.device(kw["device"]) if kw.get("device") is not None else torch.get_default_device()
        if not self._eligible(device):
            return self._real_empty(*args, **kw)
        dtype = kw.get("dtype") or torch.get_default_dtype()
        return self._alloc(size, dtype, device, bool(kw.get("requires_grad", False)))

    def _empty_like(self, t, **kw):
        plain = set(kw) <= {"dtype", "device", "requires_grad"}
        if not plain or not isinstance(t, torch.Tensor) or t.layout != torch.strided:
            return self._real_empty_like(t, **kw)
        device = torch.device(kw["device"]) if kw.get("device") is not None else t.device
        if not self._eligible(device):
            return self._real_empty_like(t, **kw)
        # the real function preserves the strides of a dense permuted input: only the contiguous result is served from a pool
        if self._real_empty_like(t, device="meta").stride() != _contiguous_strides(t.shape):
            return self._real_empty_like(t, **kw)
        return self._alloc(tuple(t.shape), kw.get("dtype") or t.dtype, device, bool(kw.get("requires_grad", False)))

    def __enter__(self):
        self.monkeypatch.setattr(torch, "empty", self._empty)
        self.monkeypatch.setattr(torch, "empty_like", self._empty_like)
        return self

    def __exit__(self, *exc):
        self.monkeypatch.setattr(torch, "empty", self._real_empty)
        self.monkeypatch.setattr(torch, "empty_like", self._real_empty_like)
        return False

    # ---- the guards ----
    def check(self):
        """Every guard band of every pool still holds the fill byte, byte for byte."""
        with self._lock:
            pools = list(self.pools)
        by_device = {}
        for entry in pools:
            by_device.setdefault(entry[0].device, []).append(entry)
        for entries in by_device.values():
            bands = torch.stack([torch.cat([pool[:GUARD], pool[GUARD + nbytes:]]) for pool, nbytes, _, _ in entries])
            bad = (bands != self.fill).any(dim=1)
            if bool(bad.any()):
                i = int(bad.nonzero()[0])
                pool, nbytes, shape, dtype = entries[i]
                at = (bands[i] != self.fill).nonzero().flatten().tolist()
                where = [f"{a - GUARD} (before)" if a < GUARD else f"+{a - GUARD} (behind)" for a in at[:8]]
                raise AssertionError(f"guard band of the allocation shape {shape} dtype {dtype} ({nbytes} bytes) was written: "
                                     f"{len(at)} bytes differ from {self.fill:#04x}, at byte offsets {where}")
        return len(pools)

    def release(self):
        """Forget the pools (between the runs of one test, so that their memory returns to the allocator)."""
        with self._lock:
            self.pools.clear()


def fill_value(fill, dtype, device="cpu"):
    """The one-element tensor of ``dtype`` whose every byte is ``fill``."""
    return torch.full((dtype.itemsize,), fill, dtype=torch.uint8, device=device).view(dtype)


def moated(t, fill, ld=None, offset=0, guard_rows=2, device=None, dtype=torch.float32):
    """Put the host tensor ``t`` (2-D, or contiguous N-D) into a pool on ``device`` whose every other byte is ``fill``.

    ``t`` may also be a shape: the operand's own region is then left at the fill (an output).  ``ld``: row stride in elements (2-D only;
    default: the row length), ``offset``: elements between the 256-byte aligned start of the operand's region and its first element,
    ``guard_rows``: rows of poison before and after (at least 256 bytes).  Returns ``(view, check)``; ``check()`` asserts that the pool
    outside the view is untouched."""
    if isinstance(t, torch.Tensor):
        shape, dtype, src = tuple(t.shape), t.dtype, t
    else:
        shape, src = tuple(int(s) for s in t), None
    device = torch.device(device) if device is not None else (src.device if src is not None else torch.device("cpu"))
    if ld is None:
        strides = _contiguous_strides(shape)
        row = shape[-1] if shape else 1
    else:
        assert len(shape) == 2 and ld >= shape[1], "moated: a leading dimension needs a 2-D operand no wider than it"
        strides, row = (ld, 1), ld
    isz = dtype.itemsize
    span = 1 + sum((s - 1) * st for s, st in zip(shape, strides)) if all(s > 0 for s in shape) else 0      # elements first .. last
    if ld is not None and shape[0] > 0:
        span = shape[0] * ld                           # the padding behind the last row belongs to the moat, and to the pool
    lead = -(-max(guard_rows * row * isz, GUARD) // GUARD) * GUARD
    nelem = lead // isz + offset + span + lead // isz
    pool = torch.full((nelem * isz,), fill, dtype=torch.uint8, device=device)
    typed = pool.view(dtype)
    view = typed.as_strided(shape, strides, lead // isz + offset)
    if src is not None:
        view.copy_(src)
    poison = fill_value(fill, dtype, device)

    def check():
        probe = pool.clone()
        probe.view(dtype).as_strided(shape, strides, lead // isz + offset).copy_(poison.expand(shape) if shape else poison[0])
        bad = probe != fill
        if bool(bad.any()):
            at = (bad.nonzero().flatten() // isz).unique()[:8].tolist()
            first = lead // isz + offset
            where = [f"element {a - first} = row {(a - first) // row} + {(a - first) % row}" if a >= first else f"element {a - first} (before)"
                     for a in at]
            raise AssertionError(f"moat around the operand shape {shape} ld {row} offset {offset} was written: {int(bad.sum())} bytes differ "
                                 f"from {fill:#04x}; first at {where}")

    return view, check
