"""Hostile device memory for the op-level tests: every tensor a kernel sees is the middle of its own larger allocation.

An Arena hands out device tensors.  Each one sits between two bands of at least BAND bytes, and every byte of the allocation starts as 0xFF:
as float32 / float64 that is a NaN with all bits set, as int64 it is -1, as uint8 it is 255 (the ignore id, the hostile value for labels).

  inp(array)              the data copied in; the arena keeps a device copy of the bytes
  out(shape, dtype)       the interior stays 0xFF; untouched=True declares an output the call must leave alone
  inout(array)            a buffer the op updates in place: bands, no intact check
  verify()                on the device, bringing back one flag per check (and the first offending offset only when a check fails):
                            every band byte of every tensor is still 0xFF             -> "<name>: band before|after ..."
                            every inp tensor has the bytes of its copy                -> "<name>: input changed ..."
                            no float32 / float64 / int64 element of an out tensor still has all bits set (arithmetic cannot produce that
                            pattern from inputs that do not hold it)                  -> "<name>: output element ... never written"
                            an out(..., untouched=True) tensor is still all 0xFF      -> "<name>: untouched output written ..."

A load past the end of an input reads the band: a NaN that reaches a result fails every `rel_err(...) < tol` and `assert_array_equal` the tests
already make.

BAND is a condition, not a measurement: it exceeds the largest block tile any of the convolution, pool and loss kernels stores -- 256 rows x 256
fp32 columns = 256 KiB (conv_bf16_256_kernel<256> and the fp8 kernel's 256-row tile; the fp32 implicit GEMMs and the weight gradients stop at
128 x 128) -- so a block that runs a whole tile past an end still lands in memory this module owns and checks.  Tensors start at a multiple of
256 bytes, so the 16-byte paths run as they do on an allocation of their own.

session(lib) is what the adopted modules' autouse fixtures wrap a test in: an Arena that inp / out / inout below reach as the current one, the op
context "op_poison_scratch" on (the two per-stream scratch pools are NaN at every hand-out), verify() at the end, the option put back."""
import contextlib
import ctypes as C

import numpy as np
import torch

BAND = 1 << 20
ALIGN = 256
CHECKED_OUT_DTYPES = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int64: torch.int64}


class HostileMemoryError(AssertionError):
    """verify() found something; .failures is a list of (tensor name, kind, byte offset, distance), kind one of 'before', 'after', 'changed',
    'unwritten', 'written'; the offset counts from the start of what the check covers (the band, or the tensor), distance is the number of
    bytes between a 'before' offence and the tensor's first byte (0 for the other kinds)."""
    def __init__(self, failures):
        self.failures = failures
        text = {"before": "%s: band before the tensor overwritten, first at byte %d of the band (%d bytes before the tensor)",
                "after": "%s: band after the tensor overwritten, first at byte %d past its end",
                "changed": "%s: input changed, first at byte %d",
                "unwritten": "%s: output element at byte %d never written (all bits still set)",
                "written": "%s: untouched output written, first at byte %d"}
        lines = []
        for name, kind, off, extra in failures:
            lines.append(text[kind] % ((name, off, extra) if kind == "before" else (name, off)))
        super().__init__("; ".join(lines))


class _Item:
    def __init__(self, name, kind, raw, lo, nbytes, tensor, copy=None):
        self.name, self.kind, self.raw, self.lo, self.nbytes, self.tensor, self.copy = name, kind, raw, lo, nbytes, tensor, copy


class Arena:
    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.items = []

    # ---- allocation ----------------------------------------------------------------------------------------------------------------------
    def _carve(self, shape, dtype, name, kind):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        esize = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * esize
        raw = torch.full((2 * BAND + nbytes + ALIGN,), 0xFF, dtype=torch.uint8, device=self.device)
        lo = BAND + (-(raw.data_ptr() + BAND)) % ALIGN
        tensor = raw[lo:lo + nbytes].view(dtype).reshape(shape)
        assert tensor.data_ptr() % ALIGN == 0 and lo >= BAND and raw.numel() - (lo + nbytes) >= BAND
        item = _Item(name or "%s#%d" % (kind, len(self.items)), kind, raw, lo, nbytes, tensor)
        self.items.append(item)
        return item

    def inp(self, array, name=None):
        a = np.ascontiguousarray(array)
        src = torch.from_numpy(a.copy())
        item = self._carve(a.shape, src.dtype, name, "inp")
        item.tensor.copy_(src)
        item.copy = item.raw[item.lo:item.lo + item.nbytes].clone()
        return item.tensor

    def out(self, shape, dtype=torch.float32, name=None, untouched=False):
        return self._carve(shape, dtype, name, "untouched" if untouched else "out").tensor

    def inout(self, array, name=None):
        a = np.ascontiguousarray(array)
        src = torch.from_numpy(a.copy())
        item = self._carve(a.shape, src.dtype, name, "inout")
        item.tensor.copy_(src)
        return item.tensor

    # ---- checks --------------------------------------------------------------------------------------------------------------------------
    def _checks(self):
        """(item, kind, bad) with bad a device bool vector over the bytes (or elements: see scale) of what the check covers; nothing is synchronised"""
        for it in self.items:
            raw, lo, hi = it.raw, it.lo, it.lo + it.nbytes
            yield it, "before", raw[:lo] != 0xFF, 1
            yield it, "after", raw[hi:] != 0xFF, 1
            body = raw[lo:hi]
            if it.kind == "inp":
                yield it, "changed", body != it.copy, 1
            elif it.kind == "untouched":
                yield it, "written", body != 0xFF, 1
            elif it.kind == "out" and it.tensor.dtype in CHECKED_OUT_DTYPES:
                as_int = CHECKED_OUT_DTYPES[it.tensor.dtype]
                yield it, "unwritten", body.view(as_int) == -1, torch.empty((), dtype=as_int).element_size()

    def verify(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        checks = list(self._checks())
        flags = torch.stack([bad.any() for _, _, bad, _ in checks]).cpu().numpy() if checks else np.zeros(0, bool)
        failures = []
        for (it, kind, bad, scale), flag in zip(checks, flags):
            if not flag:
                continue
            first = int(torch.nonzero(bad)[0, 0].item()) * scale          # (only on a failure: one more round trip)
            failures.append((it.name, kind, first, it.lo - first if kind == "before" else 0))
        if failures:
            raise HostileMemoryError(failures)


# ---- the current arena of a test (the adopted modules' fixtures set it) ------------------------------------------------------------------
_current = []


def current():
    assert _current, "no hostile.session is open: the module's autouse fixture opens one per test"
    return _current[-1]


def inp(array, name=None):
    return current().inp(array, name)


def out(shape, dtype=torch.float32, name=None, untouched=False):
    return current().out(shape, dtype, name, untouched)


def inout(array, name=None):
    return current().inout(array, name)


def poisoned_bytes(L):
    v = C.c_int64(-1)
    L.check(L.lib.fcn8s_get_option(None, b"op_scratch_poisoned_bytes", C.byref(v)))
    return int(v.value)


@contextlib.contextmanager
def session(L):
    """One test's worth: a fresh Arena as the current one and NaN scratch pools; at the end verify() and the option as it was.
    L: fcn8s_tensorflow_amd._lib."""
    prev = C.c_int64(-1)
    L.check(L.lib.fcn8s_get_option(None, b"op_poison_scratch", C.byref(prev)))
    L.check(L.lib.fcn8s_set_option(None, b"op_poison_scratch", 1))
    arena = Arena()
    _current.append(arena)
    try:
        yield arena
        arena.verify()
    finally:
        _current.pop()
        arena.items.clear()
        L.lib.fcn8s_set_option(None, b"op_poison_scratch", int(prev.value))
