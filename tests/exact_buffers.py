"""Caller buffers exactly as large and exactly as aligned as the C headers promise (include/pcpx.h, conventions): the arena of
tests/test_gpu_exact_buffers.py.  A helper module, no conftest; it works on CPU tensors as on GPU ones.

Every GPU test of the suite otherwise hands the library tensors straight from torch's allocator: at least 256-byte aligned, with
allocator slack behind them and usually another tensor in front.  An Arena hands out views of ONE uint8 allocation instead, each
laid out as

    guard | payload | guard

  guard    at least GUARD = 16 KiB of the byte 0xA5 on either side.  A condition, not a measurement: twice the largest block one
           wavefront writes (64 rows x 33 floats of FPFH are 8.3 KiB, 64 kNN rows of 32 words 8 KiB).
  payload  exactly the bytes asked for, filled with 0x5A (an output) or with the given data (an input), at an address that is
           `misalign` modulo 16: by default the element size (4 for float / uint32, 8 for uint64 / double; 1 for uint8), that is
           the least alignment the element type has.  An empty payload is legal: an address between two guards.

check() finds every write outside the payloads; untouched() asserts that elements the contract leaves to the caller still hold
the fill.  An over-read cannot be seen directly, but it reads 0xA5A5A5A5 -- as an index out of every range, as a float about
-2.9e-16 -- so a result that depends on it differs from the expected one."""
import numpy as np

GUARD = 16384
GUARD_BYTE = 0xA5
FILL_BYTE = 0x5A
KINDS = {"u8": ("uint8", 1), "u32": ("int32", 4), "f32": ("float32", 4), "u64": ("int64", 8), "f64": ("float64", 8)}


def _torch():
    import torch
    return torch


def kind_of(array):
    """the kind of a numpy array's dtype"""
    return {"uint8": "u8", "bool": "u8", "uint32": "u32", "int32": "u32", "float32": "f32", "uint64": "u64", "int64": "u64",
            "float64": "f64"}[np.asarray(array).dtype.name]


class Arena:
    def __init__(self, device, nbytes=32 << 20):
        t = _torch()
        self.device = t.device(device)
        self.bytes = t.full((int(nbytes),), GUARD_BYTE, dtype=t.uint8, device=self.device)
        self.base = self.bytes.data_ptr()
        self.cursor = 0    # every byte below it is a payload or a guard in front of one
        self.buffers = []  # (name, first byte, bytes)

    def take(self, name, length, kind, misalign=None, data=None):
        """a view of `length` elements of `kind` at an address that is `misalign` modulo 16 (default: the element size), filled with
        0x5A or with `data` (a numpy array of that many elements of that size)"""
        t = _torch()
        dtype, size = KINDS[kind]
        misalign = size if misalign is None else int(misalign)
        assert misalign % size == 0 and 0 <= misalign < 16, (name, kind, misalign)
        nbytes = int(length) * size
        first = self.cursor + GUARD
        first += (misalign - (self.base + first)) % 16
        assert first + nbytes + GUARD <= self.bytes.numel(), "the arena is full: %s needs %d bytes" % (name, nbytes)
        payload = self.bytes[first:first + nbytes]
        if data is None:
            payload.fill_(FILL_BYTE)
        else:
            raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
            assert raw.size == nbytes, (name, raw.size, nbytes)
            payload.copy_(t.from_numpy(raw.copy()))
        self.buffers.append((name, first, nbytes))
        self.cursor = first + nbytes
        return payload.view(getattr(t, dtype))

    def address(self, name):
        """the payload's address (a view of no element cannot tell it)"""
        return self.base + [b for b in self.buffers if b[0] == name][-1][1]

    def check(self, what=""):
        """after the caller has drained the streams: every guard byte is still 0xA5.  Compared on the device; names the buffer, the
        side and the first changed offset (bytes before the payload's first byte, or behind its last)."""
        t = _torch()
        end = min(self.cursor + GUARD, self.bytes.numel())
        bad = self.bytes[:end] != GUARD_BYTE
        for _name, first, nbytes in self.buffers:
            bad[first:first + nbytes] = False
        if not bool(bad.any()):
            return
        at = int(t.nonzero(bad)[0, 0])
        # the guard that holds the byte lies between two payloads: the nearer one is named
        best = None
        for name, first, nbytes in self.buffers:
            for side, distance in (("before", first - at), ("after", at - (first + nbytes) + 1)):
                if 0 < distance <= GUARD + 16 and (best is None or distance < best[0]):
                    best = (distance, name, side)
        distance, name, side = best
        value = int(self.bytes[at])
        raise AssertionError("%s: a write outside its buffers: %d byte(s) %s the payload of %r (byte 0x%02X), %d guard byte(s) changed in all"
                             % (what, distance, side, name, value, int(bad.sum())))

    @staticmethod
    def untouched(view, mask, what=""):
        """the elements of `view` (a tensor or a numpy array) under `mask` (one flag per element, or per row of a 2-d view) still
        hold the 0x5A fill"""
        t = _torch()
        if not hasattr(view, "data_ptr"):
            view = t.from_numpy(np.ascontiguousarray(view).copy())
        rows = view.shape[0] if view.dim() > 1 else view.numel()
        raw = view.contiguous().view(t.uint8).reshape(rows, -1)
        m = t.as_tensor(np.asarray(mask, bool).reshape(-1), device=raw.device)
        if m.numel() != rows:  # (one flag per element of a 2-d view)
            raw = raw.reshape(m.numel(), -1)
        bad = (raw != FILL_BYTE).any(1) & m
        if bool(bad.any()):
            at = int(t.nonzero(bad)[0, 0])
            raise AssertionError("%s: %d element(s) the call should have left alone were written, the first at %d" % (what, int(bad.sum()), at))
