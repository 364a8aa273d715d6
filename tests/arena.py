"""One guarded allocation for every pointer a test hands to the library (a helper module, not a conftest).

Arena(torch, device, fill) owns one uint8 tensor, filled with a pattern. take(nbytes, align) carves a view of
exactly nbytes bytes out of it:
  - the view's address is a multiple of `align` and not of 2 * align, so a pointer has the alignment
    include/ghs_mst.h promises and no more (16 for u / v / w / workspace / index, 8 for 64-bit arrays, 4 for
    32-bit outputs, 1 for flags);
  - RED_ZONE bytes that belong to no view lie before and after every view. 64 KiB is a condition, not a
    measurement: it is more than one 1024-thread workgroup storing 16 B per lane (16 KiB), so a tail lane,
    wave or workgroup that runs past its buffer lands in a red zone, never in a neighbouring view.
check() compares every byte outside the views with the fill, in one compare on the arena's device, and returns
the offsets that changed; describe() names the view each offset lies next to. snapshot() / unchanged() cover
the buffers a call declares input-only, and the whole arena for a call that must write nothing.

The fill is a constant byte or "ramp" (position-dependent). A store of the constant c into a red zone filled
with c is invisible, so one case runs under two fills that differ in every byte (0x00 and 0xA5): an
out-of-bounds store of any constant is caught by at least one run.

Works on CPU tensors too (tests/test_arena.py shows there that it fails when it should)."""
import numpy as np

RED_ZONE = 64 * 1024
FILLS = (0x00, 0xA5)


class Arena:
    def __init__(self, torch, device, fill, capacity=48 << 20):
        self.torch, self.fill = torch, fill
        if fill == "ramp":
            pos = torch.arange(capacity, dtype=torch.int64, device=device)
            self.pristine = ((pos * 167 + 13) & 0xFF).to(torch.uint8)
        else:
            assert isinstance(fill, int) and 0 <= fill <= 0xFF, fill
            self.pristine = torch.full((capacity,), fill, dtype=torch.uint8, device=device)
        self.buf = self.pristine.clone()
        self.base = self.buf.data_ptr()
        self.in_view = torch.zeros(capacity, dtype=torch.bool, device=device)
        self.views = {}          # name -> (offset, nbytes), in order of address
        self.cursor = 0          # the end of the last view

    # ---- carving --------------------------------------------------------------------------------------------
    def take(self, nbytes, align, name=None):
        """A view of exactly nbytes bytes (a zero-length view still has an address: see ptr)."""
        nbytes, align = int(nbytes), int(align)
        assert nbytes >= 0 and align >= 1 and align & (align - 1) == 0
        off = self.cursor + RED_ZONE
        while (self.base + off) % align or (self.base + off) % (2 * align) == 0:
            off += 1 if (self.base + off) % align else align
        if off + nbytes + RED_ZONE > self.buf.numel():
            raise MemoryError(f"arena of {self.buf.numel()} bytes is full at {name!r} ({nbytes} bytes)")
        name = name if name is not None else f"view{len(self.views)}"
        assert name not in self.views, name
        self.views[name] = (off, nbytes)
        self.in_view[off:off + nbytes] = True
        self.cursor = off + nbytes
        return self.buf[off:off + nbytes]

    def view(self, name):
        off, nbytes = self.views[name]
        return self.buf[off:off + nbytes]

    def ptr(self, name):
        """The address of a view as an int (torch gives an empty view no address of its own)."""
        return self.base + self.views[name][0]

    def put(self, name, array, align):
        """take() a view the size of a numpy array and copy the array's bytes into it."""
        a = np.ascontiguousarray(array)
        v = self.take(a.nbytes, align, name)
        self.write(name, a)
        return v

    def write(self, name, array, stream_ordered=False):
        """Copy a numpy array of the view's size over the view (on the current stream)."""
        a = np.ascontiguousarray(array)
        v = self.view(name)
        assert a.nbytes == v.numel(), (name, a.nbytes, v.numel())
        if a.nbytes:
            src = self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy())
            if stream_ordered and v.is_cuda:
                src = src.pin_memory()
            v.copy_(src, non_blocking=stream_ordered)
        return v

    def read(self, name, dtype=np.uint8, count=None):
        """The view's bytes on the host as `dtype` (the first `count` elements)."""
        a = self.view(name).cpu().numpy().view(dtype)
        return a.copy() if count is None else a[:count].copy()

    # ---- checking -------------------------------------------------------------------------------------------
    def check(self):
        """The offsets of all changed red-zone bytes (one device-side compare)."""
        bad = (self.buf != self.pristine) & ~self.in_view
        return bad.nonzero().reshape(-1).cpu().numpy().tolist()

    def nearest(self, offset):
        """(name, side, distance) of the view nearest to a red-zone offset: side "before" or "after" the
        view, distance 1 for the byte that touches it."""
        best = None
        for name, (off, nb) in self.views.items():
            if offset < off:
                cand = (off - offset, "before", name)
            else:
                assert offset >= off + nb, "a red-zone byte lies in no view"
                cand = (offset - (off + nb) + 1, "after", name)
            best = cand if best is None or cand[0] < best[0] else best
        return (best[2], best[1], best[0]) if best else (None, None, None)

    def describe(self, offsets, limit=8):
        """For messages: each offset with the view it lies next to, e.g. 'd_core: 4 after'."""
        out = ["%s: %s %s" % (n, d, s) for n, s, d in (self.nearest(o) for o in offsets[:limit])]
        if len(offsets) > limit:
            out.append(f"... {len(offsets)} bytes in all")
        return out

    def names(self, offsets):
        """The names of the views the changed bytes lie next to."""
        return sorted({self.nearest(o)[0] for o in offsets})

    def snapshot(self):
        return self.buf.clone()

    def unchanged(self, snap, name=None):
        """Is the view `name` (default: the whole arena) byte-identical to the snapshot?"""
        if name is None:
            return bool(self.torch.equal(self.buf, snap))
        off, nbytes = self.views[name]
        return bool(self.torch.equal(self.buf[off:off + nbytes], snap[off:off + nbytes]))
