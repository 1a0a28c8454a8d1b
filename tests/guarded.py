"""Guard-band allocations for the tests of the device entry points (tests/test_gpu_device_extents.py).

The `*_device` entry points of include/corenav_gp.h hand the caller's pointers straight to kernels that work in padded shapes.
A test that gives every argument a tensor of its own cannot see a store one padded row past an output, nor a result that
depends on what lies behind an input: the allocator rounds and spreads the tensors.  A Slab is ONE torch.uint8 allocation out
of which every argument of a call is carved as a named region,

    [before-guard] region 0 [after-guard] [before-guard] region 1 [after-guard] ...

each region with at least `guard_bytes` of guard on either side, starting 256-byte aligned plus `misalign` ELEMENTS (the header
promises no alignment beyond the element's own: a slice of a larger array is a legitimate caller).  The guards, every input
region and the `keep` elements of an output region (the gap columns of a strided array, the entries of unselected windows, an
optional output that is not passed) are protected: snapshot() copies the slab to the host before the call, check() lists
what changed among the protected bytes after it.

Reach of the method.  The default guard of 64 KiB is a condition, not a measurement: it covers a full padded row of every
shape the tests run (the largest is 128 doubles, 1 KiB) many times over; a stray store that lands further away than that from
every region is outside this checker's reach.  A READ past an extent is only visible when it reaches a result: the tests run
the same call over guards of different content and compare the outputs bitwise.  Nothing here touches the device beyond plain
torch copies and fills inside the slab's own allocation, so the same class runs on CPU tensors (tests/test_guarded_cpu.py)."""
import numpy as np
import torch

ALIGN = 256


def itemsize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


class _Region:
    __slots__ = ("name", "dtype", "shape", "misalign", "role", "keep", "item", "nbytes", "start", "end", "lo", "hi")


class Slab:
    """Declare every region with region(), then use view() / ptr() / fill*() / snapshot() / check(): the allocation is made at
    the first use, after which no region can be added."""

    def __init__(self, device, guard_bytes=65536):
        self.device = torch.device(device)
        self.guard = int(guard_bytes)
        self.regions = {}
        self.buf = None

    # ---- layout -----------------------------------------------------------------------------------------------------------
    def region(self, name, dtype, shape, misalign=0, role="output", keep=None):
        """role "input": the whole region is protected.  role "output": only the elements where `keep` (a bool array that
        broadcasts to `shape`; None = no element) is True are."""
        assert self.buf is None, "regions are declared before the slab is used"
        assert name not in self.regions and role in ("input", "output")
        r = _Region()
        r.name, r.dtype, r.shape, r.misalign, r.role = name, dtype, tuple(int(s) for s in shape), int(misalign), role
        r.item = itemsize(dtype)
        r.nbytes = int(np.prod(r.shape, dtype=np.int64)) * r.item
        r.keep = None if keep is None else np.ascontiguousarray(np.broadcast_to(np.asarray(keep, dtype=bool), r.shape))
        self.regions[name] = r
        return name

    def _build(self):
        if self.buf is not None:
            return
        cap = sum(2 * self.guard + ALIGN + r.misalign * r.item + r.nbytes for r in self.regions.values()) + ALIGN
        buf = torch.zeros(cap, dtype=torch.uint8, device=self.device)
        base, pos = buf.data_ptr(), 0
        for r in self.regions.values():
            r.lo = pos                                             # [lo, start): the before-guard (with the alignment slack)
            a = base + pos + self.guard
            r.start = (a + ALIGN - 1) // ALIGN * ALIGN - base + r.misalign * r.item
            r.end = r.start + r.nbytes
            r.hi = pos = r.end + self.guard                        # [end, hi): the after-guard
        assert pos <= cap
        self.buf = buf[:pos]
        prot = np.ones(pos, dtype=bool)
        for r in self.regions.values():
            if r.role == "output":
                prot[r.start:r.end] = False if r.keep is None else np.repeat(r.keep.reshape(-1), r.item)
        self.protected = prot

    def view(self, name):
        """The region as a tensor of its dtype and shape (a view of the slab)."""
        self._build()
        r = self.regions[name]
        return self.buf[r.start:r.end].view(r.dtype).view(r.shape)

    def ptr(self, name):
        self._build()
        r = self.regions[name]
        p = self.buf.data_ptr() + r.start
        assert p % r.item == 0 and (r.misalign or p % ALIGN == 0)
        return p

    # ---- content ----------------------------------------------------------------------------------------------------------
    def fill_guards(self, byte):
        self._build()
        for r in self.regions.values():
            self.buf[r.lo:r.start].fill_(byte)
            self.buf[r.end:r.hi].fill_(byte)

    def fill(self, name, byte):
        self._build()
        r = self.regions[name]
        self.buf[r.start:r.end].fill_(byte)

    def snapshot(self):
        """A host copy of the slab as it stands (the guards and the input regions among it)."""
        self._build()
        return self.buf.cpu().numpy().copy()

    def check(self, snapshot):
        """[(region, side, first offset, byte count)] of the protected bytes that differ from `snapshot`: side "before" (offset
        < 0, relative to the region's first byte), "after" (offset >= 0, relative to the first byte past the region), "input"
        or "gap" (offset from the region's first byte).  Empty when nothing outside the outputs was written."""
        cur = self.buf.cpu().numpy()
        changed = (cur != snapshot) & self.protected
        if not changed.any():
            return []
        found = []
        for r in self.regions.values():
            inner = "input" if r.role == "input" else "gap"
            for side, lo, hi, origin in (("before", r.lo, r.start, r.start), (inner, r.start, r.end, r.start),
                                         ("after", r.end, r.hi, r.end)):
                idx = np.flatnonzero(changed[lo:hi])
                if idx.size:
                    found.append((r.name, side, int(lo + idx[0] - origin), int(idx.size)))
        return found
