"""The checker of tests/guarded.py on CPU tensors: simulated overruns of one element are reported with the region's name and
the byte offset, a clean run reports nothing.  (tests/test_gpu_device_extents.py repeats one control on the device.)"""
import numpy as np
import pytest
import torch

from guarded import ALIGN, Slab, itemsize

NTH, STRIDE = 5, 8
ODD = float(np.frombuffer(bytes([0x11] * 8), dtype=np.float64)[0])   # no byte in common with the prefills or the inputs


def make(misalign=0, guard=4096):
    """Regions as a strided gradient call has them: an fp64 input, an fp64 output, a strided output with gap columns, an int32
    output, an fp32 output; every output prefilled 0xFF, guards 0xA5."""
    s = Slab("cpu", guard_bytes=guard)
    s.region("dX", torch.float64, (3, 2, 15), misalign, role="input")
    s.region("dmean", torch.float64, (3, 20), misalign)
    s.region("dgrad", torch.float64, (3, STRIDE), misalign, keep=np.arange(STRIDE) >= NTH)
    s.region("dinfo", torch.int32, (3,), misalign)
    s.region("dvar32", torch.float32, (3, 20), misalign)
    s.fill_guards(0xA5)
    s.view("dX").copy_(torch.arange(90, dtype=torch.float64).view(3, 2, 15))
    for name in ("dmean", "dgrad", "dinfo", "dvar32"):
        s.fill(name, 0xFF)
    return s


def raw(s):
    """The slab's bytes, writable (a store through this view is what a stray kernel store would be)."""
    return s.buf.numpy()


@pytest.mark.parametrize("misalign", [0, 1])
def test_layout(misalign):
    s = make(misalign)
    end = 0
    for name, r in s.regions.items():
        assert s.ptr(name) % ALIGN == misalign * r.item and s.ptr(name) % r.item == 0
        assert r.start - r.lo >= s.guard and r.hi - r.end == s.guard and r.lo == end
        end = r.hi
        assert tuple(s.view(name).shape) == r.shape and s.view(name).dtype == r.dtype
        assert s.view(name).data_ptr() == s.ptr(name)
    assert end == s.buf.numel()
    assert torch.equal(s.view("dX"), torch.arange(90, dtype=torch.float64).view(3, 2, 15))
    assert torch.isnan(s.view("dmean")).all() and (s.view("dinfo") == -1).all() and torch.isnan(s.view("dvar32")).all()
    r = s.regions["dmean"]
    assert (raw(s)[r.lo:r.start] == 0xA5).all() and (raw(s)[r.end:r.hi] == 0xA5).all()


@pytest.mark.parametrize("misalign", [0, 1])
def test_a_clean_run_reports_nothing(misalign):
    s = make(misalign)
    snap = s.snapshot()
    s.view("dmean").copy_(torch.rand(3, 20, dtype=torch.float64))
    s.view("dgrad")[:, :NTH] = 1.5
    s.view("dinfo").zero_()
    s.view("dvar32").fill_(2.0)
    assert s.check(snap) == []
    # a store of the value a byte already holds is not a change (the reason the GPU tests run two guard patterns)
    r = s.regions["dmean"]
    raw(s)[r.end] = 0xA5
    assert s.check(snap) == []


@pytest.mark.parametrize("misalign", [0, 1])
@pytest.mark.parametrize("name", ["dmean", "dinfo", "dvar32", "dX"])
def test_one_element_before_and_after_a_region(name, misalign):
    s = make(misalign)
    r = s.regions[name]
    item = itemsize(r.dtype)
    snap = s.snapshot()
    raw(s)[r.end:r.end + item] = 0
    assert s.check(snap) == [(name, "after", 0, item)]
    raw(s)[r.start - item:r.start] = 0
    assert s.check(snap) == [(name, "before", -item, item), (name, "after", 0, item)]
    # a padded row further out: the first offset and the number of changed bytes
    s = make(misalign)
    r = s.regions[name]
    snap = s.snapshot()
    raw(s)[r.end + 3 * item:r.end + 7 * item] = 1
    assert s.check(snap) == [(name, "after", 3 * item, 4 * item)]


def test_a_store_into_a_stride_gap():
    s = make()
    snap = s.snapshot()
    s.view("dgrad")[:, :NTH] = 0.25
    assert s.check(snap) == []
    s.view("dgrad")[1, NTH] = 0.25
    assert s.check(snap) == [("dgrad", "gap", (STRIDE + NTH) * 8, 8)]
    s.view("dgrad")[2, STRIDE - 1] = 0.25      # the last gap element belongs to the documented extent, not to the guard
    assert s.check(snap) == [("dgrad", "gap", (STRIDE + NTH) * 8, 16)]


def test_a_store_into_an_input_region():
    s = make()
    snap = s.snapshot()
    s.view("dX")[2, 1, 14] = ODD
    assert s.check(snap) == [("dX", "input", 89 * 8, 8)]
    s.view("dX")[2, 1, 14] = 89.0              # the same value back: nothing to report
    assert s.check(snap) == []


def test_an_output_that_is_kept_whole_is_an_optional_output_not_passed():
    s = Slab("cpu", guard_bytes=512)
    s.region("dlogml", torch.float64, (4,), keep=True)
    s.region("dinfo", torch.int32, (4,), keep=np.array([False, True, False, True]))
    s.fill_guards(0x3F)
    s.fill("dlogml", 0x3F)
    s.fill("dinfo", 0xFF)
    snap = s.snapshot()
    s.view("dinfo")[0] = 0
    s.view("dinfo")[2] = 0
    assert s.check(snap) == []
    s.view("dlogml")[3] = ODD
    s.view("dinfo")[3] = 0
    assert s.check(snap) == [("dlogml", "gap", 24, 8), ("dinfo", "gap", 12, 4)]


def test_a_narrow_store_is_counted_in_bytes():
    """A 4-byte store where 8 are due leaves half of the element: the count tells."""
    s = make()
    r = s.regions["dmean"]
    snap = s.snapshot()
    raw(s)[r.end:r.end + 4] = 0
    assert s.check(snap) == [("dmean", "after", 0, 4)]


def test_regions_are_fixed_once_the_slab_is_used():
    s = make()
    with pytest.raises(AssertionError):
        s.region("late", torch.float64, (1,))
