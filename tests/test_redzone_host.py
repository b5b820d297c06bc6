"""The guarded allocator of tests/_redzone.py, tested on CPU tensors: it finds a one-byte write on either side of a body, hands out
exact sizes, and records what was allocated.  (The harness is never tested by giving a kernel a short buffer.)"""
import pytest
import torch

from _redzone import ALIGN, BACK_MIN, FRONT, GUARD_BYTE, RedZone


def test_clean_run_passes_and_layout_is_as_stated():
    with RedZone("cpu") as rz:
        a = torch.empty(7, 3, dtype=torch.float32, device="cpu")
        b = torch.zeros((5,), dtype=torch.int32)
        c = torch.full((4,), 2.5, dtype=torch.float64, device="cpu")
    rz.check()
    assert a.shape == (7, 3) and a.is_contiguous() and torch.isnan(a).all()   # 0xFF body: NaN as fp32
    assert b.tolist() == [0] * 5 and c.tolist() == [2.5] * 4
    a.fill_(1.0), b.fill_(3), c.fill_(0.0)   # writing the whole body touches no guard
    rz.check()
    for t, rec in zip((a, b, c), rz.records):
        assert t.data_ptr() % ALIGN == 0
        assert rec.start >= FRONT and rec.raw.data_ptr() + rec.start == t.data_ptr()
        assert rec.nbytes == t.numel() * t.element_size()
        assert rec.raw.numel() - rec.start - rec.nbytes == max(BACK_MIN, rec.nbytes)   # the back guard starts at byte n exactly
    torch.empty(3)   # the patch is gone
    assert len(rz.records) == 3


def test_back_guard_grows_with_the_body():
    rz = RedZone("cpu")
    with rz:
        t = torch.empty(BACK_MIN + 1000, dtype=torch.uint8)
    rec = rz.records[0]
    assert rec.raw.numel() - rec.start - rec.nbytes == t.numel()


@pytest.mark.parametrize("body", [0xFF, 0x00])
def test_body_pattern(body):
    with RedZone("cpu", body=body) as rz:
        e = torch.empty(9, dtype=torch.int32)
        z = torch.zeros(9, dtype=torch.int32)
    assert e.tolist() == [-1 if body else 0] * 9 and z.tolist() == [0] * 9
    rz.check()
    with pytest.raises(ValueError):
        RedZone("cpu", body=0x55)


@pytest.mark.parametrize("where", ["before", "after"])
def test_one_byte_outside_is_reported(where):
    with RedZone("cpu") as rz:
        torch.empty(16, dtype=torch.float32)
        victim = torch.empty((3, 5), dtype=torch.float32)
        torch.empty(16, dtype=torch.float32)
    rec = rz.records[1]
    assert rec.nbytes == victim.numel() * 4 == 60
    pos = rec.start - 1 if where == "before" else rec.start + rec.nbytes
    rec.raw[pos] = 0   # a torch write one byte outside the body
    with pytest.raises(AssertionError) as err:
        rz.check()
    msg = str(err.value)
    assert "allocation #1" in msg and "shape (3, 5)" in msg and "torch.float32" in msg and "60 bytes" in msg
    off = -1 if where == "before" else 60
    assert f"bytes {off} .. {off} " in msg
    assert rz.records[0].damage() is None and rz.records[2].damage() is None and rec.damage() == (off, off)


def test_first_and_last_damaged_offsets():
    with RedZone("cpu") as rz:
        t = torch.empty(10, dtype=torch.uint8)
    rec = rz.records[0]
    rec.raw[rec.start - 3] = 1
    rec.raw[rec.start + t.numel() + 8] = 1
    assert rec.damage() == (-3, 18)


def test_shapes_as_tuple_varargs_and_zero_size():
    with RedZone("cpu") as rz:
        a = torch.empty((2, 3), dtype=torch.int16)
        b = torch.empty(2, 3, dtype=torch.int16)
        c = torch.empty([2, 3], dtype=torch.int16)
        d = torch.empty(torch.Size((2, 3)), dtype=torch.int16)
        z0 = torch.empty(0, dtype=torch.float32)
        z1 = torch.zeros((0, 3), dtype=torch.float32)
        s = torch.full((), 7, dtype=torch.int32)
    assert a.shape == b.shape == c.shape == d.shape == (2, 3)
    assert z0.shape == (0,) and z1.shape == (0, 3) and z0.numel() == z1.numel() == 0
    assert s.shape == () and int(s) == 7
    assert [r.nbytes for r in rz.records] == [12, 12, 12, 12, 0, 0, 4]
    rz.check()


def test_like_functions_of_a_guarded_tensor():
    with RedZone("cpu") as rz:
        x = rz.guarded(torch.arange(12, dtype=torch.float32).reshape(3, 4))
        e = torch.empty_like(x)
        z = torch.zeros_like(x)
        h = torch.empty_like(x, dtype=torch.uint8)
        p = torch.empty_like(x.t())   # not contiguous: passes through, keeps torch's strides
    assert x.tolist() == torch.arange(12.0).reshape(3, 4).tolist()
    assert e.shape == z.shape == h.shape == (3, 4) and z.abs().sum() == 0 and h.dtype == torch.uint8
    assert [r.kind for r in rz.records] == ["guarded", "empty_like", "zeros_like", "empty_like"]
    assert p.shape == (4, 3)
    e.copy_(x), z.copy_(x)
    rz.check()


def test_ones_and_full_like():
    src = torch.zeros((2, 3), dtype=torch.int32)
    with RedZone("cpu") as rz:
        x = rz.guarded(src)
        o = torch.ones((2, 2), dtype=torch.float32)
        ol = torch.ones_like(x)
        fl = torch.full_like(x, 7)
        fp = torch.full_like(x.t(), 7)   # not contiguous: passes through
    assert o.tolist() == [[1.0, 1.0], [1.0, 1.0]] and ol.tolist() == [[1] * 3] * 2 and fl.tolist() == [[7] * 3] * 2 and fp.shape == (3, 2)
    assert [r.kind for r in rz.records] == ["guarded", "ones", "ones_like", "full_like"]
    rz.check()


def test_guarded_offsets_and_exact_size():
    src = torch.arange(5, dtype=torch.float32)
    rz = RedZone("cpu")
    g0, g4, g8 = rz.guarded(src), rz.guarded(src, offset_bytes=4), rz.guarded(src, 8)
    assert g0.data_ptr() % 256 == 0 and g4.data_ptr() % 16 == 4 and g8.data_ptr() % 16 == 8
    for g, rec in zip((g0, g4, g8), rz.records):
        assert g.tolist() == src.tolist() and rec.nbytes == 20 and rec.kind == "guarded"
        assert int(rec.raw[rec.start + 20]) == GUARD_BYTE and int(rec.raw[rec.start - 1]) == GUARD_BYTE
    rz.check()
    with pytest.raises(ValueError):
        rz.guarded(torch.zeros(2, dtype=torch.float64), offset_bytes=4)
    gr = rz.guarded(torch.ones(3, requires_grad=True))
    assert not gr.requires_grad and gr.grad_fn is None and gr._base is None   # a plain tensor, not an autograd view


def test_scratch_offset_moves_flat_byte_tensors_only():
    with RedZone("cpu", scratch_offset=16) as rz:
        s = torch.empty(100, dtype=torch.uint8)
        z = torch.zeros((64,), dtype=torch.uint8)
        img = torch.empty((4, 25), dtype=torch.uint8)
        f = torch.empty(100, dtype=torch.float32)
    assert s.data_ptr() % 256 == 16 and z.data_ptr() % 256 == 16 and img.data_ptr() % 256 == 0 and f.data_ptr() % 256 == 0
    assert [r.nbytes for r in rz.records] == [100, 64, 100, 400] and int(z.sum()) == 0
    rec = rz.records[0]
    rec.raw[rec.start - 1] = 0   # the 16 bytes in front of a moved body are guard as well
    assert rec.damage() == (-1, -1)


def test_pass_through():
    with RedZone("cpu") as rz:
        m = torch.empty(4, device="meta")                      # another device
        q = torch.empty(4, dtype=torch.float32, requires_grad=True)   # another keyword argument
        k = torch.zeros(size=(4,))                             # no positional size
        o = torch.arange(4)                                    # not a patched factory
    assert m.device.type == "meta" and q.requires_grad and k.shape == (4,) and o.sum() == 6
    assert rz.records == []
    with RedZone("meta") as rz2:
        c = torch.empty(4)   # default device is the CPU, the harness guards another one
    assert rz2.records == [] and c.device.type == "cpu"


def test_default_device_decides_a_call_without_one():
    prev = torch.get_default_device()
    try:
        torch.set_default_device("meta")
        with RedZone("cpu") as rz:
            m = torch.empty(4)                 # goes to the default device, which is not the guarded one
            c = torch.empty(4, device="cpu")
        with RedZone("meta") as rz2:
            d = torch.empty(4, dtype=torch.uint8)   # ... and here it is
    finally:
        torch.set_default_device(prev)
    assert m.device.type == "meta" and c.device.type == "cpu" and [r.shape for r in rz.records] == [(4,)]
    assert d.device.type == "meta" and len(rz2.records) == 1


def test_coverage_record():
    src = torch.zeros(100, dtype=torch.uint8)
    with RedZone("cpu") as rz:
        x = rz.guarded(src)
        torch.empty(1000, dtype=torch.uint8)
        torch.empty((25,), dtype=torch.float32)
    assert rz.allocations() == [(0, "guarded", (100,), torch.uint8, 100), (1, "empty", (1000,), torch.uint8, 1000),
                                (2, "empty", (25,), torch.float32, 100)]
    assert rz.allocations("guarded") == [(0, "guarded", (100,), torch.uint8, 100)]
    assert rz.saw_bytes(1000) and not rz.saw_bytes(999) and not rz.saw_bytes(1001)
    assert x.numel() == 100 and rz.saw_bytes(100)   # the fp32 one; a guarded input alone would not count
    with RedZone("cpu") as other:
        torch.empty((10, 10), dtype=torch.uint8)     # 100 bytes, but no flat tensor
        torch.empty(25, dtype=torch.int32)           # 100 bytes, but neither uint8 nor float32
    assert not other.saw_bytes(100) and len(other.records) == 2
    rz.require("thousand", 1000)
    with pytest.raises(AssertionError, match="not covered"):
        rz.require("short by a word", 996)
    only_input = RedZone("cpu")
    only_input.guarded(torch.zeros(64, dtype=torch.uint8))
    assert not only_input.saw_bytes(64)


def test_patch_is_removed_on_error_and_not_reentrant():
    real = torch.empty
    rz = RedZone("cpu")
    with pytest.raises(RuntimeError, match="boom"):
        with rz:
            assert torch.empty is not real
            raise RuntimeError("boom")
    assert torch.empty is real and torch.zeros_like.__name__ == "zeros_like"
    with rz:
        with pytest.raises(RuntimeError, match="re-entrant"):
            rz.__enter__()
    assert torch.empty is real
