"""tests/arena.py on CPU tensors: the harness of the memory-contract tests fails when it should. A torch store
one element past a view, or one before it, is reported next to the right buffer; a store inside a view is not;
every view has the alignment asked for and no more, and 64 KiB of red zone on both sides."""
import numpy as np
import pytest
import torch

from arena import FILLS, RED_ZONE, Arena

CAP = 1 << 20


def _arena(fill):
    a = Arena(torch, "cpu", fill, capacity=CAP)
    a.take(4 * 37, 16, "d_u")
    a.take(8 * 5, 8, "d_key")
    a.take(4 * 11, 4, "d_out")
    a.take(13, 1, "d_flags")
    return a


@pytest.mark.parametrize("fill", FILLS + ("ramp",))
def test_fresh_arena_is_clean(fill):
    a = _arena(fill)
    assert a.check() == []
    snap = a.snapshot()
    assert a.unchanged(snap) and all(a.unchanged(snap, k) for k in a.views)


@pytest.mark.parametrize("fill", FILLS + ("ramp",))
def test_store_one_element_past_a_view_is_reported(fill):
    a = _arena(fill)
    off, nb = a.views["d_out"]
    a.buf[off + nb:off + nb + 4].view(torch.int32)[0] = 0x11223344      # the 12th element of an 11-element output
    bad = a.check()
    assert bad == list(range(off + nb, off + nb + 4))
    assert a.names(bad) == ["d_out"]
    assert a.nearest(bad[0]) == ("d_out", "after", 1)
    assert "d_out" in a.describe(bad)[0] and "after" in a.describe(bad)[0]


@pytest.mark.parametrize("fill", FILLS + ("ramp",))
def test_store_one_element_before_a_view_is_reported(fill):
    a = _arena(fill)
    off, _ = a.views["d_key"]
    a.buf[off - 8:off].view(torch.int64)[0] = 0x0102030405060708
    bad = a.check()
    assert bad == list(range(off - 8, off))
    assert a.names(bad) == ["d_key"]
    assert a.nearest(bad[-1]) == ("d_key", "before", 1)


@pytest.mark.parametrize("fill", FILLS + ("ramp",))
def test_store_inside_a_view_is_not_reported(fill):
    a = _arena(fill)
    snap = a.snapshot()
    a.view("d_out").view(torch.int32)[:] = 0x5A5A5A5A
    a.view("d_flags")[-1] = 7                                            # the last byte of a view is the view's
    a.view("d_u")[0] = 9                                                 # and so is the first
    assert a.check() == []
    assert not a.unchanged(snap, "d_out") and not a.unchanged(snap, "d_flags") and not a.unchanged(snap)
    assert a.unchanged(snap, "d_key")


def test_a_constant_store_is_caught_by_one_of_the_two_fills():
    """Writing the byte c over a red zone filled with c changes nothing: the reason a case runs twice."""
    for c in (0x00, 0xA5, 0x3C, 0xFF):
        seen = []
        for fill in FILLS:
            a = _arena(fill)
            off, nb = a.views["d_flags"]
            a.buf[off + nb] = c
            seen.append(a.check() == [off + nb])
        assert any(seen), c
    assert all((x ^ y) for x, y in [FILLS])                              # the two fills differ


@pytest.mark.parametrize("align", [1, 4, 8, 16])
def test_alignment_is_exactly_what_was_asked(align):
    a = Arena(torch, "cpu", 0xA5, capacity=CAP)
    for i, nbytes in enumerate((0, 1, 7, 64, 4097)):
        v = a.take(nbytes, align, f"b{i}")
        p = a.ptr(f"b{i}")
        assert v.numel() == nbytes and v.dtype == torch.uint8
        assert p % align == 0 and p % (2 * align) != 0, (align, p)
        if nbytes:
            assert v.data_ptr() == p


def test_red_zones_surround_every_view():
    a = _arena(0x00)
    spans = sorted(a.views.values())
    assert spans[0][0] >= RED_ZONE
    for (o0, n0), (o1, _) in zip(spans, spans[1:]):
        assert o1 - (o0 + n0) >= RED_ZONE
    assert a.buf.numel() - (spans[-1][0] + spans[-1][1]) >= RED_ZONE
    assert RED_ZONE >= 4 * 1024 * 16                                      # 4 x one 1024-lane workgroup at 16 B per lane
    with pytest.raises(MemoryError):
        a.take(CAP, 16, "too_big")


def test_put_write_read_round_trip():
    a = Arena(torch, "cpu", "ramp", capacity=CAP)
    x = np.arange(1, 38, dtype=np.uint32)
    a.put("d_u", x, 16)
    assert np.array_equal(a.read("d_u", np.uint32), x) and a.check() == []
    a.write("d_u", x[::-1])
    assert np.array_equal(a.read("d_u", np.uint32, 3), x[::-1][:3])
    a.put("empty", np.zeros(0, np.uint32), 16)
    assert a.read("empty", np.uint32).size == 0 and a.ptr("empty") % 16 == 0
