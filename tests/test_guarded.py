"""The guarded arena of the buffer-contract tests (tests/guarded.py) on the
CPU: its layout, the natural-only alignment of misalign=True, and that planted
damage is found and reported against the right view with the right distance.
This is how the detector is proven; no broken kernel is ever built or run."""
import numpy as np
import pytest
import torch

from guarded import ALIGN, GUARD, Arena

CPU = torch.device("cpu")
DTYPES = [(torch.uint8, 1), (torch.int32, 4), (torch.int64, 8), (torch.float64, 8)]


def three_views(poison=0xA5, misalign=False):
    a = Arena(CPU, poison, nbytes=1 << 16)
    node = a.alloc((3, 65), torch.int32, misalign, name="node")
    status = a.alloc((3, 65), torch.uint8, misalign, name="status")
    done = a.alloc((3, 65), torch.int64, misalign, name="done")
    return a, node, status, done


@pytest.mark.parametrize("poison", [0xA5, 0x5A])
def test_layout_and_clean_check(poison):
    a, node, status, done = three_views(poison)
    base = a.buf.data_ptr()
    assert [v.name for v in a.views] == ["node", "status", "done"]
    assert [v.nbytes for v in a.views] == [3 * 65 * 4, 3 * 65, 3 * 65 * 8]
    for t, v in zip((node, status, done), a.views):
        assert t.is_contiguous() and t.data_ptr() == base + v.offset and t.data_ptr() % ALIGN == 0
        assert bool((t.view(-1).view(torch.uint8) == poison).all())  # outputs start out poisoned
    # every view has GUARD bytes of its own on both sides
    assert a.views[0].offset >= GUARD and a.views[-1].end + GUARD <= a.buf.numel()
    for p, n in zip(a.views, a.views[1:]):
        assert n.offset - p.end >= 2 * GUARD
    assert int(a.inside.sum()) == sum(v.nbytes for v in a.views)
    a.check()
    node.fill_(7)
    status.fill_(5)
    done.fill_(-1)
    a.check()  # writes inside the views are no damage
    with pytest.raises(MemoryError):
        a.alloc(1 << 16, torch.uint8)


def test_band_values_are_refusable_inputs():
    """What a kernel would read from a band: negative under 0xA5, huge under 0x5A."""
    a5 = Arena(CPU, 0xA5, nbytes=3 * GUARD).buf
    assert int(a5[:8].view(torch.int64)[0]) < 0 and int(a5[:4].view(torch.int32)[0]) < 0
    assert float(a5[:8].view(torch.float64)[0]) < 0
    p5 = Arena(CPU, 0x5A, nbytes=3 * GUARD).buf
    assert int(p5[:8].view(torch.int64)[0]) > 2**61 and int(p5[:4].view(torch.int32)[0]) > 10**9


@pytest.mark.parametrize("dtype,size", DTYPES)
def test_misalign_is_natural_alignment_and_no_more(dtype, size):
    a = Arena(CPU, 0xA5, nbytes=1 << 16)
    for k in range(3):
        t = a.alloc((5, 13), dtype, misalign=True, name=f"v{k}")
        assert t.data_ptr() % ALIGN == size  # 256 k + itemsize
        assert t.data_ptr() % size == 0 and t.data_ptr() % (2 * size) != 0
        assert t.element_size() == size and t.is_contiguous()
    a.check()


def test_fill_and_put_copy_exactly():
    a = Arena(CPU, 0x5A, nbytes=1 << 16)
    x = np.arange(3 * 7, dtype=np.int64).reshape(3, 7) - 5
    v = a.put(x, misalign=True, name="x")
    np.testing.assert_array_equal(v.numpy(), x)
    w = a.alloc((3, 7), torch.int32, name="w")
    with pytest.raises(TypeError):
        a.fill(w, x)  # int64 into int32: refused, not converted
    with pytest.raises(TypeError):
        a.fill(w, np.zeros((7, 3), np.int32))
    a.check()


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("where,view,dist,text", [
    ("before", "status", -1, "'status' overran before its start by 1 element(s): first damaged byte at -1 "),
    ("after", "node", +1, "'node' overran past its end by 1 element(s): first damaged byte at +1 "),
    ("far", "done", +4095, "'done' overran past its end by 512 element(s): first damaged byte at +4095 "),
    ("far_before", "done", -4095, "'done' overran before its start by 512 element(s): first damaged byte at -4095 "),
])
def test_planted_damage_is_reported(where, view, dist, text, misalign):
    a, node, status, done = three_views(0xA5, misalign)
    v = {x.name: x for x in a.views}[view]
    i = v.offset + dist if dist < 0 else v.end - 1 + dist
    assert not bool(a.inside[i])
    a.buf[i] = 0x00
    msg = a.damage()
    assert msg is not None and text in msg, msg
    assert f"arena byte {i}," in msg and "1 damaged byte(s)" in msg
    with pytest.raises(AssertionError, match=f"'{view}' overran"):
        a.check()
    a.buf[i] = 0xA5  # repaired: clean again
    a.check()


def test_damage_equal_to_the_other_poison_is_seen():
    a, node, status, done = three_views(0x5A)
    a.buf[a.views[0].end] = 0xA5
    assert "'node' overran past its end by 1 element(s)" in a.damage()
