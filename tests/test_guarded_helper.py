"""CPU self-test of tests/guarded.py: a checker that cannot fail is worth nothing.  One byte written into the front guard,
one into the back guard and one missing write in the interior are each reported with buffer name and offset; an untouched
guard with a fully written interior passes; padded_rows puts the rows where it says and poison everywhere else."""
import numpy as np
import pytest

from guarded import CANARIES, MIN_GUARD, guarded_out, padded_rows, poison_feature_rows


def _filled(canary, shape=(5, 7, 12), dtype=np.int16, guard=100):
    g = guarded_out(shape, dtype, canary, guard, name="d_mfcc")
    want = (np.arange(np.prod(shape)) % 251 + 1).astype(dtype).reshape(shape)
    g.view[...] = want
    return g, want


@pytest.mark.parametrize("canary", CANARIES)
def test_untouched_guards_and_written_interior_pass(canary):
    g, want = _filled(canary)
    assert g.ptr % 16 == 0 and g.lo >= MIN_GUARD and len(g.flat) - g.hi >= MIN_GUARD
    assert g.check() and g.check_equals(want)
    assert np.array_equal(g.interior(), want)
    fresh = guarded_out((3, 4), np.uint32, canary, 64, name="d_scores")
    assert fresh.check_untouched()
    assert (fresh.interior().view(np.uint8) == canary).all()


@pytest.mark.parametrize("canary", CANARIES)
def test_one_byte_in_the_front_guard_is_reported(canary):
    g, want = _filled(canary)
    g.flat[g.lo - 1] ^= 0xFF
    with pytest.raises(AssertionError, match=r"d_mfcc .*front guard modified, bytes -1\.\.-1 "):
        g.check()
    with pytest.raises(AssertionError, match="front guard"):
        g.check_equals(want)
    g.flat[g.lo - 1] ^= 0xFF
    g.flat[0] ^= 1  # the far end of the guard counts too
    with pytest.raises(AssertionError, match=r"front guard modified, bytes -%d\.\.-%d " % (g.lo, g.lo)):
        g.check()


@pytest.mark.parametrize("canary", CANARIES)
def test_one_byte_in_the_back_guard_is_reported_with_its_record(canary):
    g, want = _filled(canary)
    rec = 7 * 12 * 2
    g.flat[g.hi + rec + 3] ^= 0xFF  # record B + 1 = 6, row 0, column 1 (byte 3)
    with pytest.raises(AssertionError, match=r"back guard modified, bytes %d\.\.%d .*record 6, row 0, column 1" % (6 * rec + 3, 6 * rec + 3)):
        g.check()
    g.flat[g.hi + rec + 3] ^= 0xFF
    g.flat[g.hi] ^= 0x10  # the byte right after the interior: record B
    with pytest.raises(AssertionError, match=r"bytes %d\.\.%d .*record 5, row 0, column 0" % (5 * rec, 5 * rec)):
        g.check_equals(want)


@pytest.mark.parametrize("canary", CANARIES)
def test_a_missing_write_in_the_interior_is_reported(canary):
    g, want = _filled(canary)
    g.view[3, 6, :] = np.frombuffer(bytes([canary, canary]), np.int16)[0]  # the kernel "forgot" the last row of record 3
    off = ((3 * 7 + 6) * 12) * 2
    with pytest.raises(AssertionError, match=r"d_mfcc .*interior differs .* %d\.\.%d .*record 3, row 6, column 0.*24 of them still hold the canary" % (off, off + 23)):
        g.check_equals(want)
    # with the other canary the same forgotten row is still wrong: no canary value can stand in for the answer twice
    other = CANARIES[1 - CANARIES.index(canary)]
    g2, _ = _filled(other)
    g2.view[3, 6, :] = np.frombuffer(bytes([other, other]), np.int16)[0]
    with pytest.raises(AssertionError, match="interior differs"):
        g2.check_equals(want)
    # a refused call must leave the interior alone
    g3 = guarded_out((4,), np.uint32, canary, 16, name="status")
    g3.view[2] = 0
    with pytest.raises(AssertionError, match=r"status .*interior written at bytes 8\.\.11 \(element 2\)"):
        g3.check_untouched()


def test_ignore_mask_excludes_exactly_the_named_bytes():
    g, want = _filled(CANARIES[0])
    g.view[0, 0, 0] = want[0, 0, 0] + 1
    mask = np.zeros(g.nbytes, bool)
    mask[0:2] = True
    assert g.check_equals(want, ignore=mask)
    g.view[0, 0, 1] = want[0, 0, 1] + 1
    with pytest.raises(AssertionError, match="record 0, row 0, column 1"):
        g.check_equals(want, ignore=mask)


@pytest.mark.parametrize("poison", ["adc", "ffff"])
@pytest.mark.parametrize("lead,stride,tail", [(0, 24, 0), (8, 32, 16), (1, 21, 5), (4104, 24 + 4104, 4104)])
def test_padded_rows_layout_and_poison(poison, lead, stride, tail):
    rng = np.random.default_rng(lead + stride)
    rows = rng.integers(0, 4096, (5, 21)).astype(np.uint16)
    flat = padded_rows(rows, stride, lead, tail, poison)
    assert flat.dtype == np.uint16 and len(flat) == lead + 5 * stride + tail
    mask = np.ones(len(flat), bool)
    for b in range(5):
        assert np.array_equal(flat[lead + b * stride:lead + b * stride + 21], rows[b])
        mask[lead + b * stride:lead + b * stride + 21] = False
    pad = flat[mask]
    if poison == "ffff":
        assert (pad == 0xFFFF).all()
        return
    assert np.isin(pad, (0, 4095)).all()
    for b in range(5):
        a = lead + b * stride + 21
        gap = flat[a:a + stride - 21] if b < 4 else flat[a:]
        if len(gap):  # the sample right after the row is the code farthest from the row's last one, then alternating
            assert gap[0] == (0 if rows[b, 20] >= 2048 else 4095)
            assert (gap[1:] != gap[:-1]).all()
    if lead:
        assert flat[lead - 1] == (0 if rows[0, 0] >= 2048 else 4095)


def test_poison_feature_rows():
    rec = np.arange(3 * 6 * 12, dtype=np.int16).reshape(3, 6, 12)
    keep = rec.copy()
    poison_feature_rows(rec, [0, 4, 6])
    assert np.isin(rec[0], (32767, -32768)).all() and np.array_equal(rec[2], keep[2])
    assert np.array_equal(rec[1, :4], keep[1, :4]) and np.isin(rec[1, 4:], (32767, -32768)).all()
    assert (rec[1, 4:].reshape(-1)[1:] != rec[1, 4:].reshape(-1)[:-1]).all()
    s16 = padded_rows(keep[2].reshape(1, -1).view(np.uint16), 80, 8, 8, "s16").view(np.int16)
    assert np.isin(s16[:8], (32767, -32768)).all() and np.array_equal(s16[8:80], keep[2].reshape(-1))
