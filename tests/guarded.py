"""Guarded output buffers and poisoned, padded input rows for the buffer-contract tests (tests/test_buffer_contracts.py).

The value tests of this suite hand every entry point exactly sized, zero-filled outputs and densely packed inputs.  The
helpers here take both away: an output is an interior view of one larger allocation whose every byte -- guards and
interior -- starts as a canary, and an input row sits at a caller-chosen stride and base offset with everything that
is not input filled with the values a kernel that reads too far would notice most.

Plain module (no fixtures, no pytest settings); the CPU self-test is tests/test_guarded_helper.py.
"""
import numpy as np

CANARIES = (0xA5, 0x3C)  # every "fully written?" check runs once with each: a canary that happens to be the answer cannot hide
MIN_GUARD = 4096


def _index_of(off_bytes, shape, itemsize):
    """byte offset relative to the interior -> 'record r, row w, column c' of a C-ordered array of `shape` (the first
    index is not bounded: offsets in the back guard name record B, B + 1, ...; in the front guard they are negative)"""
    elem = off_bytes // itemsize
    idx = []
    for n in reversed(shape[1:]):
        elem, r = divmod(elem, n)
        idx.append(r)
    idx.append(elem)
    names = ("record", "row", "column")
    idx = idx[::-1]
    if len(idx) <= 3:
        return ", ".join(f"{names[i + 3 - len(idx)] if len(idx) > 1 else 'element'} {v}" for i, v in enumerate(idx))  # 1-D: element
    return "index " + str(tuple(idx))


class GuardedOut:
    """ONE flat allocation [front guard | interior | back guard], all of it canary bytes.  `view` (host) / `ptr` (both) address
    the interior, whose first byte is 16-byte aligned.  device None: numpy; else a torch device string."""

    def __init__(self, name, shape, dtype, canary, guard_bytes, device=None):
        self.name, self.shape, self.dtype = name, tuple(int(s) for s in shape), np.dtype(dtype)
        self.canary, self.device = int(canary) & 0xFF, device
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        guard = (max(int(guard_bytes), MIN_GUARD) + 15) // 16 * 16
        total = guard + self.nbytes + guard + 16
        if device is None:
            self.flat = np.full(total, self.canary, np.uint8)
            base = self.flat.ctypes.data
        else:
            import torch
            self.flat = torch.full((total,), self.canary, dtype=torch.uint8, device=device)
            base = self.flat.data_ptr()
        self.lo = guard + (-(base + guard)) % 16
        self.hi = self.lo + self.nbytes
        self.ptr = base + self.lo
        assert self.ptr % 16 == 0 and self.lo >= guard and total - self.hi >= guard
        self.view = None if device is not None else self.flat[self.lo:self.hi].view(self.dtype).reshape(self.shape)

    def _host_bytes(self):
        return self.flat if self.device is None else self.flat.cpu().numpy()

    def interior(self):
        """the interior as a numpy array of the requested dtype and shape (a copy)"""
        return self._host_bytes()[self.lo:self.hi].copy().view(self.dtype).reshape(self.shape)

    def _where(self, off):
        where = _index_of(off, self.shape, self.dtype.itemsize)
        if self.dtype.names:  # a record type: name the field the byte belongs to
            at = off % self.dtype.itemsize
            for f in self.dtype.names:
                sub, o = self.dtype.fields[f][:2]
                if o <= at < o + sub.itemsize:
                    where += f", field {f} + {at - o}"
        return where

    def check(self):
        """both guards still hold the canary; otherwise the first and last modified byte, relative to the interior"""
        raw = self._host_bytes()
        for what, a, b in (("front", 0, self.lo), ("back", self.hi, len(raw))):
            bad = np.nonzero(raw[a:b] != self.canary)[0]
            if len(bad):
                first, last = int(bad[0]) + a - self.lo, int(bad[-1]) + a - self.lo
                raise AssertionError(
                    f"buffer {self.name} {self.shape}: {what} guard modified, bytes {first}..{last} relative to the interior "
                    f"({len(bad)} bytes; first = {self._where(first)}, last = {self._where(last)}; the interior is "
                    f"{self.nbytes} bytes)")
        return True

    def check_equals(self, expected, ignore=None):
        """guards intact and the interior equal to `expected` byte for byte.  ignore: boolean byte mask [nbytes] of bytes the
        contract leaves undefined (must be stated by the caller's test)."""
        self.check()
        exp = np.ascontiguousarray(expected)
        assert exp.nbytes == self.nbytes, (self.name, exp.nbytes, self.nbytes)
        got = self._host_bytes()[self.lo:self.hi]
        diff = got != exp.view(np.uint8).reshape(-1)
        if ignore is not None:
            diff &= ~ignore
        bad = np.nonzero(diff)[0]
        if len(bad):
            first, last = int(bad[0]), int(bad[-1])
            still = int((got[bad] == self.canary).sum())
            raise AssertionError(
                f"buffer {self.name} {self.shape}: interior differs from the oracle in {len(bad)} bytes, {first}..{last} "
                f"(first = {self._where(first)}, last = {self._where(last)}); {still} of them still hold the canary "
                f"0x{self.canary:02X} (never written); got {got[first:first + 8].tolist()} want "
                f"{exp.view(np.uint8).reshape(-1)[first:first + 8].tolist()}")
        return True

    def check_untouched(self):
        """guards AND interior still hold the canary (a refused call writes nothing)"""
        self.check()
        bad = np.nonzero(self._host_bytes()[self.lo:self.hi] != self.canary)[0]
        if len(bad):
            raise AssertionError(f"buffer {self.name} {self.shape}: interior written at bytes {int(bad[0])}..{int(bad[-1])} "
                                 f"({self._where(int(bad[0]))}) by a call that must write nothing")
        return True


def guarded_out(shape, dtype, canary, guard_bytes, device=None, name="out"):
    return GuardedOut(name, shape, dtype, canary, guard_bytes, device)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _alternating(n, first, other):
    out = np.empty(n, np.uint16)
    out[0::2] = first
    out[1::2] = other
    return out


def padded_rows(rows_u16, stride, lead=0, tail=0, poison="adc"):
    """rows [B, buf_len] -> one flat uint16 allocation of lead + B*stride + tail samples, row b at lead + b*stride; every
    sample that is not rows[b][:buf_len] is poison:
      "adc"   the loudest thing a 12-bit converter produces, alternating 0 / 4095, the phase of every gap chosen so that
              the sample right after a row (and the one right before row 0) is far from its real neighbour;
      "ffff"  constant 0xFFFF words (outside the 12-bit range);
      "s16"   alternating +32767 / -32768 (s16 feature rows)."""
    rows = np.ascontiguousarray(rows_u16).view(np.uint16)
    B, n = rows.shape
    assert stride >= n
    flat = np.empty(lead + B * stride + tail, np.uint16)

    def fill(a, b, neighbour, at_end=False):
        if b <= a:
            return
        if poison == "ffff":
            flat[a:b] = 0xFFFF
            return
        hi, lo = (0x7FFF, 0x8000) if poison == "s16" else (4095, 0)
        far = lo if (int(neighbour) < 0x8000 if poison == "s16" else int(neighbour) >= 2048) else hi
        g = _alternating(b - a, far, hi + lo - far)
        flat[a:b] = g[::-1] if at_end else g  # at_end: the LAST sample of the gap is the one next to the neighbour

    fill(0, lead, rows[0, 0], at_end=True)
    for b in range(B):
        a = lead + b * stride
        flat[a:a + n] = rows[b]
        fill(a + n, a + stride if b + 1 < B else len(flat), rows[b, n - 1])
    return flat


def poison_feature_rows(rec, frames):
    """rec int16 [B, R, nc]: every row >= frames[b] of record b becomes alternating +32767 / -32768 (in place); returns rec"""
    B, R, nc = rec.shape
    pat = _alternating(R * nc, 0x7FFF, 0x8000).view(np.int16).reshape(R, nc)
    for b in range(B):
        rec[b, int(frames[b]):] = pat[int(frames[b]):]
    return rec


# ---- every DTW form (moved unchanged from tests/test_gpu_parity.py) ---------------------------------------------------------
def _dtw_all_modes(eng, im, inf):
    """sr_dtw_batch with the batch kernels (small-launch mode 1), with one workgroup per pair wherever the band fits
    (mode 2, k_dtw_cells), with four lanes per pair (mode 3, k_dtw_quad), in the automatic mode and with k_dtw_cells' literal
    fallback forced: scores and results must be the same bytes; returns the first"""
    from stm32_speech_recognition_amd.engine import dev_hook
    eng.set_small_launch(1)
    sc, res = eng.dtw(im, inf)
    for mode in (2, 3, 0):
        eng.set_small_launch(mode)
        sc2, res2 = eng.dtw(im, inf)
        assert np.array_equal(sc, sc2), mode
        assert res.tobytes() == res2.tobytes(), mode
    # k_dtw_cells' fallback for walks that leave dtw_limit's band (a step with all three candidates outside): the literal
    # walk on the staged rows, forced for every pair by the development hook -- which exists only in the -DSR_TESTING build
    # of the library, so an engine with the same configuration and store is opened there
    et = eng.clone(testing=True)
    dev_hook("cells_literal", 1)
    try:
        et.set_small_launch(2)
        sc3, res3 = et.dtw(im, inf)
    finally:
        dev_hook("cells_literal", 0)
        et.close()
        eng.set_small_launch(0)
    assert np.array_equal(sc, sc3) and res.tobytes() == res3.tobytes()
    return sc, res
