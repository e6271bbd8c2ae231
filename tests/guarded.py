"""A guarded arena for calling the C entries of libfcpp.so on buffers whose surroundings are watched (a helper, not a test file).

The suite's other tests hand every operator outputs that torch.empty sized exactly: a store past the end lands in the allocator's 512-byte
rounding or in a neighbour, an element that is never written may still hold the right value of an earlier call, and every pointer is
512-byte aligned.  An Arena carves named slots out of ONE uint8 buffer -- a numpy array for the host twins (fcpp_debug_*), a torch CUDA
tensor for the device entries -- so that all three show:

  layout     every slot has at least GUARD = 256 bytes of guard in front of it and behind it.  256 is a condition, not a measurement: more
             than one 64-lane row of int8 and more than 16 doubles, so a write that is off by a few elements or by one wavefront row of a
             narrow type lands in a guard.
  alignment  a slot starts at an ADDRESS that is a multiple of its element size and deliberately no multiple of 16: = 8 (mod 16) for 8-byte
             types, = 4 (mod 8) for 4-byte types, odd for bytes -- what a C caller's naturally aligned pointers may look like.
  fill       guards hold the byte 0xA5, output slots 0x5A in every byte, input slots a copy of the input.
  check      after the call (and a synchronise): every guard byte is still 0xA5; every input slot has the bits that were put in; every
             output slot has the bits of expected[name]; a slot declared written=False is still all 0x5A; and no ELEMENT of expected[name]
             is the all-0x5A pattern, so "still pre-filled" and "correct" exclude each other (a condition on the inputs the caller chose).
  in-out     a slot the call reads and writes (inout): pre-filled with the input and checked against expected[name] like an output; an
             expected element may be the all-0x5A pattern only where the input element is that very value.
  mask       an output the call may write only in part (the connector rows of fields without a kept point, the unused tail of a corner's
             row): a boolean mask of the elements it must leave alone, given to output() or to check().  Those must still hold the pre-fill;
             all the others are checked as ever, the pre-fill rule included.
An output passed as NULL has no slot.  Failures raise GuardError (an AssertionError) whose message names the slot.
"""
import ctypes as C

import numpy as np

GUARD = 256
GUARD_BYTE = 0xA5
FILL_BYTE = 0x5A


class GuardError(AssertionError):
    pass


class _Slot:
    def __init__(self, name, dtype, count, data, written, inout=False, keep=None):
        self.name, self.dtype, self.count, self.data, self.written = name, np.dtype(dtype), int(count), data, written
        self.inout = inout          # data = the input the slot is pre-filled with; checked like an output
        self.keep = keep            # bool per element of an output: True = the call must leave it alone (None: it writes them all)
        self.start = self.end = -1

    @property
    def nbytes(self):
        return self.count * self.dtype.itemsize


def _as_bytes(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1).view(np.uint8)


class Arena:
    """declare the slots (input / output), build() on the host or on a device, call the entry with ptr(name), then check(expected)"""

    def __init__(self):
        self._slots = {}
        self._image = None          # the host buffer, or the host image the device buffer was made from
        self._dev = None            # the torch tensor of a device arena
        self._base = 0

    # ---- declaration ----------------------------------------------------------------------------------------------------------------
    def _add(self, slot):
        if self._image is not None:
            raise ValueError('the arena is built')
        if slot.name in self._slots:
            raise ValueError('slot %r declared twice' % slot.name)
        if slot.dtype.itemsize not in (1, 2, 4, 8):
            raise ValueError('slot %r: element size %d' % (slot.name, slot.dtype.itemsize))
        self._slots[slot.name] = slot
        return self

    def input(self, name, array, dtype=None):
        a = np.ascontiguousarray(array, dtype=dtype)
        return self._add(_Slot(name, a.dtype, a.size, _as_bytes(a, a.dtype).copy(), False))

    def inout(self, name, array, dtype=None):
        """a slot the call reads AND writes: pre-filled with the input, checked against expected[name]"""
        a = np.ascontiguousarray(array, dtype=dtype)
        return self._add(_Slot(name, a.dtype, a.size, _as_bytes(a, a.dtype).copy(), True, inout=True))

    def output(self, name, dtype, count, written=True, keep=None):
        """written=False: a slot the call is handed (or not) and must leave alone; keep: a boolean mask, one entry per element, of the
        elements the call must leave alone (check(keep=...) may bring it instead, when only the call's results tell)"""
        n = int(np.prod(count))
        return self._add(_Slot(name, dtype, n, None, written, keep=self._mask(name, keep, n)))

    @staticmethod
    def _mask(name, keep, count):
        if keep is None:
            return None
        m = np.ascontiguousarray(keep).reshape(-1)
        if m.dtype != np.bool_ or m.size != count:
            raise ValueError('slot %r: the mask is %s x %d, the slot has %d elements' % (name, m.dtype, m.size, count))
        return m.copy()

    # ---- layout ---------------------------------------------------------------------------------------------------------------------
    def build(self, device=None):
        """device=None: a numpy buffer (host pointers); else a torch device: the same layout in one CUDA tensor"""
        at = 0
        for s in self._slots.values():
            at += GUARD
            size = s.dtype.itemsize
            at += (size - at) % (2 * size)          # at = size (mod 2 size): a multiple of the element size, never of 16
            s.start, s.end = at, at + s.nbytes
            at = s.end
        total = at + GUARD
        room = np.empty(total + 16, dtype=np.uint8)
        image = room[(-room.ctypes.data) % 16:][:total]          # the layout's residues are those of the addresses: a 16-byte aligned base
        image[:] = GUARD_BYTE
        for s in self._slots.values():
            image[s.start:s.end] = FILL_BYTE if s.data is None else s.data
        self._image = image
        if device is None:
            self._base = image.ctypes.data
        else:
            import torch
            self._dev = torch.from_numpy(image).to(device)
            self._base = self._dev.data_ptr()
        if self._base % 16:
            raise GuardError('the arena buffer itself is not 16-byte aligned')
        for s in self._slots.values():
            addr, size = self._base + s.start, s.dtype.itemsize
            assert addr % size == 0 and addr % (2 * size) == size and addr % 16 != 0, s.name
        return self

    def address(self, name):
        return self._base + self._slots[name].start

    def ptr(self, name):
        """the slot's address for ctypes; a name that was not declared is a NULL pointer (an output the call is not asked for)"""
        return C.c_void_p(self.address(name)) if name in self._slots else None

    def span(self, name):
        s = self._slots[name]
        return s.start, s.end

    @property
    def raw(self):
        """the bytes of a host arena (guards included)"""
        if self._dev is not None:
            raise ValueError('a device arena has no host bytes: use snapshot()')
        return self._image

    def view(self, name):
        """a host arena's slot as an array of its type"""
        s = self._slots[name]
        return self.raw[s.start:s.end].view(s.dtype)

    def snapshot(self):
        if self._dev is None:
            return self._image
        import torch
        torch.cuda.synchronize(self._dev.device)
        return self._dev.cpu().numpy()

    def read(self, name, image=None):
        s = self._slots[name]
        image = self.snapshot() if image is None else image
        return image[s.start:s.end].copy().view(s.dtype)

    # ---- the check ------------------------------------------------------------------------------------------------------------------
    def check(self, expected, keep=None):
        """expected: {name: array} for exactly the written output slots and the in-out slots.  keep: {name: boolean mask} of elements of
        written output slots that the call must leave alone (in place of a mask given to output(); what expected[name] holds there is not
        looked at).  -> {name: array} of what the slots hold"""
        img = self.snapshot()
        slots = list(self._slots.values())
        outputs = {s.name for s in slots if s.inout or (s.data is None and s.written)}
        if set(expected) != outputs:
            raise GuardError('expected values for %s, written output slots %s' % (sorted(expected), sorted(outputs)))
        masks = {s.name: s.keep for s in slots if s.keep is not None}
        for name, m in (keep or {}).items():
            s = self._slots.get(name)
            if s is None or s.inout or s.data is not None or not s.written:
                raise GuardError('a mask for %r, which is no written output slot' % name)
            masks[name] = self._mask(name, m, s.count)
        # 1: the guards
        guard = np.ones(len(img), dtype=bool)
        for s in slots:
            guard[s.start:s.end] = False
        hit = np.flatnonzero(guard & (img != GUARD_BYTE))
        if hit.size:
            msgs = []
            for pos in hit[:8]:
                before = [s for s in slots if s.end <= pos]
                after = [s for s in slots if s.start > pos]
                where = []
                if before:
                    where.append('%d bytes behind the end of slot %r' % (pos - before[-1].end, before[-1].name))
                if after:
                    where.append('%d bytes in front of slot %r' % (after[0].start - pos, after[0].name))
                msgs.append('byte %d (%s) holds 0x%02X' % (pos, ', '.join(where), img[pos]))
            raise GuardError('%d guard bytes were written: %s' % (hit.size, '; '.join(msgs)))
        got = {}
        for s in slots:
            have = img[s.start:s.end]
            if s.data is not None and not s.inout:
                # 2: the inputs
                bad = np.flatnonzero(have != s.data)
                if bad.size:
                    raise GuardError('input slot %r was written: %d bytes differ, the first in element %d' % (s.name, bad.size, bad[0] // s.dtype.itemsize))
                continue
            if not s.written:
                bad = np.flatnonzero(have != FILL_BYTE)
                if bad.size:
                    raise GuardError('slot %r must not be written: %d bytes differ from the pre-fill, the first in element %d'
                                     % (s.name, bad.size, bad[0] // s.dtype.itemsize))
                continue
            # 3, 4: the outputs
            e = np.asarray(expected[s.name])
            if e.dtype != s.dtype or e.size != s.count:
                raise GuardError('expected[%r]: %s x %d, the slot holds %s x %d' % (s.name, e.dtype, e.size, s.dtype, s.count))
            want = _as_bytes(e, s.dtype)
            size = s.dtype.itemsize
            is_fill = (want.reshape(-1, size) == FILL_BYTE).all(axis=1)
            if s.inout:          # (an element the call may leave as it was put in)
                is_fill &= (want.reshape(-1, size) != s.data.reshape(-1, size)).any(axis=1)
            differ = (have.reshape(-1, size) != want.reshape(-1, size)).any(axis=1)
            kept = masks.get(s.name)
            if kept is not None:          # (the elements the call must leave alone: still the pre-fill, whatever expected[name] holds there)
                touched = np.flatnonzero(kept & (have.reshape(-1, size) != FILL_BYTE).any(axis=1))
                if touched.size:
                    k = int(touched[0])
                    raise GuardError('output slot %r: %d of the %d elements the call must leave alone were written, the first element %d: %r'
                                     % (s.name, touched.size, int(kept.sum()), k, have.view(s.dtype)[k:k + 1].tolist()))
                is_fill &= ~kept
                differ &= ~kept
            prefilled = np.flatnonzero(is_fill)
            if prefilled.size:
                raise GuardError('expected[%r][%d] is the pre-fill pattern itself: choose other inputs' % (s.name, prefilled[0]))
            bad = np.flatnonzero(differ)
            if bad.size and s.inout:
                k = int(bad[0])
                untouched = int((have.reshape(-1, size)[bad] == s.data.reshape(-1, size)[bad]).all(axis=1).sum())
                raise GuardError('in-out slot %r: %d of %d elements differ (%d of them still the input), the first element %d: %r, expected %r'
                                 % (s.name, bad.size, s.count, untouched, k, have.view(s.dtype)[k:k + 1].tolist(), want.view(s.dtype)[k:k + 1].tolist()))
            if bad.size:
                k = int(bad[0])
                untouched = int((have.reshape(-1, size)[bad] == FILL_BYTE).all(axis=1).sum())
                raise GuardError('output slot %r: %d of %d elements differ (%d of them still pre-filled), the first element %d: %r, expected %r'
                                 % (s.name, bad.size, s.count, untouched, k, have.view(s.dtype)[k:k + 1].tolist(), want.view(s.dtype)[k:k + 1].tolist()))
            got[s.name] = have.copy().view(s.dtype)
        return got
