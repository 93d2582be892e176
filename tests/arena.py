"""A guarded arena (TEST INFRASTRUCTURE): one uint8 allocation laid out as [front guard | payload | back guard].

The payload is handed out as a DeviceArray over a view of the allocation, so a kernel that is given it runs on memory whose
neighbourhood the test owns: a store past either end of the payload lands in a guard and `check()` finds it; with the guards
holding NaN (`fill='nan'`) a load past either end that reaches an output makes that output NaN.  GPU address sanitizers are
not available to this suite; this is what it has instead.

Each guard is at least GUARD_MIN bytes and at least GUARD_LINES lines of the array (`line` elements each; the longest axis
unless given) -- 32 lines is the largest tile of any pass kernel, so a whole stray tile lands inside the guard, never beyond
the allocation.  The guards hold seeded, non-constant bytes, so a stray store of zeros, of NaN or of data shows.  Works on a
host tensor too (tests/test_arena_host.py holds the mechanism without a device)."""
import numpy as np
import torch

GUARD_MIN = 1 << 20
GUARD_LINES = 32
ALIGN = 256
_PATTERNS = {}


def _pattern(nbytes, seed):
    """`nbytes` seeded random bytes (cached: the arenas of a test session share them)."""
    key = (nbytes, seed)
    if key not in _PATTERNS:
        _PATTERNS[key] = np.random.default_rng(seed).integers(0, 256, size=nbytes, dtype=np.uint8)
    return _PATTERNS[key]


class GuardError(AssertionError):
    pass


class Arena:
    """arena.array: the payload, a DeviceArray(shape, dtype) that starts `offset_elems` elements past a 256-byte boundary.
    fill = 'bytes': both guards hold random bytes; 'nan': they hold NaN in the payload's real type (every whole real that fits
    between the allocation's edge and the payload, random bytes in what is left), for the input side of a dependence check."""
    def __init__(self, shape, dtype, fill='bytes', offset_elems=0, line=None, seed=20240, device=None):
        from mpi4py_fft_amd.array import DeviceArray, default_device, torch_dtype
        assert fill in ('bytes', 'nan'), fill
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.dtype = np.dtype(dtype)
        item = self.dtype.itemsize
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * item
        line = max(self.shape) if line is None else int(line)
        self.guard = max(GUARD_MIN, GUARD_LINES * line * item)
        dev = default_device() if device is None else torch.device(device)
        # (the allocation's own base need not be 256-byte aligned on every allocator: ALIGN bytes of slack place the payload)
        raw = -(-self.guard // ALIGN) * ALIGN + ALIGN + int(offset_elems) * item + self.nbytes + self.guard
        self.buf = torch.empty(raw, dtype=torch.uint8, device=dev)
        base = self.buf.data_ptr()
        self.start = -(-(base + self.guard) // ALIGN) * ALIGN - base + int(offset_elems) * item       # payload's first byte
        self.end = self.start + self.nbytes
        assert self.guard <= self.start and self.end + self.guard <= raw
        assert (base + self.start - int(offset_elems) * item) % ALIGN == 0
        host = _pattern(raw, seed).copy()
        if fill == 'nan':
            rdt = np.dtype('f4' if self.dtype.char in 'fF' else 'f8')
            k = self.start // rdt.itemsize
            host[self.start - k * rdt.itemsize:self.start].view(rdt)[:] = np.nan
            k = (raw - self.end) // rdt.itemsize
            host[self.end:self.end + k * rdt.itemsize].view(rdt)[:] = np.nan
        self.fill = host
        self.buf.copy_(torch.from_numpy(host))
        view = self.buf[self.start:self.end].view(torch_dtype(self.dtype)).reshape(self.shape)
        self.array = DeviceArray(self.shape, self.dtype, tensor=view)
        assert self.array.data_ptr == base + self.start and self.array.is_contiguous()

    def damage(self):
        """[(side, first, last, count)] of the guards that no longer hold their fill: byte offsets of the first and the last
        differing byte RELATIVE TO THE PAYLOAD -- negative in the front guard (-1 is the byte before the payload), counted from
        the payload's end in the back guard (0 is the first byte behind it) -- and the number of differing bytes."""
        if self.buf.is_cuda:
            torch.cuda.synchronize(self.buf.device)
        now = self.buf.cpu().numpy()
        out = []
        for side, lo, hi, origin in (('front', 0, self.start, self.start), ('back', self.end, now.size, self.end)):
            bad = np.flatnonzero(now[lo:hi] != self.fill[lo:hi])
            if bad.size:
                out.append((side, int(bad[0]) + lo - origin, int(bad[-1]) + lo - origin, int(bad.size)))
        return out

    def check(self, what=''):
        """Both guards bit for bit against their fill; GuardError (an AssertionError) names side, extent and count."""
        found = self.damage()
        if found:
            raise GuardError('%s: %s' % (what, '; '.join('%s guard of the %s %s payload: %d bytes differ, offsets %d ... %d'
                                                         % (side, self.shape, self.dtype.char, count, first, last)
                                                         for side, first, last, count in found)))

    def payload_bytes(self):
        """The payload as host bytes (whatever it holds, NaN payloads and zero signs included)."""
        return self.buf[self.start:self.end].cpu().numpy()
