"""Guarded device buffers for the per-kernel parity tests (tests/test_gpu_ops.py).

A fresh `torch.empty` from the caching allocator very often returns the block a previous case just freed -- with that case's
(correct) answer still in it -- and rounds its size up, so a kernel that skips a tile, never launches, or stores past the end of
its output can still pass.  Everything here makes those defects visible:

  guarded_out(shape, dtype)  one allocation: front guard | payload | back guard.  The guards hold a fixed seeded byte pattern,
                             the payload a sentinel bit pattern no kernel produces (a non-canonical NaN; uint8 outputs: a fill
                             byte chosen by the caller, run twice with 0x00 and 0xFF).  After the kernel: check_guards() (guards
                             bitwise intact), assert_written(region) (no sentinel left), isfinite -- all three via check().
  guarded_in(t)              a copy of an input between NaN guards: a read past its logical end that reaches a result shows up
                             as a NaN.  Padding that an input's contract defines as zero is part of the payload and stays zero.
  tile_err(got, ref, block)  the largest blockwise relative error: a ragged last tile 1 % off, or one wrong 32 x 32 block, is
                             invisible in a normwise error over a large tensor.

Works on any torch device (the CPU self-tests in test_guarded_helpers.py use device='cpu')."""
import torch
import torch.nn.functional as F

GUARD_MIN_BYTES = 64 * 1024
GUARD_ROWS = 256
GUARD_ALIGN = 256            # payload offset: keeps the 16-byte (and wider) alignment of the kernels' vector stores
LOCAL_TOL = 2e-3             # blockwise bound: fp16 storage costs at most 4.9e-4 per element, so 4x margin

# non-canonical (signalling) NaNs: arithmetic only ever produces the canonical quiet NaN, so a payload word that still holds
# one of these was never stored to
SENTINEL = {torch.float16: (torch.int16, 0x7D5A), torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5)}
_NAN_BITS = {torch.float16: (torch.int16, 0x7E00), torch.bfloat16: (torch.int16, 0x7FC0), torch.float32: (torch.int32, 0x7FC00000)}
_PATTERN_SEED = 0x5EED


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def guard_bytes(shape, dtype):
    """max(64 KiB, 256 rows of the last dimension), rounded up to a multiple of 256 bytes (a flat output's row: one element)"""
    row = (int(shape[-1]) if len(shape) >= 2 else 1) * _itemsize(dtype)
    g = max(GUARD_MIN_BYTES, GUARD_ROWS * row)
    return (g + GUARD_ALIGN - 1) // GUARD_ALIGN * GUARD_ALIGN


_patterns = {}


def _pattern(nbytes, seed, device):
    key = (nbytes, seed, str(device))
    if key not in _patterns:
        g = torch.Generator().manual_seed(seed)
        _patterns[key] = torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.uint8).to(device)
    return _patterns[key]


class GuardedOut:
    """Output buffer between two guards.  `t` is the logical output (shape, dtype) -- pass t.data_ptr() to the kernel."""

    def __init__(self, shape, dtype, device='cuda', fill=None):
        self.shape, self.dtype = tuple(int(s) for s in shape), dtype
        self.guard = guard_bytes(self.shape, dtype)
        self.nbytes = _numel(self.shape) * _itemsize(dtype)
        self.buf = torch.empty(2 * self.guard + self.nbytes, dtype=torch.uint8, device=device)
        self.front = _pattern(self.guard, _PATTERN_SEED, device)
        self.back = _pattern(self.guard, _PATTERN_SEED + 1, device)
        self.buf[:self.guard] = self.front
        self.buf[self.guard + self.nbytes:] = self.back
        payload = self.buf[self.guard:self.guard + self.nbytes]
        if dtype == torch.uint8:
            assert fill is not None, 'uint8 outputs have no spare bit pattern: run the kernel on a 0x00 and a 0xFF fill'
            self._ity, self._sent = torch.uint8, int(fill)
        else:
            assert fill is None and dtype in SENTINEL, dtype
            self._ity, self._sent = SENTINEL[dtype]
        payload.view(self._ity).fill_(self._sent)
        self.t = payload.view(dtype).view(self.shape)

    def data_ptr(self):
        return self.t.data_ptr()

    def _bits(self, region):
        b = self.buf[self.guard:self.guard + self.nbytes].view(self._ity).view(self.shape)
        return b if region is None else b[region]

    def check_guards(self):
        for side, lo, pat in (('front', 0, self.front), ('back', self.guard + self.nbytes, self.back)):
            bad = (self.buf[lo:lo + self.guard] != pat).nonzero()
            if bad.numel():
                first = int(bad[0])
                where = f'{self.guard - first} byte(s) before the payload' if side == 'front' else f'payload end + {first}'
                raise AssertionError(f'{side} guard damaged: {bad.numel()} byte(s), first at {where} '
                                     f'(output {self.shape} {self.dtype}, {self.nbytes} bytes)')

    def assert_written(self, region=None):
        left = self._bits(region) == self._sent
        if bool(left.any()):
            idx = left.nonzero()
            raise AssertionError(f'{idx.shape[0]} of {left.numel()} output element(s) never written, first at '
                                 f'{tuple(int(v) for v in idx[0])} of region {region} (output {self.shape})')

    def assert_untouched(self, region):
        """the region (e.g. padding the caller owns) must still hold the sentinel"""
        hit = self._bits(region) != self._sent
        if bool(hit.any()):
            idx = hit.nonzero()
            raise AssertionError(f'{idx.shape[0]} element(s) written outside the logical output, first at '
                                 f'{tuple(int(v) for v in idx[0])} of region {region} (output {self.shape})')

    def assert_finite(self, region=None):
        if self.dtype.is_floating_point:
            v = self.t if region is None else self.t[region]
            fin = torch.isfinite(v)
            if not bool(fin.all()):
                idx = (~fin).nonzero()
                raise AssertionError(f'{idx.shape[0]} non-finite output element(s), first at {tuple(int(i) for i in idx[0])}')

    def check(self, region=None):
        """all three checks; returns the logical output"""
        self.check_guards()
        self.assert_written(region)
        self.assert_finite(region)
        return self.t


def guarded_out(shape, dtype, device='cuda', fill=None):
    return GuardedOut(shape, dtype, device, fill)


def guarded_in(t, device='cuda'):
    """A device copy of `t` between NaN guards (the returned view keeps the whole allocation alive).  Integer inputs get
    0xFF guards."""
    g = guard_bytes(tuple(t.shape) or (1,), t.dtype)
    nbytes = t.numel() * t.element_size()
    buf = torch.empty(2 * g + nbytes, dtype=torch.uint8, device=device)
    if t.dtype in _NAN_BITS:
        ity, bits = _NAN_BITS[t.dtype]
        buf[:g].view(ity).fill_(bits)
        buf[g + nbytes:].view(ity).fill_(bits)
    else:
        buf[:g].fill_(0xFF)
        buf[g + nbytes:].fill_(0xFF)
    out = buf[g:g + nbytes].view(t.dtype).view(t.shape)
    out.copy_(t)
    return out


def _block_sums(x, block):
    """sum of x over each block of `block` (trailing partial blocks included)"""
    pads = []
    for s, b in zip(reversed(x.shape), reversed(block)):
        pads += [0, (-int(s)) % b]
    x = F.pad(x, pads)
    shape = []
    for s, b in zip(x.shape, block):
        shape += [int(s) // b, b]
    return x.reshape(shape).sum(dim=tuple(range(1, 2 * len(block), 2)))


def tile_err(got, ref, block=(32, 32)):
    """max over blocks of ||d_blk|| / max(||ref_blk||, 0.25 rms(ref) sqrt(n_blk)); `block` gives a size per dimension (the
    floor keeps blocks where the reference is nearly zero from judging rounding noise).  Evaluated in fp64 on got's device."""
    got = torch.as_tensor(got).detach()
    got, ref = got.to(torch.float64), torch.as_tensor(ref).detach().to(got.device, torch.float64)
    assert got.shape == ref.shape and len(block) == ref.dim(), (got.shape, ref.shape, block)
    d2 = _block_sums((got - ref) ** 2, block)
    r2 = _block_sums(ref ** 2, block)
    n = _block_sums(torch.ones_like(ref), block)
    rms = float(ref.pow(2).mean().sqrt())
    den = torch.maximum(r2.sqrt(), 0.25 * rms * n.sqrt()).clamp_min(1e-30)
    return float((d2.sqrt() / den).max())
